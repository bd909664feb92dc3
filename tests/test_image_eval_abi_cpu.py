"""CPU-side checks of the image-quality evaluation surface (no GPU): the two C-ABI symbols exist with the declared prototypes,
the size query and the argument checks behave as the header says (nothing is launched: every call here has null pointers), both
hosts export the surface, and the fixture tests/golden/image_metrics_ref.npz (written by tests/golden/make_image_metrics_golden.py
from the reference's scripts/utils/image_utils.py and loss_utils.py) is what a float64 restatement of the PSNR says it is."""
import ctypes
import inspect
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_metrics_ref.npz")
CASES = ("a", "b", "c", "d", "d_masked", "e")


def test_c_abi_exports_the_image_metrics_entry_points_with_the_declared_prototypes():
    from gps_slam_amd import _build, _lib
    raw = ctypes.CDLL(_build.build())
    i32, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    want = {"gps_image_metrics_workspace_bytes": (i64, [i32, i32, i32]),
            "gps_image_metrics": (i32, [i32, i32, i32, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp])}
    for name, sig in want.items():
        assert hasattr(raw, name), name
        assert _lib.PROTOTYPES[name] == sig, name
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gps_slam_hip.h")).read()
    assert "GPS_API int64_t gps_image_metrics_workspace_bytes(int K, int H, int W);" in hdr
    assert "GPS_API int gps_image_metrics(int K, int H, int W, int dtype, const void *render, const void *gt, const float *depth," in hdr
    assert "#define GPS_IMAGE_U8 0" in hdr and "#define GPS_IMAGE_F32 1" in hdr


def test_workspace_size_query_is_negative_for_bad_sizes_and_monotone():
    from gps_slam_amd import _lib
    lib = _lib.load_library()
    q = lib.gps_image_metrics_workspace_bytes
    for bad in ((0, 480, 640), (1, 0, 640), (1, 480, 0), (-1, 480, 640), (1, -5, 640), (1, 480, -7)):
        assert q(*bad) < 0, bad
    assert q(1, 1, 1) > 0
    sizes = (1, 5, 31, 32, 33, 64, 65, 480, 640, 1200)
    for k in (1, 2, 16):
        for i, h in enumerate(sizes):
            for j, w in enumerate(sizes):
                assert q(k, h, w) > 0
                assert q(k + 1, h, w) >= q(k, h, w)
                if i + 1 < len(sizes):
                    assert q(k, sizes[i + 1], w) >= q(k, h, w)
                if j + 1 < len(sizes):
                    assert q(k, h, sizes[j + 1]) >= q(k, h, w)
    assert q(16, 480, 640) == 16 * q(1, 480, 640)           # one slot per tile and view
    assert q(1, 33, 65) == 6 * q(1, 32, 32)                 # 2 x 3 tiles


def test_every_bad_argument_is_refused_before_any_launch():
    """all pointers that are not the one under test are either null too or a dummy that is never dereferenced: every call
    must return GPS_ERR_ARG (-1) from the argument checks"""
    from gps_slam_amd import _lib
    lib = _lib.load_library()
    f = lib.gps_image_metrics
    P = 4096                                                  # a non-null, 8-byte aligned address nobody reads
    ws = int(lib.gps_image_metrics_workspace_bytes(2, 45, 70))
    ok = dict(K=2, H=45, W=70, dtype=0, render=P, gt=P, depth=None, workspace=P, workspace_bytes=ws, mse=P, ssim=P, sse_u8=P)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["K"], a["H"], a["W"], a["dtype"], a["render"], a["gt"], a["depth"], a["workspace"], a["workspace_bytes"],
                 a["mse"], a["ssim"], a["sse_u8"], None)

    for kw in (dict(K=0), dict(K=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-2),                    # sizes
               dict(dtype=2), dict(dtype=-1),                                                          # unknown dtype
               dict(render=None), dict(gt=None),                                                       # null images
               dict(mse=None), dict(ssim=None), dict(sse_u8=None),                                     # null outputs
               dict(workspace=None), dict(workspace_bytes=ws - 1), dict(workspace_bytes=0)):           # missing / short workspace
        assert call(**kw) == -1, kw
    # with everything null the first failing check decides as well
    assert f(0, 0, 0, 7, None, None, None, None, 0, None, None, None, None) == -1
    assert f(1, 8, 8, 0, None, None, None, None, 0, None, None, None, None) == -1


def test_both_hosts_export_the_surface():
    from gps_slam_amd import _build, _build_host, _lib, image_eval
    _build.build()
    _lib.load_library()
    _build_host.build()
    import gps_slam_amd._host as h
    sig = inspect.signature(image_eval.image_metrics)
    assert list(sig.parameters) == ["render", "gt", "depth"] and sig.parameters["depth"].default is None
    assert callable(h.imageMetrics)
    doc = h.imageMetrics.__doc__
    for name in sig.parameters:
        assert name in doc, name
    for field in ("psnr", "ssim", "mse", "sse_u8", "psnr_mean", "ssim_mean"):
        assert hasattr(h.ImageMetrics, field), field
    for field in ("psnr", "ssim", "psnr_mean", "ssim_mean", "cam_ids", "metrics"):
        assert hasattr(h.ImageEvalResult, field), field
    doc = h.SLAMPipeline.evalImages.__doc__
    assert "cams" in doc and "depth_mask: bool = False" in doc and "source: str = 'rgb'" in doc, doc
    # the Python pipeline has no renderEvalImgs and therefore no evalImages (image_eval's docstring says so)
    from gps_slam_amd.slam_pipeline import SLAMPipeline
    assert not hasattr(SLAMPipeline, "renderEvalImgs") and not hasattr(SLAMPipeline, "evalImages")
    assert "evalImages" in image_eval.__doc__
    # wrong shapes / dtypes are refused on the host, before the device is touched
    import torch
    with pytest.raises(ValueError):
        image_eval.image_metrics(torch.zeros(4, 4, 3), torch.zeros(4, 4, 3))            # not on the device
    with pytest.raises(RuntimeError):
        h.imageMetrics(torch.zeros(4, 4, 3), torch.zeros(4, 4, 3))


def _psnr_f64(render, gt, depth):
    """image_utils.py:19-21 on metric_general.py:59-64's operands, float64 numpy"""
    a, b = render.astype(np.float64) / 255.0, gt.astype(np.float64) / 255.0
    if depth is not None:
        m = (depth > 0)[..., None]
        a, b = a * m, b * m
    mse = ((a - b) ** 2).mean()
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(1.0 / np.sqrt(mse))


def test_fixture_is_what_a_float64_restatement_of_the_psnr_says():
    g = np.load(GOLD)
    sizes = {"a": (1, 11, 5), "b": (1, 32, 32), "c": (1, 33, 65), "d": (1, 45, 70), "d_masked": (1, 45, 70), "e": (4, 45, 70)}
    n_inf = 0
    for case in CASES:
        render, gt = g[case + "_render"], g[case + "_gt"]
        depth = g[case + "_depth"] if case + "_depth" in g.files else None
        assert render.dtype == np.uint8 and gt.dtype == np.uint8 and render.shape == sizes[case] + (3,) == gt.shape
        assert (depth is None) == (case in "abcd")
        for k in range(render.shape[0]):
            want = float(g[case + "_psnr_f64"][k])
            got = _psnr_f64(render[k], gt[k], None if depth is None else depth[k])
            if np.isinf(want):
                assert want > 0 and got == want, (case, k)
                n_inf += 1
            else:
                assert abs(got - want) <= 1e-9, (case, k, got, want)
            # the reference's float32 run stays close to its float64 run (these spreads set the GPU test's SSIM bound)
            assert 0.0 < g[case + "_ssim_f64"][k] <= 1.0
            assert abs(g[case + "_ssim_f32"][k] - g[case + "_ssim_f64"][k]) < 2e-5
    assert n_inf == 2                                           # e: identical images, and everything masked
    assert tuple(g["e_ssim_f64"][2:]) == (1.0, 1.0) and tuple(g["e_ssim_f32"][2:]) == (1.0, 1.0)
    # the mask acts, and zeroing is not excluding (the parity trap of csrc/image_metrics.hip)
    d = g["d_masked_depth"][0]
    assert np.isnan(d).any() and (d < 0).any() and (d[0] == 0).all() and (d[25:39, 22:42] > 0).sum() == 0
    assert np.array_equal(g["e_render"][0], g["d_render"][0]) and np.array_equal(g["e_depth"][0], d, equal_nan=True)
    masked, unmasked = float(g["d_masked_psnr_f64"][0]), float(g["d_psnr_f64"][0])
    assert masked - unmasked > 0.3
    keep = d > 0
    a, b = g["d_render"][0].astype(np.float64) / 255.0, g["d_gt"][0].astype(np.float64) / 255.0
    excluded = 20.0 * np.log10(1.0 / np.sqrt(((a - b)[keep] ** 2).mean()))
    assert abs(excluded - masked) > 0.3, (excluded, masked)
