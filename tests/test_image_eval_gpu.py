"""gps_image_metrics (csrc/image_metrics.hip) and its two hosts against THE REFERENCE'S OWN NUMBERS: tests/golden/image_metrics_ref.npz
holds what scripts/utils/image_utils.py: psnr and scripts/utils/loss_utils.py: ssim return on scripts/metric_general.py:59-66's
operands, on float32 inputs (as the reference runs them) and on float64 inputs (tests/golden/make_image_metrics_golden.py).

Bounds, none of them taken from the kernel's output:
  * squared error of uint8 images: exact (int64), mse to 1 ulp of float64 (one correctly rounded division);
  * PSNR: 1e-4 dB.  A relative error d in the MSE moves the PSNR by 4.34 d dB; exact integer SSE, or fp32 squares summed in
    double, leave d at a few 2^-23; the bound is ~100 x that.  +inf is matched exactly;
  * SSIM: max(1e-5, 4 x |ssim_f32_ref - ssim_f64_ref|) per view, both values from the fixture: 1e-5 is the per-pixel bound the
    SSIM map is held to (tests/test_reference_python_pin.py) and a mean cannot exceed it; the second term is four times the
    rounding spread the reference's own float32 evaluation shows on that view.  Identical images and all-masked views: exactly 1."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("a", "b", "c", "d", "d_masked", "e")
_cache = {}


def _gold():
    if "gold" not in _cache:
        import os
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_metrics_ref.npz"))
        _cache["gold"] = {k: g[k] for k in g.files}
    return _cache["gold"]


def _case(name):
    g = _gold()
    return g[name + "_render"], g[name + "_gt"], g.get(name + "_depth")


def _T(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _unit(u8):
    """to_tensor's uint8 -> float32 .div(255), ON THE CPU: a true division (the device's division of a tensor by a Python scalar
    multiplies by the rounded reciprocal, which is another float for some levels)"""
    return torch.as_tensor(np.ascontiguousarray(u8)).to(torch.float32).div(255)


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


def _run(render, gt, depth=None):
    """the Python host on numpy or device inputs -> dict of numpy arrays (one device -> host copy per output)"""
    from gps_slam_amd import image_eval
    r = image_eval.image_metrics(render if torch.is_tensor(render) else _T(render), gt if torch.is_tensor(gt) else _T(gt),
                                 depth if torch.is_tensor(depth) else _T(depth))
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def _result(name):
    """every fixture case through the kernel ONCE, shared by the tests below"""
    if ("res", name) not in _cache:
        _cache[("res", name)] = _run(*_case(name))
    return _cache[("res", name)]


def _ssim_bound(name, k):
    g = _gold()
    return max(1e-5, 4.0 * abs(float(g[name + "_ssim_f32"][k]) - float(g[name + "_ssim_f64"][k])))


def _window(dtype):
    """loss_utils.py:46-54 restated: float32 taps, normalised, outer product, then the images' dtype"""
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().expand(3, 1, 11, 11).contiguous().to(dtype)


def _torch_metrics(render_u8, gt_u8, depth=None, dtype=torch.float64):
    """metric_general.py:59-66 as plain torch ops on the CPU, one view [H,W,3] uint8 -> (psnr, ssim)"""
    to_tensor = lambda a: torch.as_tensor(np.ascontiguousarray(a)).permute(2, 0, 1).contiguous().to(dtype).div(255).unsqueeze(0)
    a, b = to_tensor(render_u8), to_tensor(gt_u8)
    if depth is not None:
        m = torch.as_tensor(np.ascontiguousarray(depth))[None, None] > 0
        a, b = a * m, b * m
    mse = ((a - b) ** 2).mean()
    psnr = float(20 * torch.log10(1.0 / torch.sqrt(mse)))
    w = _window(dtype)
    conv = lambda t: F.conv2d(t, w, padding=5, groups=3)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return psnr, float(ssim.mean())


def _masked_u8(render, gt, depth, k):
    a, b = render[k].astype(np.int64), gt[k].astype(np.int64)
    if depth is not None:
        m = (depth[k] > 0)[..., None]
        a, b = a * m, b * m
    return a, b


# ---------------------------------------------------------------------------------------------- 1. exact SSE
@pytest.mark.parametrize("name", CASES)
def test_uint8_squared_error_is_exact_and_mse_is_its_quotient(name):
    render, gt, depth = _case(name)
    r = _result(name)
    assert r["sse_u8"].dtype == np.int64 and r["mse"].dtype == np.float64
    K, H, W = render.shape[:3]
    for k in range(K):
        a, b = _masked_u8(render, gt, depth, k)
        want = int(((a - b) ** 2).sum())
        assert int(r["sse_u8"][k]) == want, (name, k, int(r["sse_u8"][k]), want)
        want_mse = want / float(255 ** 2 * 3 * H * W)
        assert abs(r["mse"][k] - want_mse) <= np.spacing(want_mse), (name, k, r["mse"][k], want_mse)


# ---------------------------------------------------------------------------------------------- 2. PSNR against the reference
@pytest.mark.parametrize("name", CASES)
def test_psnr_matches_the_reference(name):
    g, r = _gold(), _result(name)
    for k, want in enumerate(g[name + "_psnr_f64"]):
        got = float(r["psnr"][k])
        print("%s[%d]: psnr %.9f dB, reference (float64) %.9f, (float32) %.9f" % (name, k, got, want, g[name + "_psnr_f32"][k]))
        if np.isinf(want):
            assert got == want, (name, k, got)
        else:
            assert abs(got - want) <= 1e-4, (name, k, got, want)
    finite = np.isfinite(g[name + "_psnr_f64"])
    if finite.all():
        assert abs(r["psnr_mean"] - g[name + "_psnr_f64"].mean()) <= 1e-4
    else:
        assert r["psnr_mean"] == float("inf")   # metric.py:60: the mean of a list with an +inf in it


# ---------------------------------------------------------------------------------------------- 3. SSIM against the reference
@pytest.mark.parametrize("name", CASES)
def test_ssim_matches_the_reference(name):
    g, r = _gold(), _result(name)
    assert r["ssim"].dtype == np.float64
    for k, want in enumerate(g[name + "_ssim_f64"]):
        got, bound = float(r["ssim"][k]), _ssim_bound(name, k)
        print("%s[%d]: ssim %.10f, reference (float64) %.10f, (float32) %.10f, |diff| %.3e, bound %.3e"
              % (name, k, got, want, g[name + "_ssim_f32"][k], abs(got - want), bound))
        assert abs(got - want) <= bound, (name, k, got, want, bound)
    assert abs(r["ssim_mean"] - g[name + "_ssim_f64"].mean()) <= max(_ssim_bound(name, k) for k in range(len(r["ssim"])))
    if name == "e":   # render == gt, and a depth that masks everything: C1 C2 / (C1 C2)
        assert r["ssim"][2] == 1.0 and r["ssim"][3] == 1.0, (r["ssim"][2] - 1.0, r["ssim"][3] - 1.0)
        assert r["mse"][2] == 0.0 and r["mse"][3] == 0.0 and r["sse_u8"][2] == 0 and r["sse_u8"][3] == 0


# ---------------------------------------------------------------------------------------------- 4. the operator's values
def test_ssim_sum_equals_the_sum_of_the_operators_map():
    """Case d_masked: gps_ssim_fwd (channels-last) on the / 255 float images, its map summed in float64, against ssim * 3 H W of
    the metrics kernel, within 1e-12 relative (only the order of the float64 additions differs).  The metrics kernel evaluates
    the expression through splat_ssim.hpp's value_as_operator, which spells out the floating-point contraction hipcc gives
    ssim_fwd_kernel: with the expression evaluated unfused the sums differed by 8.7e-10 relative.  The float32 input path on
    the very same tensors gives the uint8 path's sum bit for bit."""
    from gps_slam_amd import gsplat_ops
    render, gt, depth = _case("d_masked")
    H, W = render.shape[1:3]
    m = torch.as_tensor((depth[0] > 0).astype(np.float32))[..., None]
    a = (_unit(render[0]) * m).unsqueeze(0).contiguous().to(DEV)
    b = (_unit(gt[0]) * m).unsqueeze(0).contiguous().to(DEV)
    smap = gsplat_ops.fusedssim(0.01 ** 2, 0.03 ** 2, a, b, train=False, channels_last=True)[0]
    want = float(smap.double().sum())
    got = float(_result("d_masked")["ssim"][0]) * 3 * H * W
    print("metrics kernel sum %.12f, operator map sum %.12f, relative difference %.3e" % (got, want, abs(got - want) / want))
    rf = _run(a, b)
    assert float(rf["ssim"][0]) == float(_result("d_masked")["ssim"][0])
    assert abs(got - want) <= 1e-12 * want, (got, want, abs(got - want) / want)


# ---------------------------------------------------------------------------------------------- 5. batch and layout
def test_batch_equals_single_views_float_input_and_repeat_calls_bitwise():
    render, gt, depth = _case("e")
    r4 = _result("e")
    for k in range(4):
        r1 = _run(render[k:k + 1], gt[k:k + 1], depth[k:k + 1])
        for key in ("mse", "ssim", "sse_u8"):
            assert r1[key][0] == r4[key][k], (k, key, r1[key][0], r4[key][k])
    again = _run(render, gt, depth)
    for key in ("mse", "ssim", "sse_u8", "psnr"):
        assert np.array_equal(again[key], r4[key]), key
    # [H,W,3] with [H,W] and [H,W,1] depths are the K = 1 call
    one = _run(render[0], gt[0], depth[0])
    one1 = _run(render[0], gt[0], depth[0][..., None])
    for key in ("mse", "ssim", "sse_u8"):
        assert one[key].shape == (1,) and one[key][0] == r4[key][0] and one1[key][0] == r4[key][0], key
    # float32 input built as uint8 / 255: the same SSIM bit for bit, the MSE within 1e-6 relative (fp32 differences squared in
    # double against exact integers), no integer sum
    rf = _run(_unit(render).to(DEV), _unit(gt).to(DEV), depth)
    assert np.array_equal(rf["ssim"], r4["ssim"])
    assert np.all(np.abs(rf["mse"] - r4["mse"]) <= 1e-6 * r4["mse"]) and (rf["sse_u8"] == 0).all()
    assert rf["mse"][2] == 0.0 and rf["mse"][3] == 0.0 and np.isposinf(rf["psnr"][2:]).all()


def test_swapped_width_and_height_against_a_float64_torch_formulation():
    """case c transposed (65 x 33: three tile rows, two tile columns) guards the x / y tile indexing; the window is separable and
    symmetric, so the exact value is that of case c and the fixture's spread of case c bounds this view as well"""
    g = _gold()
    render, gt, _ = _case("c")
    rt, gtt = np.ascontiguousarray(render.transpose(0, 2, 1, 3)), np.ascontiguousarray(gt.transpose(0, 2, 1, 3))
    assert rt.shape == (1, 65, 33, 3)
    psnr64, ssim64 = _torch_metrics(rt[0], gtt[0])
    assert abs(ssim64 - float(g["c_ssim_f64"][0])) <= 1e-12 and abs(psnr64 - float(g["c_psnr_f64"][0])) <= 1e-9   # the formulation itself
    r = _run(rt, gtt)
    print("c swapped: psnr %.9f (float64 torch %.9f), ssim %.10f (%.10f)" % (r["psnr"][0], psnr64, r["ssim"][0], ssim64))
    assert abs(r["psnr"][0] - psnr64) <= 1e-4
    assert abs(r["ssim"][0] - ssim64) <= _ssim_bound("c", 0)
    assert int(r["sse_u8"][0]) == int(_result("c")["sse_u8"][0])


# ---------------------------------------------------------------------------------------------- 6. hosts agree
def test_cpp_host_and_python_host_return_equal_tensors():
    from gps_slam_amd import image_eval
    h = _host()
    render, gt, depth = (_T(x) for x in _case("e"))
    p = image_eval.image_metrics(render, gt, depth)
    c = h.imageMetrics(render, gt, depth)
    for key in ("psnr", "ssim", "mse", "sse_u8"):
        t = getattr(c, key)
        assert t.dtype == p[key].dtype and t.device == p[key].device and torch.equal(t, p[key]), key
    assert c.psnr_mean == p["psnr_mean"] == float("inf") and c.ssim_mean == p["ssim_mean"]
    c0, p0 = h.imageMetrics(render[:2], gt[:2]), image_eval.image_metrics(render[:2], gt[:2])   # no depth, finite means
    assert c0.psnr_mean == p0["psnr_mean"] and math.isfinite(c0.psnr_mean) and torch.equal(c0.ssim, p0["ssim"])
    assert torch.equal(h.imageMetrics(render[1], gt[1], depth[1]).ssim, p["ssim"][1:2])         # [H,W,3] and [H,W]
    # mismatches raise on both hosts
    for bad in ((render, gt[:3], None), (render, gt.float(), None), (render[..., :2], gt[..., :2], None), (render, gt, depth[:3]),
                (render, gt, depth.double()), (render.to(torch.int32), gt.to(torch.int32), None)):
        with pytest.raises(ValueError):
            image_eval.image_metrics(*bad)
        with pytest.raises(RuntimeError):
            h.imageMetrics(*bad)


# ---------------------------------------------------------------------------------------------- 7. pipeline
def test_pipeline_eval_images_on_the_cpp_host():
    """the 160 x 120, 31-frame orbit on the C++ host: evalImages against renderEvalImgs' own images and PSNR, the depth mask, the
    TSDF-colour source, the error paths; renderEvalImgs' output is what it was"""
    h = _host()
    W, Hh, n = 160, 120, 31
    seq = synth.make_sequence(W, Hh, n, step_deg=0.5)
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    rgb = torch.as_tensor(rgba).to(DEV)
    dep = torch.as_tensor(seq["depth"].astype(np.int16)).to(DEV)
    eng = h.ITMBasicEngine(W, Hh, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
    model = h.SLAMGaussianModel()
    model.loadConfig(dict(capacity=1 << 17))
    pipe = h.SLAMPipeline(eng, model, 7)
    for i in range(n):
        cam = h.Camera(W, Hh, seq["fx"], seq["fy"], seq["cx"], seq["cy"], True, torch.as_tensor(seq["c2w"][i].astype(np.float32)))
        cam.id = i
        cam.image, cam.depth = rgb[i][..., :3].float() / 255.0, (dep[i].float() / 1000.0).unsqueeze(-1)
        pipe.processFrame(i, cam, rgb[i], dep[i])
    torch.cuda.synchronize()
    assert model.getGaussianNum() > 100
    cams = pipe.optCams()[:2]
    assert len(cams) == 2
    ev = pipe.renderEvalImgs(cams)
    keys = [set(e) for e in ev]
    r = pipe.evalImages(cams)
    assert list(r.cam_ids) == [c.id for c in cams] and len(r.psnr) == 2 and len(r.ssim) == 2
    assert r.psnr_mean == r.metrics.psnr_mean and r.ssim_mean == r.metrics.ssim_mean
    assert abs(r.psnr_mean - sum(r.psnr) / 2) <= 1e-12 and abs(r.ssim_mean - sum(r.ssim) / 2) <= 1e-15
    for k in range(2):
        a8, b8 = ev[k]["rgb_u8"].cpu().numpy(), ev[k]["gt_u8"].cpu().numpy()
        assert abs(r.psnr[k] - float(ev[k]["psnr_u8"])) <= 1e-3, (k, r.psnr[k], float(ev[k]["psnr_u8"]))   # (that one is float32)
        _, s64 = _torch_metrics(a8, b8)
        _, s32 = _torch_metrics(a8, b8, dtype=torch.float32)
        bound = max(1e-5, 4.0 * abs(s32 - s64))
        print("view %d: psnr %.6f (renderEvalImgs %.6f), ssim %.9f (float64 torch %.9f, float32 %.9f, bound %.2e)"
              % (k, r.psnr[k], float(ev[k]["psnr_u8"]), r.ssim[k], s64, s32, bound))
        assert abs(r.ssim[k] - s64) <= bound, (k, r.ssim[k], s64, bound)
    stack = lambda key, evs: torch.stack([e[key] for e in evs])
    direct = h.imageMetrics(stack("rgb_u8", ev), stack("gt_u8", ev))
    assert torch.equal(direct.psnr, r.metrics.psnr) and torch.equal(direct.ssim, r.metrics.ssim) and torch.equal(direct.sse_u8, r.metrics.sse_u8)
    # depth mask: a 20 x 20 block of one camera's depth set to zero
    d = cams[0].depth.clone()
    d[40:60, 50:70] = 0.0
    cams[0].depth = d
    rm = pipe.evalImages(cams, depth_mask=True)
    want = h.imageMetrics(stack("rgb_u8", ev), stack("gt_u8", ev), torch.stack([c.depth for c in cams]))
    for key in ("psnr", "ssim", "mse", "sse_u8"):
        assert torch.equal(getattr(rm.metrics, key), getattr(want, key)), key
    assert abs(rm.psnr[0] - r.psnr[0]) > 1e-3, (rm.psnr[0], r.psnr[0])   # the mask acts
    # the TSDF-colour baseline
    rr = pipe.evalImages(cams, source="raycast_color")
    want = h.imageMetrics(stack("raycast_color_u8", ev), stack("gt_u8", ev))
    for key in ("psnr", "ssim", "mse", "sse_u8"):
        assert torch.equal(getattr(rr.metrics, key), getattr(want, key)), key
    assert not torch.equal(rr.metrics.sse_u8, r.metrics.sse_u8)
    # error paths
    with pytest.raises(RuntimeError):
        pipe.evalImages(cams, source="depth")
    no_depth = h.Camera(W, Hh, seq["fx"], seq["fy"], seq["cx"], seq["cy"], False, cams[1].c2w_slam.cpu())
    no_depth.id, no_depth.image = 99, cams[1].image
    no_depth.toGPU()
    assert len(pipe.evalImages([no_depth]).psnr) == 1
    with pytest.raises(RuntimeError):
        pipe.evalImages([cams[0], no_depth], depth_mask=True)
    no_image = h.Camera(W, Hh, seq["fx"], seq["fy"], seq["cx"], seq["cy"], True, cams[1].c2w_slam.cpu())
    no_image.toGPU()
    with pytest.raises(RuntimeError):
        pipe.evalImages([no_image])
    # renderEvalImgs is what it was
    ev2 = pipe.renderEvalImgs(cams)
    assert [set(e) for e in ev2] == keys
    for k in range(2):
        for key in ("rgb_u8", "gt_u8", "raycast_color_u8"):
            assert torch.equal(ev2[k][key], ev[k][key]), (k, key)
