"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads without a GPU,
and exports every symbol include/*.h declares (no compute calls here)."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = []
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        names += re.findall(r"GPS_API[^;(]*?\b(gps_\w+)\s*\(", open(h).read())
    return sorted(set(names))


def test_header_declares_the_path():
    names = _declared()
    for must in ("gps_proj_fwd", "gps_proj_bwd", "gps_sh_fwd", "gps_sh_bwd", "gps_isect_tiles_no_depth",
                 "gps_raster_ges_fwd", "gps_raster_ges_bwd_gs", "gps_compose_l1", "gps_adam_step"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from gps_slam_amd import _build, _lib
    so = _build.build()
    raw = ctypes.CDLL(so)
    for name in _declared():
        assert hasattr(raw, name), "libgpsslam_hip.so does not export %s" % name
        assert name in _lib.PROTOTYPES, "python binding lacks %s" % name
    lib = _lib.load_library()
    assert b"gfx950" in lib.gps_version()
    # the shipped library carries no probe switch and every tunable at its shipped value (A/B variants say what they are)
    assert lib.gps_build_flags() == b"", lib.gps_build_flags()


def test_tsdf_scratch_bytes_are_the_recorded_ones():
    """gps_tsdf_scratch_bytes is visible to callers (per-view scratch buffers, saved state): the layout function behind it must
    return what the library returned before the layout had one description (tests/golden/make_tsdf_scratch_bytes_golden.py:
    five image sizes x four table sizes, ragged and minimal ones included)."""
    import json
    from gps_slam_amd import _lib
    lib = _lib.load_library()
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "tsdf_scratch_bytes.json")))
    assert len(table["rows"]) == 20
    for w, h, n_buckets, n_excess, want in table["rows"]:
        assert lib.gps_tsdf_scratch_bytes(w, h, n_buckets, n_excess) == want, (w, h, n_buckets, n_excess)


def test_no_wrong_result_experiment_paths_in_the_product_kernels():
    """Timing experiments that produce wrong results live in tools/probe/ (or in the history), not behind macros in csrc/."""
    import re
    csrc = os.path.join(ROOT, "gps_slam_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        txt = open(os.path.join(csrc, f), errors="ignore").read()
        assert "wrong results" not in txt and not re.search(r"GPS_\w*EXPERIMENT", txt) and "GPS_RAYCAST_STATS" not in txt, f
        assert "getenv" not in txt, "%s: no environment overrides inside the kernel library" % f


def test_no_cpu_fallback_when_library_missing(tmp_path):
    from gps_slam_amd import _lib
    with pytest.raises(RuntimeError):
        _lib.load_library(str(tmp_path / "nope.so"))


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under gps_slam_amd/ may reference it."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "gps_slam_amd")):
        if "build" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "import oracle" not in txt and "from oracle" not in txt and "liboracle" not in txt, f


def test_cpp_host_layer_builds_loads_and_mirrors_the_reference_surface():
    """gps_slam_amd/host (C++/libtorch over the C-ABI) builds with g++ and exposes the reference's operator surface
    (gsplat/gsplat_wapper.hpp), model (include/raw_gs_model.h), engine and pipeline names.  No compute without a GPU."""
    from gps_slam_amd import _build, _build_host, _lib
    _build.build()
    _lib.load_library()
    _build_host.build()
    import gps_slam_amd._host as h
    for name in ("SphericalHarmonicsNew", "FullyFusedProjection", "RasterizeToPixelsGes_NewParallel", "isectTilesNoDepth",
                 "isectOffsetEncodeNoDepth", "distCUDA2", "simpleKNN", "degFromSh", "numShBases", "rgb2sh", "sh2rgb",
                 "Camera", "SLAMGaussianModel", "ITMBasicEngine", "SLAMPipeline"):
        assert hasattr(h, name), name
    assert [h.numShBases(d) for d in range(5)] == [1, 4, 9, 16, 25] and h.degFromSh(16) == 3
    import torch
    rgb = torch.tensor([[0.25, 0.5, 1.0]])
    assert torch.allclose(h.sh2rgb(h.rgb2sh(rgb)), rgb)
    m = h.SLAMGaussianModel()
    for meth in ("forward", "computeLoss", "trainStep", "initOptimizers", "optimizersStep", "optimizersZeroGrad",
                 "prunePoints", "addGaussians", "getGaussianNum"):
        assert hasattr(m, meth), meth
    # host-side pose algebra runs without a GPU: poseInv(c2w) @ c2w == I
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.3, -0.2, 1.5])
    c2w[:3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert torch.allclose(h.poseInv(c2w) @ c2w, torch.eye(4), atol=1e-6)


def test_gaussian_ply_format_is_the_reference_layout(tmp_path):
    """3DGS PLY of RawGaussianParams::savePly (raw_gs_param.cpp:159-217): header text, property order (f_rest channel-major),
    row size, raw parameters; host code only."""
    import numpy as np
    from gps_slam_amd.gs_model import gaussian_ply_properties, read_gaussian_ply, write_gaussian_ply
    rng = np.random.default_rng(0)
    n, K = 7, 16
    t = dict(means=rng.normal(size=(n, 3)), scales=rng.normal(size=(n, 3)), quats=rng.normal(size=(n, 4)),
             featuresDc=rng.normal(size=(n, 3)), featuresRest=rng.normal(size=(n, K - 1, 3)), opacities=rng.normal(size=(n, 1)))
    t = {k: v.astype(np.float32) for k, v in t.items()}
    path = str(tmp_path / "g.ply")
    write_gaussian_ply(path, t["means"], t["scales"], t["quats"], t["featuresDc"], t["featuresRest"], t["opacities"])
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n")
    lines = head.decode().split("\n")
    props = gaussian_ply_properties(3, 45)
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 7"]
    assert lines[3:-1] == ["property float " + p for p in props] and len(props) == 62
    assert props[:9] == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] and props[9] == "f_rest_0"
    assert props[54:] == ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    rows = np.frombuffer(body, "<f4").reshape(n, 62)
    assert np.array_equal(rows[:, :3], t["means"]) and not rows[:, 3:6].any()
    # f_rest_j for j < 15 is colour channel 0 of SH coefficient j + 1 (transpose(1, 2) before the flatten)
    assert np.array_equal(rows[:, 9:24], t["featuresRest"][:, :, 0]) and np.array_equal(rows[:, 24:39], t["featuresRest"][:, :, 1])
    assert np.array_equal(rows[:, 54], t["opacities"][:, 0]) and np.array_equal(rows[:, 58:], t["quats"])
    back = read_gaussian_ply(path)
    for k in t:
        assert np.array_equal(back[k], t[k]), k


def test_gaussian_ply_of_both_hosts_is_the_golden_file_byte_for_byte(tmp_path):
    """RawGaussianParams::savePly (src/raw_gs_param.cpp:159-217) against tests/golden/gaussian_ply_n2_k16.ply -- a file written
    by tests/golden/make_gaussian_ply_golden.py from the reference writer's property list and row order with nothing of this
    package imported (data, not a self-comparison): the C++ host's savePly and the Python mirror's must both produce exactly
    those 2,022 bytes from the same tensors, and the reader must give the tensors back."""
    import numpy as np
    import torch
    from gps_slam_amd import _build, _build_host, _lib
    from gps_slam_amd.gs_model import read_gaussian_ply, write_gaussian_ply
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    want = open(os.path.join(gdir, "gaussian_ply_n2_k16.ply"), "rb").read()
    t = dict(np.load(os.path.join(gdir, "gaussian_ply_n2_k16.npz")))
    assert len(want) == 2022 and want.count(b"\n", 0, want.index(b"end_header")) == 3 + 62
    write_gaussian_ply(str(tmp_path / "p.ply"), t["means"], t["scales"], t["quats"], t["featuresDc"], t["featuresRest"], t["opacities"])
    assert open(tmp_path / "p.ply", "rb").read() == want
    _build.build()
    _lib.load_library()
    _build_host.build()
    import gps_slam_amd._host as h
    p = h.SLAMGaussianModel().getGaussianParms()   # (host tensors: savePly is host code, raw_gs_param.cpp copies to the CPU first)
    p.add([torch.as_tensor(t[k]) for k in ("means", "scales", "quats", "featuresDc", "featuresRest", "opacities")])
    p.savePly(str(tmp_path / "c.ply"))
    assert open(tmp_path / "c.ply", "rb").read() == want
    back = read_gaussian_ply(str(tmp_path / "c.ply"))
    for k in t:
        assert np.array_equal(back[k].reshape(t[k].shape), t[k]), k


def test_adam_scalars_of_both_hosts_are_the_reference_optimisers():
    """The doubles libtorch's torch::optim::Adam runs with when it is constructed the way RawGaussianModel::initOptimizers
    constructs it (src/raw_gs_model.cpp:661-671: eps, betas and rates pass through float variables) -- read back from the
    library itself (oracle/libtorch_adam.cpp) -- are what the Python host hands to the kernels, and the C++ host's source carries
    the same literals; three steps of the library on the CPU agree with a float32 restatement that uses them (and NOT with one
    that uses 0.9 / 0.999 / 1e-15, which rounds 1-5 passed: the second moment differs by 1.3e-5 relative)."""
    import numpy as np
    import torch
    from gps_slam_amd import gs_model
    from oracle import libtorch_adam_build
    mod = libtorch_adam_build.load()
    eps, b1, b2 = mod.RefAdam.scalars()
    assert (b1, b2, eps) == (0.8999999761581421, 0.9990000128746033, 1.0000000036274937e-15)
    assert (gs_model.ADAM_BETA1, gs_model.ADAM_BETA2, gs_model.ADAM_EPS) == (b1, b2, eps)
    src = open(os.path.join(ROOT, "gps_slam_amd", "host", "raw_gs_model.cpp")).read()
    assert "kAdamBeta1 = (double)0.9f" in src and "kAdamBeta2 = (double)0.999f" in src and "kAdamEps = (double)1e-15f" in src
    gen = torch.Generator().manual_seed(0)
    p0 = torch.randn((4096, 3), generator=gen)
    lr = float(np.float32(5e-3))
    ref = mod.RefAdam([p0], [lr])
    f = np.float32

    def restated(beta1, beta2, eps_):
        p, m, v = p0.numpy().copy(), np.zeros((4096, 3), f), np.zeros((4096, 3), f)
        g_ = torch.Generator().manual_seed(1)
        for step in (1, 2, 3):
            g = (torch.randn((4096, 3), generator=g_) * 1e-3).numpy()
            m = (m * f(beta1) + g * f(1.0 - beta1)).astype(f)
            v = (v * f(beta2) + (g * g).astype(f) * f(1.0 - beta2)).astype(f)
            denom = (np.sqrt(v) / f(np.sqrt(1.0 - beta2 ** step)) + f(eps_)).astype(f)
            p = (p - f(lr / (1.0 - beta1 ** step)) * (m / denom).astype(f)).astype(f)
        return p, v
    g_ = torch.Generator().manual_seed(1)
    for step in (1, 2, 3):
        ref.step([torch.randn((4096, 3), generator=g_) * 1e-3])
    v_lib = ref.exp_avg_sq()[0].numpy()
    p_new, v_new = restated(b1, b2, eps)
    p_old, v_old = restated(0.9, 0.999, 1e-15)
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    assert rel(v_new, v_lib) < 5e-7, rel(v_new, v_lib)            # a few float32 ulps (CPU ATen fuses differently)
    assert rel(v_old, v_lib) > 5e-6, rel(v_old, v_lib)            # the 1.3e-5 of (1 - 0.999) vs (1 - 0.999f)
    assert float(np.abs(p_new - ref.parameters()[0].numpy()).max()) < 1e-6
