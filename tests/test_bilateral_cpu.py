"""The bilateral depth filter (ITMLibSettings::useBilateralFilter) without a device: the two new exports exist with the declared
signatures and report every argument error before any device work, the TSDF.use_bilateral_filter key on both config routes, the
Python default, and the fixture (tests/golden/bilateral.npz, written by tests/golden/make_bilateral_golden.py): its inputs
regenerate, its own conditions hold, and the float32 transcription of the filter reproduces the reference's images."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from tests import bilateral_cases as cases
from tests.digests import crc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bilateral.npz")


def _lib():
    from gps_slam_amd import _build, _lib
    _build.build()
    return _lib.load_library()


def _host():
    from gps_slam_amd import _build_host
    _lib()
    _build_host.build()
    import gps_slam_amd._host as h
    return h


def test_c_abi_exports_the_entry_points_with_the_declared_signatures():
    from gps_slam_amd import _build, _lib
    raw = ctypes.CDLL(_build.build())
    i32, i64, vp, S = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(_lib.TsdfState)
    want = {"gps_tsdf_filter_scratch_bytes": (i64, [i32, i32]),
            "gps_tsdf_convert_filter_depth": (i32, [S, vp, vp, vp])}
    for name, sig in want.items():
        assert hasattr(raw, name), name
        assert _lib.PROTOTYPES[name] == sig, name


def test_scratch_size():
    lib = _lib()
    assert int(lib.gps_tsdf_filter_scratch_bytes(100, 52)) == 2 * 100 * 52 * 4   # two float images
    assert int(lib.gps_tsdf_filter_scratch_bytes(4, 7)) == 2 * 4 * 7 * 4
    assert int(lib.gps_tsdf_filter_scratch_bytes(40000, 40000)) == 2 * 40000 * 40000 * 4   # past 2^31
    for w, h in ((0, 52), (100, 0), (-1, 52), (100, -7)):
        assert int(lib.gps_tsdf_filter_scratch_bytes(w, h)) < 0, (w, h)


def test_argument_errors_come_before_any_device_work():
    from gps_slam_amd._lib import TsdfState
    lib = _lib()
    buf = np.zeros(64, np.float32)   # host memory nothing may touch before the checks
    p = buf.ctypes.data
    s = TsdfState()
    s.width, s.height, s.depth = 16, 12, p
    S = ctypes.byref(s)
    f = lib.gps_tsdf_convert_filter_depth
    assert f(None, p, p, None) == -1
    assert f(S, None, p, None) == -1
    assert f(S, p, None, None) == -1
    assert f(S, p + 1, p, None) == -1          # int16 image on an odd address
    for off in (1, 2, 3):
        assert f(S, p, p + off, None) == -1    # float scratch off its alignment
    for w, h in ((0, 12), (16, 0), (-16, 12), (16, -12)):
        bad = TsdfState()
        bad.width, bad.height, bad.depth = w, h, p
        assert f(ctypes.byref(bad), p, p, None) == -1, (w, h)
    no_depth = TsdfState()
    no_depth.width, no_depth.height = 16, 12
    assert f(ctypes.byref(no_depth), p, p, None) == -1
    off_depth = TsdfState()
    off_depth.width, off_depth.height, off_depth.depth = 16, 12, p + 2
    assert f(ctypes.byref(off_depth), p, p, None) == -1
    assert not buf.any()


BASE = "voxel_size: 0.01\ntrunc_dist: 0.04\nviewFrustum_min: 0.2\nviewFrustum_max: 10.0\nuse_gt_pose: false\n"


def test_use_bilateral_filter_key_of_the_tsdf_node():
    h = _host()
    assert h.tsdfConfigUseBilateralFilter(h.parse_yaml(BASE)) is False          # the absent key: every shipped config
    assert h.tsdfConfigUseBilateralFilter(h.parse_yaml(BASE + "use_bilateral_filter: true\n")) is True
    assert h.tsdfConfigUseBilateralFilter(h.parse_yaml(BASE + "use_bilateral_filter: false\n")) is False
    for wrong in ("5", "maybe", "[1, 2]"):
        with pytest.raises(Exception):
            h.tsdfConfigUseBilateralFilter(h.parse_yaml(BASE + "use_bilateral_filter: %s\n" % wrong))
    with pytest.raises(Exception):   # a closed key list
        h.tsdfConfigUseBilateralFilter(h.parse_yaml(BASE + "use_bilateral_filtre: true\n"))
    # the other readers of the node take the key too, and it changes nothing of theirs
    both = h.parse_yaml(BASE + "use_bilateral_filter: true\nuse_approximate_raycast: true\n")
    assert h.tsdfConfigUseApproximateRaycast(both) is True and h.tsdfConfigUseBilateralFilter(both) is True
    assert h.tsdfConfigUseApproximateRaycast(h.parse_yaml(BASE + "use_bilateral_filter: true\n")) is False
    assert h.tsdfConfigFailureMode(h.parse_yaml(BASE + "use_bilateral_filter: true\n")) == h.FailureMode.FAILUREMODE_IGNORE
    for name in ("setUseBilateralFilter", "usesBilateralFilter", "hasFilterScratch"):
        assert hasattr(h.ITMBasicEngine, name), name


def test_use_bilateral_filter_key_on_the_flat_route():
    """PIPE.TSDF folded into one namespace by config.flatten (typed by PIPE_KEYS) and read by createTsdfEngine's flat reader"""
    from gps_slam_amd import config
    h = _host()
    text = "PIPE:\n  TSDF:\n" + "".join("    " + line + "\n" for line in BASE.splitlines())
    flat = lambda extra: config.flatten(config.parse_yaml(text + extra)["PIPE"])
    assert "use_bilateral_filter" not in flat("")
    assert h.tsdfConfigUseBilateralFilterFlat(flat("")) is False
    on = flat("    use_bilateral_filter: true\n")
    assert on["use_bilateral_filter"] is True and h.tsdfConfigUseBilateralFilterFlat(on) is True
    off = flat("    use_bilateral_filter: false\n")
    assert off["use_bilateral_filter"] is False and h.tsdfConfigUseBilateralFilterFlat(off) is False
    for wrong in ("5", "maybe"):
        with pytest.raises(config.ConfigError):
            flat("    use_bilateral_filter: %s\n" % wrong)
    assert config.PIPE_KEYS["use_bilateral_filter"] is config.Scalar.as_bool


def test_python_default_is_off():
    from gps_slam_amd.tsdf_engine import TsdfEngine
    assert inspect.signature(TsdfEngine.__init__).parameters["use_bilateral_filter"].default is False


def test_fixture_inputs_regenerate_and_its_conditions_hold():
    G = np.load(GOLD)
    assert os.path.getsize(GOLD) < 500000
    assert sorted(G["kernel_names"]) == sorted(cases.KERNEL_CASES) and sorted(G["run_names"]) == sorted(cases.RUNS)
    for tag, (W, H) in cases.KERNEL_CASES.items():
        assert (int(G[tag + "_W"]), int(G[tag + "_H"])) == (W, H)
        assert crc(cases.kernel_depth(tag)) == G[tag + "_input_crc"], tag
    for tag in cases.RUNS:
        seq = cases.sequence(tag)
        got = np.array([crc(seq["rgb"]), crc(seq["depth"]), crc(seq["c2w"])], np.uint32)
        assert np.array_equal(got, G[tag + "_input_crc"]), tag
    # what the GPU tests rely on (the generator refuses to write the fixture otherwise)
    mm = cases.kernel_depth("k100x52")
    W, H = cases.KERNEL_CASES["k100x52"]
    ref, conv = G["k100x52_filtered"], cases.convert(mm)
    st = {}
    cases.filter_pass(conv, st)
    assert st["denormal_weights"] == int(G["k_denormal_weights_pass1"]) > 0
    assert st["zero_weights"] == int(G["k_zero_weights_pass1"]) > 0
    hole = conv < 0
    assert hole[2, 2:W - 2].any() or hole[H - 3, 2:W - 2].any() or hole[2:H - 2, 2].any() or hole[2:H - 2, W - 3].any()
    inner = ~cases.ring_mask(H, W)
    assert (inner & (ref >= 0) & (ref != conv)).any()
    for v in (200, 10000, 1):
        assert (mm == v).any()
    # the exponential: the pinned expf was called, and plain glibc's differs on some pixels -- recorded as data
    assert int(G["k100x52_expf_calls"]) > 0 and int(G["k4x7_expf_calls"]) == 0
    assert 0 < int(G["glibc_diff_pixels"]) < int(G["glibc_filtered_pixels"]) and int(G["glibc_diff_max_ulp"]) >= 1


@pytest.mark.parametrize("tag", sorted(cases.KERNEL_CASES))
def test_transcription_reproduces_the_reference(tag):
    """conversion + five passes in float32 numpy with (float) exp((double) e): bit-equal to the reference's view builder linked
    against the correctly rounded expf; ring 0.0 (+0), holes -1"""
    G = np.load(GOLD)
    W, H = cases.KERNEL_CASES[tag]
    mm = cases.kernel_depth(tag)
    got, ref = cases.filter5(mm), G[tag + "_filtered"]
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    ring = cases.ring_mask(H, W)
    assert (ref[ring].view(np.uint32) == 0).all()
    assert ((cases.convert(mm) < 0)[~ring] == (ref[~ring] == -1)).all()
    if tag == "k4x7":
        assert (ref.view(np.uint32) == 0).all()
    if tag == "k5x5":
        assert ref[2, 2] > 0 and np.count_nonzero(ref) == 1
