"""CPU-side checks of the relocaliser's C ABI (no GPU): the symbols exist with the declared signatures, every argument error is
reported before any device work, the host-side pieces -- the Gaussian coefficients and the default fern table -- are what the
header says (the coefficients: the reference's own, tests/golden/reloc_fern.npz), and the fixture's inputs regenerate."""
import ctypes
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reloc_fern.npz")


def _lib():
    from gps_slam_amd import _build, _lib
    _build.build()
    return _lib.load_library()


def test_c_abi_exports_the_relocaliser_with_the_declared_signatures():
    from gps_slam_amd import _build, _lib
    raw = ctypes.CDLL(_build.build())
    i32, f32, vp, u64 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint64
    want = {"gps_reloc_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, i32, f32, f32, f32, i32, u64]),
            "gps_reloc_destroy": (i32, [vp]),
            "gps_reloc_set_ferns": (i32, [vp, vp, vp, i32, vp]),
            "gps_reloc_process_frame": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
            "gps_reloc_read_result": (i32, [vp, ctypes.POINTER(_lib.RelocResult), vp]),
            "gps_reloc_retrieve_pose": (i32, [vp, i32, vp, vp, vp, vp]),
            "gps_reloc_export": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
            "gps_reloc_import": (i32, [vp, i32, vp, vp, vp, vp]),
            "gps_reloc_default_ferns": (i32, [i32, i32, i32, i32, f32, f32, u64, vp, vp]),
            "gps_reloc_gaussian_taps": (i32, [f32, i32, vp, vp])}
    for name, sig in want.items():
        assert hasattr(raw, name), name
        assert _lib.PROTOTYPES[name] == sig, name
    assert ctypes.sizeof(_lib.RelocResult) == 48   # added_id, n_found, ids[4], distances[4], n_entries, overflow


def test_argument_errors_come_before_any_device_work():
    lib = _lib()
    h = ctypes.c_void_p()
    ok = (64, 48, 500, 4, 0.2, 3.0, 0.2, 16, 0)
    assert lib.gps_reloc_create(None, *ok) == -1
    for bad in ((64, 48, 500, 4, 0.2, 3.0, 0.2, 0, 0),        # zero capacity
                (64, 48, 500, 4, 0.2, 3.0, 0.2, -3, 0),
                (31, 48, 500, 4, 0.2, 3.0, 0.2, 16, 0),       # no fern area: width / 32 == 0
                (64, 31, 500, 4, 0.2, 3.0, 0.2, 16, 0),
                (2048, 2048, 500, 4, 0.2, 3.0, 0.2, 16, 0),   # the 1/16 image would not fit the blur's workgroup
                (64, 48, 0, 4, 0.2, 3.0, 0.2, 16, 0),
                (64, 48, 500, 0, 0.2, 3.0, 0.2, 16, 0),
                (64, 48, 500, 8, 0.2, 3.0, 0.2, 16, 0),       # a code is one byte, and the reference's is a signed one
                (64, 48, 500, 4, 3.0, 0.2, 0.2, 16, 0)):      # empty depth range
        assert lib.gps_reloc_create(ctypes.byref(h), *bad) == -1, bad
        assert not h.value
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    from gps_slam_amd._lib import RelocResult
    res = RelocResult()
    # a NULL state is an argument error everywhere, whatever the other arguments are
    assert lib.gps_reloc_destroy(None) == -1
    assert lib.gps_reloc_info(None, p) == -1
    assert lib.gps_reloc_set_ferns(None, p, p, 2000, None) == -1
    assert lib.gps_reloc_get_ferns(None, p, p, 2000) == -1
    assert lib.gps_reloc_set_debug_outputs(None, None, None) == -1
    # (k outside 1..4 and a fern count that differs from the state's need a live state to be told apart from this error: a state
    # cannot be created without a device, so tests/test_reloc_fern_gpu.py::test_argument_checks_on_a_live_state holds those two)
    assert lib.gps_reloc_process_frame(None, p, p, p, 0, 1, 1, None) == -1
    assert lib.gps_reloc_read_result(None, ctypes.byref(res), None) == -1
    assert lib.gps_reloc_retrieve_pose(None, 0, p, p, None, None) == -1
    assert lib.gps_reloc_export(None, 0, None, None, None, p, None, None) == -1
    assert lib.gps_reloc_import(None, 0, None, None, None, None) == -1
    assert lib.gps_reloc_check_guards(None, None) == -1


def test_gaussian_coefficients_are_the_references():
    from gps_slam_amd import relocaliser as RL
    _lib()
    g = np.load(GOLD)
    taps = RL.gaussian_taps(2.5)
    assert taps.shape == (17,) and taps.dtype == np.float32
    assert np.array_equal(taps.view(np.uint32), g["coeff"].view(np.uint32))   # createGaussianFilter(17, 2.5f) of the reference, bit for bit
    assert taps[8] == 1.0 and np.array_equal(taps, taps[::-1])
    lib = _lib()
    n = ctypes.c_int(0)
    out = np.zeros(32, np.float32)
    assert lib.gps_reloc_gaussian_taps(2.5, 16, out.ctypes.data, ctypes.addressof(n)) == -1     # 17 taps do not fit 16
    assert lib.gps_reloc_gaussian_taps(0.0, 32, out.ctypes.data, ctypes.addressof(n)) == -1
    assert lib.gps_reloc_gaussian_taps(2.5, 32, None, ctypes.addressof(n)) == -1


def test_default_fern_table_follows_the_reference_sampling_rule():
    from gps_slam_amd import relocaliser as RL
    _lib()
    xy, thr = RL.default_ferns(320, 240, 500, 4, (0.2, 5.0), seed=7)
    assert xy.shape == (2000, 2) and thr.shape == (2000,)
    # locations in imgSize / 32 (10 x 7), not in the imgSize / 16 image the code reads (20 x 15): the reference's rule, quirk included
    assert xy[:, 0].min() == 0 and xy[:, 0].max() == 9 and xy[:, 1].min() == 0 and xy[:, 1].max() == 6
    assert thr.min() >= 0.2 and thr.max() < 5.0 and thr.min() < 0.3 and thr.max() > 4.9
    # uniform: every location is drawn about 2000 / 70 times (6 sigma of a binomial)
    counts = np.bincount(xy[:, 0] + 10 * xy[:, 1], minlength=70)
    assert np.all(np.abs(counts - 2000 / 70) <= 6 * np.sqrt(2000 / 70))
    again = RL.default_ferns(320, 240, 500, 4, (0.2, 5.0), seed=7)
    other = RL.default_ferns(320, 240, 500, 4, (0.2, 5.0), seed=8)
    assert np.array_equal(again[0], xy) and np.array_equal(again[1], thr)
    assert not np.array_equal(other[0], xy) and not np.array_equal(other[1], thr)
    # the fixture's tables are this generator's (thresholds rounded to the six digits of the reference's ferns.txt)
    g = np.load(GOLD)
    assert np.array_equal(g["q_fern_xy"], xy) and np.allclose(g["q_fern_thr"], thr, rtol=1e-5, atol=0)
    small = RL.default_ferns(64, 48, 500, 4, (0.2, 5.0), seed=7)[0]
    assert small[:, 0].max() == 1 and small[:, 1].max() == 0   # 64 x 48: a 2 x 1 fern area


def test_fixture_inputs_regenerate_and_hold_the_cases_the_gpu_tests_name():
    from tests import reloc_cases as cases
    g = np.load(GOLD)
    specs = [tuple(s) for s in g["q_specs"]]
    a = cases.frame_depth(320, 240, specs[1], int(g["hole_seed"]))
    b = cases.frame_depth(320, 240, specs[1], int(g["hole_seed"]))
    assert a.dtype == np.float32 and a.shape == (240, 320) and np.array_equal(a, b)
    blocks = a.reshape(15, 16, 20, 16).max(axis=(1, 3))
    assert (blocks == 0).any() and 0.03 < (a == 0).mean() < 0.2        # whole 16 x 16 blocks of holes, and scattered ones
    kinds = g["q_specs"][:, 0]
    assert (kinds == 1).sum() == 1 and (kinds == 2).sum() == 1         # one empty frame, one probe plane
    assert len(set(specs)) < len(specs)                                # identical frames
    tie = int(g["q_tie_frame"])
    assert int(g["q_added"].sum()) >= 3 and (g["q_harvest"] == 0).any()
    assert g["q_dist3"][tie, 0] == g["q_dist3"][tie, 1] and g["q_nn3"][tie, 0] > g["q_nn3"][tie, 1] >= 0
    assert any((g["q_nn3"][i] == -1).any() for i in g["q_few_frames"])
    assert any(g["q_added"][i] == 0 and g["q_dist1"][i] <= g["threshold"] for i in g["q_near_frames"])
    # the saved database is the reference's text: config.txt names its parameters, poses.txt counts the keyframes
    cfg = bytes(g["q_file_config"]).decode()
    assert cfg == "type=rgb,levels=4,numFerns=500,numDecisionsPerFern=1,harvestingThreshold=0.2", cfg
    assert bytes(g["q_file_poses"]).decode().split("\n")[0] == str(int(g["q_added"].sum()))
