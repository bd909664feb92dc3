"""The approximate raycast (ITMLibSettings::useApproximateRaycast) without a device: the far-from-point-cloud decision of
gps_track_far_from_point_cloud against the reference engine's own decisions (tests/golden/forward_render.npz, written by
tests/golden/make_forward_render_golden.py) and at the three rule edges, the TSDF.use_approximate_raycast key of
createTsdfEngine's node, and the fixture's inputs regenerated from its stored parameters."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import synth
from tests.digests import crc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_render.npz")


def _lib():
    from gps_slam_amd import _build, _lib
    _build.build()
    return _lib


def _far(L, M, pc_M, age):
    ts = L.TrackState()
    L.check(L.lib.gps_track_state_reset(C.byref(ts)), "gps_track_state_reset")
    ts.pose_M[:] = np.asarray(M, np.float32).reshape(-1).tolist()
    ts.pose_pc_M[:] = np.asarray(pc_M, np.float32).reshape(-1).tolist()
    ts.age_point_cloud = int(age)
    diff = C.c_float(-1.0)
    r = L.lib.gps_track_far_from_point_cloud(C.byref(ts), C.byref(diff))
    assert r in (0, 1), r
    return r, np.float32(diff.value)


def test_far_test_reproduces_the_reference_decisions():
    """every (pose, cloud pose, age before the frame) row of the given-pose sequences and of the tracked run: the reference took
    the forward branch exactly when the function says 'not far', and the squared distance is the reference's float, bit for bit"""
    L = _lib()
    G = np.load(GOLD)
    rows = 0
    for tag in list(G["names"]) + ["t"]:
        prep, n = G[tag + "_prep"], int(G[tag + "_n_frames"])
        pc = np.eye(4, dtype=np.float32).T.reshape(-1)   # ITMTrackingState::Reset
        for f in range(n):
            if (tag + "_pc_M") in G.files:
                assert np.array_equal(G[tag + "_pc_M"][f], pc), (tag, f)   # the cloud pose follows the full casts
            far, diff = _far(L, G[tag + "_M"][f], pc, prep[f, 0])
            assert far == 1 - int(prep[f, 2]), (tag, f, far, prep[f])
            assert diff.view(np.uint32) == np.float32(G[tag + "_diff"][f]).view(np.uint32), (tag, f, diff, G[tag + "_diff"][f])
            if far:
                pc = G[tag + "_M"][f]
            rows += 1
    assert rows == 32
    # both rules are in the fixture (the generator refuses to write it otherwise)
    a, b = G["a_prep"], G["b_prep"]
    assert (a[:, 0] > 5).any() and ((b[:, 0] >= 0) & (b[:, 0] <= 5) & (G["b_diff"] > 0.0005) & (b[:, 2] == 0)).any()


def test_far_test_rule_edges():
    L = _lib()
    eye = np.eye(4, dtype=np.float32)
    assert _far(L, eye, eye, -1)[0] == 1 and _far(L, eye, eye, -2)[0] == 1     # no point cloud yet
    assert _far(L, eye, eye, 0)[0] == 0 and _far(L, eye, eye, 5)[0] == 0
    assert _far(L, eye, eye, 6)[0] == 1                                        # older than 5 frames
    # the distance rule is `diff > 0.0005f`: with R = I the centre is -T and diff = tx * tx exactly.  0.0005f is not a square
    # of a float; the floats around its root square to one value below and one above it.
    thr = np.float32(0.0005)
    t = np.float32(np.sqrt(np.float64(thr)))
    lo = t if np.float32(t * t) <= thr else np.nextafter(t, np.float32(0))
    hi = np.nextafter(lo, np.float32(1))
    assert np.float32(lo * lo) <= thr < np.float32(hi * hi)
    for tx, want in ((lo, 0), (hi, 1)):
        M = eye.copy().T.reshape(-1)   # ORUtils layout m[col * 4 + row]: the translation is m[12..14]
        M[12] = tx
        far, diff = _far(L, M, eye.reshape(-1), 3)
        assert far == want and diff == np.float32(tx * tx), (tx, far, diff)
    # a rotated pair with the same centre is not far: centre = -R^T T
    c, s = np.float32(np.cos(0.3)), np.float32(np.sin(0.3))
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    centre = np.array([0.25, -0.5, 1.0], np.float32)
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = R
    M[:3, 3] = -(R @ centre)
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, 3] = -centre
    far, diff = _far(L, M.T.reshape(-1), T0.T.reshape(-1), 0)
    assert far == 0 and diff < 1e-12


def test_use_approximate_raycast_key_of_the_tsdf_node():
    from gps_slam_amd import _build_host
    _lib().load_library()
    _build_host.build()
    import gps_slam_amd._host as h
    base = "voxel_size: 0.01\ntrunc_dist: 0.04\nviewFrustum_min: 0.2\nviewFrustum_max: 10.0\nuse_gt_pose: false\n"
    assert h.tsdfConfigUseApproximateRaycast(h.parse_yaml(base)) is False          # the absent key: every shipped config
    assert h.tsdfConfigUseApproximateRaycast(h.parse_yaml(base + "use_approximate_raycast: true\n")) is True
    assert h.tsdfConfigUseApproximateRaycast(h.parse_yaml(base + "use_approximate_raycast: false\n")) is False
    with pytest.raises(Exception):   # a closed key list
        h.tsdfConfigUseApproximateRaycast(h.parse_yaml(base + "use_aproximate_raycast: true\n"))
    # the other reader of the node takes the key too
    assert h.tsdfConfigFailureMode(h.parse_yaml(base + "use_approximate_raycast: true\n")) == h.FailureMode.FAILUREMODE_IGNORE
    for name in ("setUseApproximateRaycast", "usesApproximateRaycast", "agePointCloud", "runRaycast", "GetLiveImage",
                 "GetForwardProjection", "forwardMissingPoints"):
        assert hasattr(h.ITMBasicEngine, name), name


def test_python_engine_has_the_option_and_the_abi_entries():
    L = _lib()
    import inspect
    from gps_slam_amd.tsdf_engine import TsdfEngine
    assert inspect.signature(TsdfEngine.__init__).parameters["use_approximate_raycast"].default is False
    for name in ("gps_tsdf_forward_block_bytes", "gps_tsdf_forward_project", "gps_tsdf_forward_fill", "gps_tsdf_forward_render",
                 "gps_tsdf_forward_missing", "gps_track_far_from_point_cloud", "gps_tsdf_prepare", "gps_tsdf_frame_map_fwd",
                 "gps_tsdf_process_frame_fwd", "gps_tsdf_render_colour_from", "gps_tsdf_render_live"):
        assert name in L.PROTOTYPES and getattr(L.lib, name) is not None, name
    assert int(L.lib.gps_tsdf_forward_block_bytes(100, 75)) == 24 * 7500 + 64
    assert int(L.lib.gps_tsdf_forward_block_bytes(0, 75)) < 0


def test_fixture_inputs_regenerate_from_its_parameters():
    G = np.load(GOLD)
    assert os.path.getsize(GOLD) < 500000
    for tag in list(G["names"]) + ["t"]:
        W, H, n = int(G[tag + "_W"]), int(G[tag + "_H"]), int(G[tag + "_n_frames"])
        seq = synth.make_sequence(W, H, n, step_deg=float(G[tag + "_step_deg"]))
        got = np.array([crc(seq["rgb"]), crc(seq["depth"]), crc(seq["c2w"])], np.uint32)
        assert np.array_equal(got, G[tag + "_input_crc"]), (tag, got, G[tag + "_input_crc"])
    assert (int(G["a_W"]), int(G["a_H"]), int(G["b_W"]), int(G["b_H"])) == (100, 75, 64, 48)
