"""The approximate raycast (ITMLibSettings::useApproximateRaycast: forward projection of the last full cast + rays for the holes)
on the device, against the REFERENCE's own CPU engine with the option on (tests/golden/forward_render.npz, written by
tests/golden/make_forward_render_golden.py): bit for bit with given poses, within the tracker's tolerance with the tracker on."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import synth
from tests.digests import crc, engine_getter, frame_digest
from tests.test_oracle_tsdf import bits_equal, check_frame

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "forward_render.npz"))
SMALL = dict(n_blocks=0x2000, n_buckets=0x4000, n_excess=0x1000)   # capacities of the engine that fuses nothing


@functools.lru_cache(maxsize=None)
def _sequence(tag):
    W, H, n = int(G[tag + "_W"]), int(G[tag + "_H"]), int(G[tag + "_n_frames"])
    seq = synth.make_sequence(W, H, n, step_deg=float(G[tag + "_step_deg"]))
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    return seq, torch.as_tensor(rgba).to(DEV), torch.as_tensor(seq["depth"].astype(np.int16)).to(DEV)


def _engine(tag, **kw):
    from gps_slam_amd.tsdf_engine import TsdfEngine
    seq = _sequence(tag)[0]
    return TsdfEngine(seq["W"], seq["H"], seq["fx"], seq["fy"], seq["cx"], seq["cy"], float(G["voxel"]), float(G["mu"]),
                      float(G["vf_min"]), float(G["vf_max"]), device=DEV, **kw)


def _project_only(eng, M):
    """gps_tsdf_forward_project at pose M into a block of its own -> (forward projection before the hole fill, count, sorted list)"""
    from gps_slam_amd._lib import check, lib
    P = eng.W * eng.H
    block = torch.zeros((int(lib.gps_tsdf_forward_block_bytes(eng.W, eng.H)) + 3) // 4, dtype=torch.int32, device=DEV)
    check(lib.gps_tsdf_forward_project(C.byref(eng.state), block.data_ptr(), M.ctypes.data, eng._stream()), "gps_tsdf_forward_project")
    n = C.c_int32(-1)
    lst = np.zeros(P, np.int32)
    check(lib.gps_tsdf_forward_missing(C.byref(eng.state), block.data_ptr(), C.byref(n), lst.ctypes.data, P, eng._stream()),
          "gps_tsdf_forward_missing")
    b = block.cpu().numpy()
    return b[:4 * P].view(np.float32).reshape(eng.H, eng.W, 4), int(n.value), np.sort(lst[:n.value]), b[4 * P:5 * P]


def _run_given_poses(tag, check=True):
    """the sequence through the Python mirror with the option on -> per forward frame the forward projection (host copy)"""
    from tests.test_tsdf_gpu import EngineView
    seq, rgb, dep = _sequence(tag)
    W, H, n = seq["W"], seq["H"], int(G[tag + "_n_frames"])
    eng = _engine(tag, use_approximate_raycast=True)
    v = EngineView(eng)
    prep, out = G[tag + "_prep"], {}
    for f in range(n):
        M, invM = eng.ProcessFrame(rgb[f], dep[f], seq["c2w"][f])
        forward = bool(prep[f, 2])
        if forward:
            out[f] = eng.GetForwardProjection().cpu().numpy().copy()
        if not check:
            continue
        assert bits_equal(M, G[tag + "_M"][f]) and bits_equal(invM, G[tag + "_invM"][f])
        assert eng.age_pointCloud == int(prep[f, 1]), (f, eng.age_pointCloud, prep[f])
        assert (eng.age_pointCloud > 0) == forward
        # every engine digest: a forward frame leaves the last full cast, the ICP maps and the visible types alone, and the next
        # allocation sees the reference's visible list
        got = frame_digest(engine_getter(v), f, W, H)
        for k, val in got.items():
            assert np.array_equal(np.asarray(val), G["%s_%s@%d" % (tag, k, f)]), (tag, k, f)
        eng.runRaycast()
        assert crc(eng.GetLiveImage().cpu().numpy()) == G[tag + "_live_crc"][f], (tag, f, "live re-render")
        if not forward:
            continue
        cnt, lst = eng.forwardMissingPoints()
        assert cnt == int(prep[f, 3]) and crc(lst) == G[tag + "_missing_crc"][f], (tag, f, cnt, prep[f])
        assert crc(out[f]) == G[tag + "_fwd_crc"][f], (tag, f, "forward projection after the hole fill")
        pre, pcnt, plst, _ = _project_only(eng, M)
        assert pcnt == cnt and np.array_equal(plst, lst)
        assert crc(pre) == G[tag + "_fwd_pre_crc"][f], (tag, f, "forward projection before the hole fill")
        if f == int(G[tag + "_full_frame"]):
            assert np.array_equal(lst, G[tag + "_full_missing"])
            assert bits_equal(pre, G[tag + "_full_fwd_pre"]) and bits_equal(out[f], G[tag + "_full_fwd"])
            assert int(prep[f, 4]) > 0   # targets with more than one source: the winner rule is pinned here
    assert int(v._c()[5]) == 0  # no rendering-block overflow
    return out


@pytest.mark.parametrize("tag", ["a", "b"])
def test_given_pose_run_is_bit_equal_to_the_reference(tag):
    out = _run_given_poses(tag)
    assert sorted(out) == [f for f in range(int(G[tag + "_n_frames"])) if G[tag + "_prep"][f, 2]]


def test_scatter_is_deterministic():
    """the same sequence twice in one process: the forward projections are bit-identical (the winner of a target is a rule, not
    a race)"""
    a, b = _run_given_poses("a", check=False), _run_given_poses("a", check=False)
    assert sorted(a) == sorted(b) and len(a) >= 6
    for f in a:
        assert bits_equal(a[f], b[f]), f


def test_hole_fill_equals_the_dense_cast():
    """on a forward frame, the pixels of the missing list hold what gps_tsdf_raycast(update_visible = 0) writes for them at the
    same pose from the same min/max image"""
    from gps_slam_amd._lib import TsdfState, check, lib
    for tag in ("a", "b"):
        seq, rgb, dep = _sequence(tag)
        eng = _engine(tag, use_approximate_raycast=True)
        full = int(G[tag + "_full_frame"])
        for f in range(full + 1):
            M, invM = eng.ProcessFrame(rgb[f], dep[f], seq["c2w"][f])
        assert eng.age_pointCloud > 0
        cnt, lst = eng.forwardMissingPoints()
        assert cnt == int(G[tag + "_prep"][full, 3]) > 0
        s = TsdfState.from_buffer_copy(eng.state)
        s.fv_minmax = eng.minmax.data_ptr()   # the free-view slot of a copy of the state: the live min/max image, another ray image
        vis_before = eng.visible_type.clone()
        check(lib.gps_tsdf_raycast(C.byref(s), invM.ctypes.data, 1, 0, eng._stream()), "gps_tsdf_raycast")
        dense = eng.fv_raycast.cpu().numpy().reshape(-1, 4)
        fwd = eng.GetForwardProjection().cpu().numpy().reshape(-1, 4)
        assert bits_equal(fwd[lst], dense[lst]), tag
        assert (fwd[lst, 3] > 0).any() and torch.equal(vis_before, eng.visible_type)


def test_option_off_is_the_old_path():
    """the new entry points without a block reproduce the digests of an existing golden exactly as gps_tsdf_process_frame does:
    through the Python mirror (gps_tsdf_process_frame_fwd, NULL block) and through gps_tsdf_frame_map_fwd with the flag set but
    no block"""
    from gps_slam_amd._lib import TrackState, check, lib
    from gps_slam_amd.tsdf_engine import TsdfEngine, pose_from_c2w
    from tests.test_tsdf_gpu import EngineView
    g = np.load(os.path.join(HERE, "golden", "tsdf_64x48_v20mm.npz"))
    get = lambda k, f: g["%s@%d" % (k, f)]
    W, H = int(g["W"]), int(g["H"])
    mk = lambda: TsdfEngine(W, H, float(g["fx"]), float(g["fy"]), float(g["cx"]), float(g["cy"]), float(g["voxel"]), float(g["mu"]),
                            float(g["vf_min"]), float(g["vf_max"]))
    eng, raw = mk(), mk()
    ts = TrackState()
    check(lib.gps_track_state_reset(C.byref(ts)), "gps_track_state_reset")
    for f in range(g["rgb"].shape[0]):
        rgb, dep = torch.as_tensor(g["rgb"][f]).to(DEV), torch.as_tensor(g["depth"][f].astype(np.int16)).to(DEV)
        eng.ProcessFrame(rgb, dep, g["c2w"][f])
        check_frame(EngineView(eng), get, f, window_only=True)
        assert eng.age_pointCloud == (-2 if f == 0 else 0) and eng.GetForwardProjection() is None
        M, invM = pose_from_c2w(g["c2w"][f])
        rgba = torch.cat([rgb, torch.full_like(rgb[..., :1], 255)], -1).contiguous() if rgb.shape[-1] == 3 else rgb
        raw.state.rgb = rgba.data_ptr()
        ts.pose_M[:] = M.tolist(); ts.pose_invM[:] = invM.tolist()
        check(lib.gps_tsdf_convert_depth(C.byref(raw.state), dep.data_ptr(), raw._stream()), "gps_tsdf_convert_depth")
        check(lib.gps_tsdf_frame_map_fwd(C.byref(raw.state), C.byref(ts), 1, 0, None, 1, raw._stream()), "gps_tsdf_frame_map_fwd")
        torch.cuda.synchronize()
        check_frame(EngineView(raw), get, f, window_only=True)
        assert ts.age_point_cloud == (-2 if f == 0 else 0) and bits_equal(np.array(ts.pose_pc_M, np.float32), M)


def test_tracked_run_takes_the_reference_branches():
    """tracker on, option on (160 x 120: the reference's own tracker answers NaN poses at 100 x 75, see the generator): the
    branch sequence is the reference's and the poses agree within the tolerance of test_tracked_process_frame_matches_reference_poses
    (tree against scan-order sums: 2e-5 on every matrix entry)"""
    tag = "t"
    seq, rgb, dep = _sequence(tag)
    eng = _engine(tag, use_approximate_raycast=True)
    eng.turnOnTracking()
    prep = G[tag + "_prep"]
    assert prep[:, 2].sum() >= 6 and (prep[:, 0] > 5).any()
    for f in range(int(G[tag + "_n_frames"])):
        M, invM = eng.ProcessFrameTracked(rgb[f], dep[f])
        assert eng.age_pointCloud == int(prep[f, 1]), (f, eng.age_pointCloud, prep[f].tolist())
        err = max(np.abs(M - G[tag + "_M"][f]).max(), np.abs(invM - G[tag + "_invM"][f]).max())
        print("frame %d: branch %d, pose error %.3g" % (f, prep[f, 2], err))
        assert err < 2e-5, (f, err)
        if prep[f, 2]:
            print("   missing %d (reference %d)" % (eng.forwardMissingPoints()[0], prep[f, 3]))


def test_cpp_host_equals_python_mirror():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    tag = "b"
    seq, rgb, dep = _sequence(tag)
    eng_p = _engine(tag, use_approximate_raycast=True)
    eng_c = h.ITMBasicEngine(seq["W"], seq["H"], seq["fx"], seq["fy"], seq["cx"], seq["cy"], float(G["voxel"]), float(G["mu"]),
                             float(G["vf_min"]), float(G["vf_max"]))
    eng_c.turnOffTracking()
    assert eng_c.usesApproximateRaycast() is False
    eng_c.setUseApproximateRaycast(True)
    eng_c.runRaycast()   # before the first frame: nothing to render
    forward_frames = 0
    for f in range(int(G[tag + "_n_frames"])):
        eng_c.pushGtPose(torch.as_tensor(seq["c2w"][f].astype(np.float32)))
        eng_c.ProcessFrame(rgb[f], dep[f])
        eng_p.ProcessFrame(rgb[f], dep[f], seq["c2w"][f])
        eng_c.runRaycast(); eng_p.runRaycast()
        assert eng_c.agePointCloud() == eng_p.age_pointCloud == int(G[tag + "_prep"][f, 1])
        assert torch.equal(eng_c.GetLiveImage(), eng_p.GetLiveImage())
        assert crc(eng_c.GetLiveImage().cpu().numpy()) == G[tag + "_live_crc"][f]
        assert torch.equal(eng_c.GetLiveVertex().view(-1), eng_p.raycast.view(-1))
        if G[tag + "_prep"][f, 2]:
            forward_frames += 1
            assert torch.equal(eng_c.GetForwardProjection().view(torch.int32), eng_p.GetForwardProjection().view(torch.int32))
            n_c, lst_c = eng_c.forwardMissingPoints()
            n_p, lst_p = eng_p.forwardMissingPoints()
            assert n_c == n_p == int(G[tag + "_prep"][f, 3]) and np.array_equal(np.sort(lst_c.numpy()), lst_p)
    assert forward_frames == 4


def _restate_forward_projection(rays, M, voxel, fx, fy, cx, cy, W, H):
    """forwardProjectPixel + the scan-order scatter of ForwardRender_common in float32 numpy, operation for operation; a
    non-finite image coordinate is dropped (the documented decision) -> (forward projection [H,W,4], winner [H*W])"""
    f32 = np.float32
    p = rays.reshape(-1, 4).astype(f32)
    M = M.astype(f32)
    vs = f32(voxel)
    with np.errstate(all="ignore"):
        x, y, z = p[:, 0] * vs, p[:, 1] * vs, p[:, 2] * vs
        one = f32(1.0)
        px = ((M[0] * x + M[4] * y) + M[8] * z) + M[12] * one
        py = ((M[1] * x + M[5] * y) + M[9] * z) + M[13] * one
        pz = ((M[2] * x + M[6] * y) + M[10] * z) + M[14] * one
        u = (f32(fx) * px) / pz + f32(cx)
        v = (f32(fy) * py) / pz + f32(cy)
        keep = ~((u < 0) | (u > f32(W - 1)) | (v < 0) | (v > f32(H - 1))) & ~np.isnan(u) & ~np.isnan(v)
        t = np.where(keep, (np.where(keep, u, 0) + f32(0.5)).astype(np.int32) + (np.where(keep, v, 0) + f32(0.5)).astype(np.int32) * W, -1)
    winner = np.full(W * H, -1, np.int32)
    for i in np.nonzero(keep)[0]:   # scan order: a later source overwrites an earlier one
        winner[t[i]] = i
    fwd = np.zeros((W * H, 4), f32)
    fwd[winner >= 0] = p[winner[winner >= 0]]
    return fwd.reshape(H, W, 4), winner


def test_degenerate_and_border_sources():
    """a hand-made ray image through gps_tsdf_forward_project: a point at the camera centre (0 / 0: NaN coordinates), points
    behind the camera, points that project to exactly W - 1 / H - 1 and just past them, two sources on one target.  Expected
    values: the float32 restatement above, which is first checked against the reference's stored scatter of a real frame.
    (forwardProjectPixel has no test of z: a point behind the camera whose MIRRORED projection falls inside the image is written,
    by the reference and here; the ones whose projection falls outside leave nothing.)"""
    from gps_slam_amd.tsdf_engine import TsdfEngine
    # the restatement against the reference's own scatter (fixture: one forward frame of sequence b in full)
    tag = "b"
    seq, rgb, dep = _sequence(tag)
    eng = _engine(tag, use_approximate_raycast=True)
    full = int(G[tag + "_full_frame"])
    for f in range(full + 1):
        M, _ = eng.ProcessFrame(rgb[f], dep[f], seq["c2w"][f])
    assert crc(eng.raycast.cpu().numpy().reshape(seq["H"], seq["W"], 4)) == G["%s_raycast@%d" % (tag, full)]   # the reference's last full cast
    want, _ = _restate_forward_projection(eng.raycast.cpu().numpy(), M, float(G["voxel"]), seq["fx"], seq["fy"], seq["cx"], seq["cy"],
                                          seq["W"], seq["H"])
    assert bits_equal(want, G[tag + "_full_fwd_pre"])

    # the hand-made image: identity pose, power-of-two voxel size and intrinsics, so the coordinates below are exact
    W, H, voxel, fx, cx, cy = 40, 30, 0.03125, 32.0, 16.0, 8.0
    e = TsdfEngine(W, H, fx, fx, cx, cy, voxel, 0.125, 0.2, 10.0, device=DEV, **SMALL)
    cam = lambda x, y, z, w=1.0: [x / voxel, y / voxel, z / voxel, w]
    up = lambda a, k: np.nextafter(np.float32(a), np.float32(np.inf)) if k == 1 else up(np.nextafter(np.float32(a), np.float32(np.inf)), k - 1)
    xr, yb = (W - 1 - cx) / fx, (H - 1 - cy) / fx   # camera x / y at z = 1 of the last column / row: 0.71875, 0.65625
    rays = np.zeros((H * W, 4), np.float32)         # everything else: points AT the camera centre (0 / 0)
    src = {
        5: cam(0.0, 0.0, 1.0),               # the principal point: target (16, 8)
        6: cam(0.0, 0.0, 2.0, 0.0),          # the same target from a ray that found nothing (w = 0), later in scan order: it wins
        50: cam(xr, 0.0, 1.0),               # exactly u = W - 1
        51: cam(0.0, yb, 1.0),               # exactly v = H - 1
        52: cam(xr, yb, 1.0),                # the last pixel
        60: cam(float(up(xr, 4)), 0.0, 1.0),     # just past W - 1
        61: cam(0.0, float(up(yb, 4)), 1.0),     # just past H - 1
        62: cam(-0.5 - 1e-3, 0.0, 1.0),          # just left of u = 0
        70: cam(1.0, 0.0, -1.0),             # behind the camera, mirrored projection u = -16: nothing
        71: cam(0.0, 1.0, -2.0),             # behind the camera, v = -8: nothing
        72: cam(-0.25, 0.0, -1.0),           # behind the camera, mirrored projection (24, 8) INSIDE: written, as the reference does
        80: cam(0.0, 0.0, 0.0),              # the camera centre with w = 1
        H * W - 1: cam(0.26, -0.2, 1.0),     # an ordinary point from the last source
    }
    for i, p in src.items():
        rays[i] = p
    e.raycast.copy_(torch.as_tensor(rays.reshape(-1)).to(DEV))
    M = np.eye(4, dtype=np.float32).reshape(-1)
    got, cnt, lst, winner = _project_only(e, M)
    want, want_winner = _restate_forward_projection(rays, M, voxel, fx, fx, cx, cy, W, H)
    assert bits_equal(got, want) and np.array_equal(winner, want_winner)
    t = lambda x, y: x + y * W
    hit = {t(16, 8): 6, t(W - 1, 8): 50, t(16, H - 1): 51, t(W - 1, H - 1): 52, t(24, 8): 72, t(24, 2): H * W - 1}
    assert {int(k): int(want_winner[k]) for k in np.nonzero(want_winner >= 0)[0]} == hit   # nothing else was written
    # (the min/max image of a fresh engine is empty: min > max everywhere, so no pixel is missing)
    assert cnt == 0 and lst.size == 0
