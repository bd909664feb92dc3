"""The engine's failure modes on the device (C++ host, ITMBasicEngine.tpp:286-366): twelve tracked 320 x 240 frames with verdicts
forced through forceTrackerResult, the counterpart of the reference's ITMForceFailTracker."""
import functools

import numpy as np
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu
W, H, N = 320, 240, 12
FAIL = 1   # the frame whose tracking is declared lost; frame 0 is a keyframe by then


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


@functools.lru_cache(maxsize=None)
def _frames():
    seq = synth.make_sequence(W, H, N, step_deg=0.5)
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    return seq, torch.as_tensor(rgba).cuda(), torch.as_tensor(seq["depth"].astype(np.int16)).cuda()


def _engine(mode=None):
    h = _host()
    seq = _frames()[0]
    eng = h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
    if mode is not None:
        eng.setFailureMode(getattr(h.FailureMode, mode))
    return eng


def _visible_blocks(eng):
    """hash slots of the live visible list that hold a block.  Slot 0 may be listed without holding one: the raycaster marks
    entry vmIndex - 1 visible and a cache hit leaves vmIndex at 1 -- the reference's quirk, kept (csrc/tsdf_render.hip); nothing
    else may be."""
    vis = set(eng.visibleIds().cpu().numpy().tolist())
    held = set(eng.allocatedSlots().cpu().numpy().tolist())
    assert vis - held <= {0}, sorted(vis - held)[:8]
    return vis & held


def _step(eng, f):
    _, rgba, depth = _frames()
    eng.ProcessFrame(rgba[f], depth[f])
    return dict(pose=eng.lastPose().numpy().copy(), counters=eng.counters().cpu().numpy()[:3].copy(), frames=eng.framesProcessed,
                count=eng.relocalisationCount, fused=eng.lastFrameFused(), result=eng.trackerResult())


@functools.lru_cache(maxsize=None)
def _plain_run():
    """the default engine, nothing forced: the poses and volume counters every other run is compared with"""
    eng = _engine()
    return [_step(eng, f) for f in range(N)]


def test_ignore_mode_does_not_look_at_verdicts():
    h = _host()
    eng = _engine()
    assert eng.failureMode() == h.FailureMode.FAILUREMODE_IGNORE
    for f in (3, 5, 6):
        eng.forceTrackerResult(f, h.TrackingResult.TRACKING_FAILED)
    eng.forceTrackerResult(8, h.TrackingResult.TRACKING_POOR)
    plain = _plain_run()
    for f in range(N):
        got = _step(eng, f)
        assert np.array_equal(got["pose"], plain[f]["pose"]) and np.array_equal(got["counters"], plain[f]["counters"]), f
        assert got["fused"] and got["frames"] == f + 1 and got["result"] == h.TrackingResult.TRACKING_GOOD
    assert not eng.hasRelocaliser() and eng.relocalisationCount == 0


def test_relocalise_mode_with_good_tracking_fuses_every_frame_as_the_default_does():
    """nothing forced: the two halves of the frame (frame_track, frame_map) give the poses and counters of the one-call path, and the
    relocaliser harvests on the way without changing them"""
    eng = _engine("FAILUREMODE_RELOCALISE")
    plain = _plain_run()
    for f in range(N):
        got = _step(eng, f)
        assert np.array_equal(got["pose"], plain[f]["pose"]) and np.array_equal(got["counters"], plain[f]["counters"]), f
        assert got["fused"] and got["frames"] == f + 1 and got["count"] == 0
    assert eng.hasRelocaliser() and eng.relocaliserEntries() >= 1
    assert np.array_equal(eng.relocaliserPose(0).numpy(), plain[0]["pose"])   # frame 0 is the first keyframe, with its pose


def test_relocalise_mode_restarts_from_the_keyframe_and_holds_fusion_until_the_count_has_run_down():
    h = _host()
    R = h.TrackingResult
    eng = _engine("FAILUREMODE_RELOCALISE")
    eng.forceTrackerResult(FAIL, R.TRACKING_FAILED)
    for f in range(FAIL + 1, N):
        eng.forceTrackerResult(f, R.TRACKING_GOOD)
    plain = _plain_run()
    before = [_step(eng, f) for f in range(FAIL)]
    for f in range(FAIL):
        assert np.array_equal(before[f]["pose"], plain[f]["pose"]) and before[f]["fused"]
    n_kf = eng.relocaliserEntries()
    assert n_kf >= 1
    allocated = set(eng.allocatedSlots().cpu().numpy().tolist())
    blocks_before, frames_before = before[-1]["counters"][0], before[-1]["frames"]
    assert len(allocated) > 100

    # the failing frame: relocalised to the nearest keyframe, tracked again from its pose, not fused
    lost = _step(eng, FAIL)
    kf = eng.lastRelocalisedTo
    assert 0 <= kf < n_kf and eng.relocaliserEntries() == n_kf       # a failed frame is never harvested
    assert lost["count"] == 10 and not lost["fused"]
    assert lost["result"] == R.TRACKING_GOOD                         # the second TrackCamera's verdict (no thresholds set)
    kf_pose = eng.relocaliserPose(kf)
    assert np.array_equal(kf_pose.numpy(), plain[0]["pose"]) if kf == 0 else True
    # ... its pose is the keyframe's, refined by that second TrackCamera: the same step on a second engine in the same state
    twin = _engine("FAILUREMODE_RELOCALISE")
    for f in range(FAIL):
        _step(twin, f)
    twin.convertDepth(_frames()[2][FAIL])
    want = twin.relocaliseFromPose(kf_pose).numpy()
    assert np.array_equal(lost["pose"], want), np.abs(lost["pose"] - want).max()
    assert not np.array_equal(lost["pose"], kf_pose.numpy())         # (the tracker did move it)

    # GOOD frames count down from 10; until 0 nothing is allocated or fused, and the visible list holds old blocks only
    seen = [lost]
    for f in range(FAIL + 1, N):
        got = _step(eng, f)
        seen.append(got)
        want_count = 10 - (f - FAIL)
        assert got["count"] == want_count, (f, got["count"])
        if want_count > 0:
            assert not got["fused"] and got["frames"] == frames_before and got["counters"][0] == blocks_before, f
            assert set(eng.allocatedSlots().cpu().numpy().tolist()) == allocated, f
            assert len(eng.visibleIds()) == got["counters"][2] > 0, f
            blocks = _visible_blocks(eng)
            assert len(blocks) > 100 and blocks <= allocated, f   # every block it lists was allocated before the failure
        else:
            assert got["fused"] and got["frames"] == frames_before + 1, f
    assert seen[-1]["count"] == 0 and seen[-1]["fused"]                # 12 frames: the last one is the first to fuse again
    assert seen[-1]["counters"][0] <= blocks_before and len(eng.allocatedSlots()) >= len(allocated)
    assert eng.relocaliserEntries() >= n_kf
    vis = eng.visibleIds().cpu().numpy()
    assert len(vis) == seen[-1]["counters"][2]


def test_stop_integration_mode_neither_fuses_nor_relocalises_a_failed_frame():
    h = _host()
    R = h.TrackingResult
    eng = _engine("FAILUREMODE_STOP_INTEGRATION")
    eng.forceTrackerResult(3, R.TRACKING_FAILED)
    plain = _plain_run()
    got = [_step(eng, f) for f in range(3)]
    eng.trackingInitialised = True       # (the reference sets it after 50 fused frames; before that every frame fuses, :338)
    allocated = set(eng.allocatedSlots().cpu().numpy().tolist())
    stopped = _step(eng, 3)
    assert stopped["result"] == R.TRACKING_POOR and not stopped["fused"]
    assert stopped["frames"] == 3 and stopped["counters"][0] == got[-1]["counters"][0]
    assert set(eng.allocatedSlots().cpu().numpy().tolist()) == allocated
    blocks = _visible_blocks(eng)
    assert len(blocks) > 100 and blocks <= allocated
    assert not eng.hasRelocaliser() and eng.relocalisationCount == 0 and eng.lastRelocalisedTo == -1
    assert np.array_equal(stopped["pose"], plain[3]["pose"])   # POOR keeps the tracker's pose: the same tracking as the plain run's
    after = _step(eng, 4)
    assert after["fused"] and after["frames"] == 4 and after["result"] == R.TRACKING_GOOD
    assert after["counters"][0] <= stopped["counters"][0]


def test_pipeline_does_not_map_from_frames_the_engine_did_not_fuse():
    """SLAMPipeline::processFrame: a frame that did not fuse is not offered as a keyframe and triggers no map update; its camera
    still gets the engine's pose.  160 x 120, 13 frames; with the reference's keyframe thresholds the first frame after frame 0
    opens the keyframe list -- unless it did not fuse."""
    h = _host()
    R = h.TrackingResult
    Wp, Hp, n = 160, 120, 13
    seq = synth.make_sequence(Wp, Hp, n, step_deg=0.5)
    rgb = torch.as_tensor(np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)).cuda()
    dep = torch.as_tensor(seq["depth"].astype(np.int16)).cuda()

    def run(forced):
        eng = h.ITMBasicEngine(Wp, Hp, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
        if forced:
            eng.setFailureMode(h.FailureMode.FAILUREMODE_RELOCALISE)
            eng.forceTrackerResult(FAIL, R.TRACKING_FAILED)
        model = h.SLAMGaussianModel()
        model.loadConfig(dict(capacity=1 << 16))
        pipe = h.SLAMPipeline(eng, model, 11, False)
        rows = []
        for i in range(n):
            c = h.Camera(Wp, Hp, seq["fx"], seq["fy"], seq["cx"], seq["cy"], True, torch.as_tensor(seq["c2w"][i].astype(np.float32)))
            c.id = i
            c.image = rgb[i][..., :3].float() / 255.0
            c.depth = (dep[i].float() / 1000.0).unsqueeze(-1)
            pipe.processFrame(i, c, rgb[i], dep[i])
            st = pipe.stats()
            invM = eng.lastPose()[1].reshape(4, 4).t()   # ORUtils column-major -> the row-major c2w the camera gets
            assert torch.equal(c.c2w_slam.cpu(), invM), i
            rows.append(dict(fused=eng.lastFrameFused(), keyframes=pipe.keyframeCount(), frames=st["frames"], opt_iters=st["opt_iters"],
                             count=eng.relocalisationCount))
        pipe.flush()
        torch.cuda.synchronize()
        # one ground-truth pose and one estimated pose per frame, fused or not: the trajectory evaluation still lines them up
        traj = pipe.evalTrajectory()
        assert np.isfinite(traj.ate_mean_cm) and len(traj.trans_error) == n
        return rows

    plain, lost = run(False), run(True)
    assert all(r["fused"] for r in plain) and plain[1]["keyframes"] == 1 and plain[-1]["opt_iters"] > 0
    assert [r["frames"] for r in lost] == list(range(1, n + 1))            # every frame is counted ...
    for i in range(FAIL, FAIL + 10):                                        # ... but the ten that did not fuse add nothing
        assert not lost[i]["fused"] and lost[i]["keyframes"] == 0 and lost[i]["opt_iters"] == 0, (i, lost[i])
    assert lost[FAIL]["count"] == 10 and lost[FAIL + 10]["count"] == 0
    assert lost[FAIL + 10]["fused"] and lost[FAIL + 10]["keyframes"] == 1   # the first frame that fuses again opens the list


def test_given_poses_follow_the_frame_index_when_a_frame_does_not_fuse():
    """tracking off (poses are given): the pose of frame i is gtC2wPoses[i] whether or not the frames before it fused"""
    h = _host()
    seq = _frames()[0]
    eng = _engine("FAILUREMODE_STOP_INTEGRATION")
    eng.turnOffTracking()
    for i in range(5):
        eng.pushGtPose(torch.as_tensor(seq["c2w"][i].astype(np.float32)))
    eng.trackingInitialised = True
    eng.forceTrackerResult(2, h.TrackingResult.TRACKING_FAILED)
    ref = _engine()
    ref.turnOffTracking()
    for i in range(5):
        ref.pushGtPose(torch.as_tensor(seq["c2w"][i].astype(np.float32)))
    for f in range(5):
        got, want = _step(eng, f), _step(ref, f)
        assert np.array_equal(got["pose"], want["pose"]), f
        assert got["fused"] == (f != 2) and got["frames"] == f + 1 - (1 if f >= 2 else 0), (f, got)
