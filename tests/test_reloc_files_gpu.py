"""The relocaliser's text files, verdict thresholds and launch timing on the device: FernRelocLib::Relocaliser<float> of the C++ host
(host/relocaliser.{hpp,cpp}) loads the database the reference saved (tests/golden/reloc_fern.npz, q_file_*), answers as the
reference does, and saves what the reference saved; the engine's SaveToFile / LoadFromFile carry Relocaliser/."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import reloc_cases as cases, synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reloc_fern.npz")
NAMES = ("config", "ferns", "frames", "poses")
W, H = 320, 240


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


def _files(d, empty=False):
    """the reference's saved database under d/ -- or, empty: its fern table with no entries"""
    g = np.load(GOLD)
    os.makedirs(d, exist_ok=True)
    for name in NAMES:
        data = bytes(g["q_file_" + name])
        if empty and name == "frames":
            data = ("%d %d 0\n" % (int(g["num_ferns"]), 1 << int(g["num_decisions"])) + "0 \n" * (int(g["num_ferns"]) << int(g["num_decisions"]))).encode()
        if empty and name == "poses":
            data = b"0\n"
        open(os.path.join(d, name + ".txt"), "wb").write(data)
    return d + "/"


def _reloc(h, g):
    return h.Relocaliser(W, H, float(g["depth_range"][0]), float(g["depth_range"][1]), float(g["threshold"]), int(g["num_ferns"]),
                         int(g["num_decisions"]), 64, 3)


def test_database_saved_by_the_reference_loads_answers_and_saves_back(tmp_path):
    h = _host()
    g = np.load(GOLD)
    r = _reloc(h, g)
    r.LoadFromDirectory(_files(str(tmp_path / "ref")))
    kf = [i for i in range(len(g["q_specs"])) if g["q_added"][i]]
    assert r.numEntries() == len(kf) >= 3
    for idx, i in enumerate(kf):   # poses.txt carries six digits of the parameters: the pose comes back to ~1e-6 of a value below 2
        pose, scene = r.RetrievePose(idx)
        assert scene == 0 and np.abs(pose.numpy().reshape(-1) - g["q_pose"][i]).max() < 2e-5, idx
    # the loaded fern table and codes are exact: the tie probe (never harvested) gets the reference's answer, tie rule included
    tie = int(g["q_tie_frame"])
    depth = torch.as_tensor(cases.frame_depth(W, H, tuple(g["q_specs"][tie]), int(g["hole_seed"]))).cuda()
    r.ProcessFrame(depth, torch.as_tensor(g["q_pose"][tie]).reshape(2, 16), 0, 3, False)
    res = r.ReadResult()
    assert res["ids"][:3] == [int(v) for v in g["q_nn3"][tie]] and res["added_id"] == -1
    assert np.array_equal(np.array(res["distances"][:3], np.float32).view(np.uint32), g["q_dist3"][tie].view(np.uint32))
    out = str(tmp_path / "out") + "/"
    os.makedirs(out)
    r.SaveToDirectory(out)
    for name in NAMES:
        assert open(out + name + ".txt", "rb").read() == bytes(g["q_file_" + name]), name


def test_database_harvested_here_saves_as_the_reference_saved_its_own(tmp_path):
    """the reference's fern table, no entries; the 22 frames through ProcessFrame; the saved files against the reference's -- the
    three that hold integers and the table byte for byte, poses.txt (the logarithm of the stored M, six digits) number by number"""
    h = _host()
    g = np.load(GOLD)
    r = _reloc(h, g)
    r.LoadFromDirectory(_files(str(tmp_path / "empty"), empty=True))
    assert r.numEntries() == 0
    depths = torch.as_tensor(cases.sequence_depths(W, H, [tuple(s) for s in g["q_specs"]], int(g["hole_seed"]))).cuda()
    for i in range(len(g["q_specs"])):
        r.ProcessFrame(depths[i], torch.as_tensor(g["q_pose"][i]).reshape(2, 16), 0, 1, bool(g["q_harvest"][i]))
    out = str(tmp_path / "out") + "/"
    os.makedirs(out)
    r.SaveToDirectory(out)
    for name in ("config", "ferns", "frames"):
        assert open(out + name + ".txt", "rb").read() == bytes(g["q_file_" + name]), name
    got = open(out + "poses.txt").read().split()
    want = bytes(g["q_file_poses"]).decode().split()
    assert len(got) == len(want) and got[0] == want[0]
    worst = max(abs(float(a) - float(b)) for a, b in zip(got, want))
    print("poses.txt: worst parameter difference %.3g, identical text: %s" % (worst, got == want))
    assert worst <= 2e-6   # the reference prints the parameters the poses were made from; ours are the float32 M's logarithm


def _engine_frames(n):
    seq = synth.make_sequence(W, H, n, step_deg=0.5)
    rgba = torch.as_tensor(np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)).cuda()
    return seq, rgba, torch.as_tensor(seq["depth"].astype(np.int16)).cuda()


def test_engine_state_files_carry_the_relocaliser(tmp_path):
    h = _host()
    seq, rgba, depth = _engine_frames(3)
    mk = lambda: h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
    a = mk()
    a.setFailureMode(h.FailureMode.FAILUREMODE_RELOCALISE)
    for f in range(3):
        a.ProcessFrame(rgba[f], depth[f])
    n = a.relocaliserEntries()
    assert n >= 1
    d = str(tmp_path / "state")
    a.SaveToFile(d)
    for name in NAMES:
        assert os.path.getsize(os.path.join(d, "Relocaliser", name + ".txt")) > 0, name
    b = mk()
    b.setFailureMode(h.FailureMode.FAILUREMODE_RELOCALISE)
    b.LoadFromFile(d)
    assert b.hasRelocaliser() and b.relocaliserEntries() == n
    assert np.abs(b.relocaliserPose(0).numpy() - a.relocaliserPose(0).numpy()).max() < 2e-5
    c = mk()                       # the default mode leaves the directory alone
    c.LoadFromFile(d)
    assert not c.hasRelocaliser()
    e = mk()                       # ... and writes no database: an engine without a relocaliser has none
    e.ProcessFrame(rgba[0], depth[0])
    d2 = str(tmp_path / "plain")
    e.SaveToFile(d2)
    assert not os.path.exists(os.path.join(d2, "Relocaliser", "frames.txt"))


def test_thresholds_on_the_inlier_share_and_the_score_give_the_verdict():
    h = _host()
    R = h.TrackingResult
    seq, rgba, depth = _engine_frames(4)
    eng = h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
    eng.setFailureMode(h.FailureMode.FAILUREMODE_STOP_INTEGRATION)
    eng.ProcessFrame(rgba[0], depth[0])
    assert eng.inlierShare() == 0.0                       # nothing tracked yet
    eng.ProcessFrame(rgba[1], depth[1])
    share, score = eng.inlierShare(), float(eng.trackDiag()[10])
    assert 0.5 < share <= 1.0 and 0.0 < score < 0.1, (share, score)   # a clean synthetic frame: most valid pixels are inliers
    t = h.PoseQualityThresholds()
    t.enabled = True
    t.poorScore, t.failedScore, t.poorInlierShare, t.failedInlierShare = 1e9, 1e9, 0.0, 0.0     # nothing can trip
    eng.setPoseQualityThresholds(t)
    eng.ProcessFrame(rgba[2], depth[2])
    assert eng.trackerResult() == R.TRACKING_GOOD and eng.lastFrameFused()
    t.poorInlierShare = 1.5                                # every share is below it: POOR by the inlier share alone
    eng.setPoseQualityThresholds(t)
    eng.trackingInitialised = True
    eng.ProcessFrame(rgba[3], depth[3])
    assert eng.trackerResult() == R.TRACKING_POOR and not eng.lastFrameFused()


def test_the_four_launches_report_to_launch_timing():
    from gps_slam_amd import relocaliser as RL
    from gps_slam_amd._lib import lib
    r = RL.FernRelocaliser(W, H, capacity=8)
    depth = torch.full((H, W), 1.5, device="cuda")
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    r.process_frame(depth, eye, eye)
    torch.cuda.synchronize()
    assert lib.gps_launch_timing_start(4096) == 0
    for _ in range(3):
        r.process_frame(depth, eye, eye)
    torch.cuda.synchronize()
    assert lib.gps_launch_timing_stop() == 0
    for kind in (9, 10, 11, 12):   # GPS_TIMED_RELOC_PYRAMID .. GPS_TIMED_RELOC_FINISH
        tot, n, mx = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        assert lib.gps_launch_timing_read(kind, ctypes.byref(tot), ctypes.byref(n), None, None, ctypes.byref(mx), None) == 0
        assert n.value == 3 and 0.0 < tot.value < 3000.0, (kind, n.value, tot.value)
    r.close()
