"""The relocaliser database's text files and the verdict thresholds without a device (host/relocaliser.cpp, host/tsdf_engine.hpp):
the four files the reference's own FernRelocLib saved (tests/golden/reloc_fern.npz, q_file_*) are read and written back byte for
byte; the SE3 parameters of poses.txt against the reference's poses."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reloc_fern.npz")
NAMES = ("config", "ferns", "frames", "poses")


def _host():
    from gps_slam_amd import _build, _build_host, _lib
    _build.build()
    _lib.load_library()
    _build_host.build()
    import gps_slam_amd._host as h
    return h


def _write_fixture_files(d):
    g = np.load(GOLD)
    os.makedirs(d, exist_ok=True)
    for name in NAMES:
        open(os.path.join(d, name + ".txt"), "wb").write(bytes(g["q_file_" + name]))


def test_load_then_save_of_the_references_database_is_byte_identical(tmp_path):
    h = _host()
    g = np.load(GOLD)
    src, dst = str(tmp_path / "in") + "/", str(tmp_path / "out") + "/"
    _write_fixture_files(src)
    os.makedirs(dst)
    n = h.relocDatabaseRewrite(src, dst, int(g["num_ferns"]), int(g["num_decisions"]), float(g["threshold"]))
    assert n == int(g["q_added"].sum()) >= 3
    for name in NAMES:
        got = open(os.path.join(dst, name + ".txt"), "rb").read()
        assert got == bytes(g["q_file_" + name]), name
    assert len(bytes(g["q_file_frames"])) > 16000   # 500 x 16 inverted lists


def test_reader_refuses_a_database_of_another_shape_and_missing_files(tmp_path):
    h = _host()
    src, dst = str(tmp_path / "in") + "/", str(tmp_path / "out") + "/"
    _write_fixture_files(src)
    os.makedirs(dst)
    for ferns, dec in ((499, 4), (500, 3), (500, 5)):
        with pytest.raises(Exception):
            h.relocDatabaseRewrite(src, dst, ferns, dec, 0.2)
    os.remove(src + "poses.txt")
    with pytest.raises(Exception) as e:
        h.relocDatabaseRewrite(src, dst, 500, 4, 0.2)
    assert "poses.txt" in str(e.value)
    _write_fixture_files(src)
    frames = open(src + "frames.txt").read().split("\n")
    open(src + "frames.txt", "w").write("\n".join(frames[:-40]))          # truncated lists
    with pytest.raises(Exception):
        h.relocDatabaseRewrite(src, dst, 500, 4, 0.2)


def test_se3_parameters_are_the_references():
    """poses.txt holds (tx ty tz rx ry rz).  The fixture has the parameters every frame's pose was made from and the M / invM the
    reference's SE3Pose made of them: ours, computed in double and rounded once, agree to float32 rounding of values below 2
    (2 ulp = 2.4e-7 per entry; the reference's float arithmetic carries a few of them), and the logarithm gives the parameters back."""
    h = _host()
    g = np.load(GOLD)
    worst_m = worst_p = 0.0
    for p, pose in zip(g["q_pose_params"], g["q_pose"]):
        got = h.relocPoseFromParams([float(v) for v in p]).numpy().reshape(-1)
        worst_m = max(worst_m, float(np.abs(got - pose).max()))
        back = np.array(h.relocParamsFromPose(torch.as_tensor(pose[:16])), np.float32)
        worst_p = max(worst_p, float(np.abs(back - p).max()))
    print("worst |M - M_ref| %.3g, worst |log(M_ref) - params| %.3g" % (worst_m, worst_p))
    assert worst_m <= 1e-6 and worst_p <= 2e-6
    # identity, a rotation by almost pi (the branch that takes the axis from the symmetric part) and a tiny one
    rng = np.random.default_rng(3)
    for scale in (0.0, 1e-6, 1.0, 3.1, 3.14158):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        p = np.concatenate([rng.normal(size=3), axis * scale]).astype(np.float32)
        M = h.relocPoseFromParams([float(v) for v in p])
        R = M[0].reshape(4, 4).t()[:3, :3].double()
        assert float((R @ R.t() - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
        assert float((M[0].reshape(4, 4).t().double() @ M[1].reshape(4, 4).t().double() - torch.eye(4, dtype=torch.float64)).abs().max()) < 1e-5
        back = np.array(h.relocParamsFromPose(M[0]), np.float32)
        # near pi the logarithm is ill-conditioned in the angle: sin(pi - th) carries the float32 rounding of R's entries
        tol = 2e-3 if scale > 3.14 else 2e-5
        assert np.abs(back - p).max() <= tol, (scale, p, back)


def test_pose_quality_verdict_pairs():
    h = _host()
    R = h.TrackingResult
    t = h.PoseQualityThresholds()
    assert (t.enabled, t.poorScore, t.poorInlierShare, t.failedScore, t.failedInlierShare) == (False, 0.0, 0.0, 0.0, 0.0)
    assert h.poseQualityVerdict(t, 1e9, 0.0) == R.TRACKING_GOOD      # disabled: always GOOD
    t.enabled = True
    t.poorScore, t.poorInlierShare, t.failedScore, t.failedInlierShare = 0.02, 0.5, 0.05, 0.2
    assert h.poseQualityVerdict(t, 0.01, 0.9) == R.TRACKING_GOOD
    assert h.poseQualityVerdict(t, 0.02, 0.5) == R.TRACKING_GOOD     # on a threshold is not beyond it
    assert h.poseQualityVerdict(t, 0.03, 0.9) == R.TRACKING_POOR     # either member of a pair trips it
    assert h.poseQualityVerdict(t, 0.01, 0.4) == R.TRACKING_POOR
    assert h.poseQualityVerdict(t, 0.06, 0.9) == R.TRACKING_FAILED
    assert h.poseQualityVerdict(t, 0.01, 0.1) == R.TRACKING_FAILED
    assert h.poseQualityVerdict(t, 0.06, 0.1) == R.TRACKING_FAILED
