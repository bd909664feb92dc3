"""Geometry and trajectory evaluation in both hosts on the GPU: eval_pcd / evalPointClouds against the reference's own metrics
(tests/golden/geo_eval_ref.npz, written by tests/golden/make_geo_eval_golden.py from scripts/geo_general.py), EvalMesh on a
fused synthetic sequence, evalTrajectory on a short tracked run."""
import os

import numpy as np
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 2.0 ** -21   # per-distance bound of tests/test_geom_nn_gpu.py
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geo_eval_ref.npz")


def _host():
    import gps_slam_amd._host as h
    return h


def _as_dict(r):
    if isinstance(r, dict):
        return {k: r[k] for k in ("accuracy_cm", "completion_cm", "accuracy_ratio", "completion_ratio", "f1", "n_rec", "n_gt")}
    return {k: getattr(r, k) for k in ("accuracy_cm", "completion_cm", "accuracy_ratio", "completion_ratio", "f1", "n_rec", "n_gt")}


def _eval(which, rec, gt, **kw):
    from gps_slam_amd import geom_eval
    if which == "python":
        return _as_dict(geom_eval.eval_pcd(rec, gt, **kw))
    if "dist_thres" in kw:
        kw["dist_thres"] = list(kw["dist_thres"])
    return _as_dict(_host().evalPointClouds(rec, gt, **kw))


@pytest.mark.parametrize("which", ["python", "cpp"])
def test_eval_pcd_matches_the_reference_metrics(which):
    g = np.load(GOLD)
    th = float(g["dist_th"])
    rec, gt = torch.as_tensor(g["rec"]).to(DEV), torch.as_tensor(g["gt"]).to(DEV)
    r = _eval(which, rec, gt, dist_thres=(th,))
    print(which, r, "reference", float(g["accuracy_cm"]), float(g["completion_cm"]), float(g["accuracy_ratio"]), float(g["completion_ratio"]), float(g["f1"]))
    # means of float64 over distances that are each within 2^-21 relative: 2^-20 relative on the mean
    assert abs(r["accuracy_cm"] - float(g["accuracy_cm"])) <= 2.0 ** -20 * float(g["accuracy_cm"])
    assert abs(r["completion_cm"] - float(g["completion_cm"])) <= 2.0 ** -20 * float(g["completion_cm"])
    assert r["n_rec"] == len(g["rec"]) and r["n_gt"] == len(g["gt"])
    # ratios: a count may differ by the number of reference distances within the per-distance bound of the threshold; the inputs
    # must keep that number small (a condition on the fixture, not a measurement)
    for d_ref, ratio, ratio_ref, count_ref in ((g["d_acc"], r["accuracy_ratio"][0], float(g["accuracy_ratio"]), int(g["count_acc"])),
                                               (g["d_comp"], r["completion_ratio"][0], float(g["completion_ratio"]), int(g["count_comp"]))):
        n = len(d_ref)
        n_near = int((np.abs(d_ref - th) <= REL * d_ref).sum())
        assert n_near <= 0.001 * n
        assert abs(round(ratio_ref / 100.0 * n) - count_ref) == 0       # the reference's float32 percentage names that count
        count = round(ratio / 100.0 * n)
        assert abs(count / n * 100.0 - ratio) < 1e-9 and abs(count - count_ref) <= n_near, (count, count_ref, n_near)
    p, q = r["accuracy_ratio"][0], r["completion_ratio"][0]
    assert abs(r["f1"][0] - 2 * p * q / (p + q)) < 1e-12
    assert abs(r["f1"][0] - float(g["f1"])) <= 1e-4 * float(g["f1"])     # the reference's F1 is float32 arithmetic on float32 ratios


def test_eval_pcd_transform_thresholds_and_subsampling_agree_between_hosts():
    g = np.load(GOLD)
    rec, gt = torch.as_tensor(g["rec"]).to(DEV), torch.as_tensor(g["gt"]).to(DEV)
    ang = 0.3
    T = np.eye(4)
    T[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
    T[:3, 3] = [0.2, -0.1, 0.05]
    moved_back = (rec.double() @ torch.as_tensor(np.linalg.inv(T)[:3, :3].T, device=DEV) + torch.as_tensor(np.linalg.inv(T)[:3, 3], device=DEV)).float()
    base = _eval("python", rec, gt, dist_thres=(0.01, 0.03, 0.1))
    a = _eval("python", moved_back, gt, transform=T, dist_thres=(0.01, 0.03, 0.1))
    b = _eval("cpp", moved_back, gt, transform=torch.as_tensor(T), dist_thres=(0.01, 0.03, 0.1))
    assert a == b                                                    # the two hosts: the same operations, the same numbers
    assert abs(a["accuracy_cm"] - base["accuracy_cm"]) < 1e-3 * base["accuracy_cm"]   # T undoes the move (float32 round trip)
    assert a["accuracy_ratio"] == sorted(a["accuracy_ratio"]) and len(a["f1"]) == 3
    # sub-sampling without replacement: min(P, sample_nums) points, the same ones in both hosts for a seed, others for another
    s1 = _eval("python", rec, gt, sample_nums=1000, seed=4)
    s2 = _eval("cpp", rec, gt, sample_nums=1000, seed=4)
    s3 = _eval("python", rec, gt, sample_nums=1000, seed=5)
    assert s1["n_rec"] == 1000 and s1 == s2 and s3["accuracy_cm"] != s1["accuracy_cm"]
    assert _eval("python", rec, gt, sample_nums=10 ** 6)["n_rec"] == len(g["rec"])


def _analytic_scene_points(n_wall, n_sphere, seed):
    """points on the analytic surfaces of tests/synth.py's scene: the room's six walls (as 12 triangles, through sample_surface)
    and the two spheres"""
    from gps_slam_amd import geom_eval
    hx, hy, hz = 3.0, 1.5, 2.5
    tris = []
    for ax, (u, v) in ((0, (1, 2)), (1, (0, 2)), (2, (0, 1))):
        half = [hx, hy, hz]
        for sgn in (-1.0, 1.0):
            c = np.zeros((4, 3))
            c[:, ax] = sgn * half[ax]
            c[:, u] = np.array([-1, 1, 1, -1]) * half[u]
            c[:, v] = np.array([-1, -1, 1, 1]) * half[v]
            tris += [c[[0, 1, 2]], c[[0, 2, 3]]]
    walls = geom_eval.sample_surface(torch.as_tensor(np.stack(tris).astype(np.float32)).to(DEV), n_wall, seed)[0]
    rng = np.random.default_rng(seed)
    pts = [walls]
    for sx, sy, sz, sr in ((0.4, 0.2, 0.3, 0.45), (-0.8, 0.5, -0.4, 0.35)):
        d = rng.normal(size=(n_sphere, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts.append(torch.as_tensor((np.array([sx, sy, sz]) + sr * d).astype(np.float32)).to(DEV))
    return torch.cat(pts), torch.as_tensor(np.stack(tris).astype(np.float32)).to(DEV)


@pytest.fixture(scope="module")
def scene_points():
    return _analytic_scene_points(400000, 20000, 9)


@pytest.mark.parametrize("which", ["python", "cpp"])
def test_eval_mesh_scores_a_fused_synthetic_sequence(which, scene_points):
    from gps_slam_amd import geom_eval
    gt, wall_tris = scene_points
    W, H, frames, voxel, mu = 64, 48, 4, 0.02, 0.08
    seq = synth.make_sequence(W, H, frames, step_deg=1.0)
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    if which == "python":
        from gps_slam_amd.tsdf_engine import TsdfEngine
        eng = TsdfEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], voxel, mu, 0.2, 10.0, device=DEV)
        for f in range(frames):
            eng.ProcessFrame(T(rgba[f]), T(seq["depth"][f].astype(np.int16)), seq["c2w"][f])
        r = _as_dict(eng.EvalMesh(gt, dist_thres=(0.03, 0.05)))
        tri, counts = eng.MeshScene(1 << 20)
        r_tri = _as_dict(eng.EvalMesh(wall_tris, sample_nums=50000, seed=3))
    else:
        h = _host()
        eng = h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], voxel, mu, 0.2, 10.0)
        eng.turnOffTracking()
        for f in range(frames):
            eng.pushGtPose(torch.as_tensor(seq["c2w"][f]))
            eng.ProcessFrame(T(rgba[f]), T(seq["depth"][f].astype(np.int16)))
        r = _as_dict(eng.EvalMesh(gt, dist_thres=[0.03, 0.05]))
        tri, counts = eng.MeshScene(1 << 20)
        r_tri = _as_dict(eng.EvalMesh(wall_tris, sample_nums=50000, seed=3))
    print(which, r)
    n = int(counts[0])
    assert n > 1000 and r["n_rec"] == 3 * n                            # every vertex of every triangle, duplicates included
    vals = [r["accuracy_cm"], r["completion_cm"]] + r["accuracy_ratio"] + r["completion_ratio"] + r["f1"]
    assert all(np.isfinite(v) for v in vals)
    assert r["accuracy_cm"] < 2 * voxel * 100.0, r                     # the surface is where the scene's surfaces are
    assert r["accuracy_ratio"][0] <= r["accuracy_ratio"][1] and r["completion_ratio"][0] > 0
    # ... and it is eval_pcd applied by hand to MeshScene()'s vertices
    by_hand = _as_dict(geom_eval.eval_pcd(tri[:n, 0:3].reshape(-1, 3).contiguous(), gt, dist_thres=(0.03, 0.05)))
    assert by_hand == r
    # ground truth given as triangles: sample_nums points sampled from them with the seed
    sampled = geom_eval.sample_surface(wall_tris, 50000, 3)[0]
    assert r_tri == _as_dict(geom_eval.eval_pcd(tri[:n, 0:3].reshape(-1, 3).contiguous(), sampled, sample_nums=50000, seed=3))
    assert r_tri["n_gt"] == 50000 and r_tri["n_rec"] == min(3 * n, 50000)


@pytest.mark.parametrize("which", ["python", "cpp"])
def test_eval_trajectory_is_ate_of_the_stored_poses(which):
    from gps_slam_amd import geom_eval
    W, H, n = 160, 120, 6
    seq = synth.make_sequence(W, H, n, step_deg=0.4)
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    est = []
    if which == "python":
        from gps_slam_amd.gs_model import Camera, SLAMGaussianModel
        from gps_slam_amd.slam_pipeline import SLAMPipeline
        from gps_slam_amd.tsdf_engine import TsdfEngine
        eng = TsdfEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], voxel_size=0.01, mu=0.04, device=DEV)
        pipe = SLAMPipeline(eng, SLAMGaussianModel(dict(capacity=1 << 12), device=DEV), work_mode="recon", use_gt_pose=False)
        for i in range(n):
            if i == 2:
                with pytest.raises(ValueError):
                    pipe.evalTrajectory()                                  # two frames: an error, not a number
            c = Camera(i, W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], seq["c2w"][i], device=DEV)
            pipe.process_frame(i, c, T(rgba[i]), T(seq["depth"][i].astype(np.int16)))
            est.append(np.asarray(eng.camPoses[-1][1], np.float64).reshape(4, 4).T)
        r = pipe.evalTrajectory()
        got = (r["ate_mean_cm"], r["ate_rmse_cm"])
    else:
        h = _host()
        eng = h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
        model = h.SLAMGaussianModel()
        model.loadConfig(dict(capacity=1 << 12))
        pipe = h.SLAMPipeline(eng, model, 1, False)
        pipe.work_mode = "recon"
        for i in range(n):
            if i == 2:
                with pytest.raises(RuntimeError):
                    pipe.evalTrajectory()
            c = h.Camera(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], True, torch.as_tensor(seq["c2w"][i].astype(np.float32)))
            c.id = i
            pipe.processFrame(i, c, T(rgba[i]), T(seq["depth"][i].astype(np.int16)))
            est.append(eng.lastPose()[1].double().numpy().reshape(4, 4).T)
        r = pipe.evalTrajectory()
        got = (r.ate_mean_cm, r.ate_rmse_cm)
    want = geom_eval.ate(np.stack(est), seq["c2w"][:n].astype(np.float64))
    print(which, got, want["ate_mean_cm"])
    assert abs(got[0] - want["ate_mean_cm"]) <= 1e-9 * max(want["ate_mean_cm"], 1e-6)
    assert abs(got[1] - want["ate_rmse_cm"]) <= 1e-9 * max(want["ate_rmse_cm"], 1e-6)
    assert 0 <= got[0] < 1.0                                               # the tracker follows the orbit to millimetres
    assert np.abs(est[-1] - est[0]).max() > 1e-3                           # ... and the camera actually moved
