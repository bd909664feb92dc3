"""What the bilateral depth filter (use_bilateral_filter: five passes of the 5 x 5 depth-adaptive filter behind the conversion) costs
and buys on a tracked 640 x 480 orbit of tests/synth whose depth carries seeded noise drawn from the filter's own model
(sigma_z = 0.0012 + 0.0019 (z - 0.4)^2 + 0.0001 / sqrt(z) * 0.25 metres, rounded to millimetres):

  * device time of the five passes per frame, by the library's launch stamps (gps_launch_timing_*, one window per frame), median
    over --stamped frames;
  * frames per second of ProcessFrameTracked alone with the option off and on (the settings alternate, --repeats times each, in
    one process; every run starts from a fresh engine and is timed after WARMUP frames, host clock around a device synchronise;
    the camera walks the orbit forth and back --passes times);
  * the trajectory error (geom_eval.ate) against the given poses and the mesh accuracy / completion (EvalMesh against points on
    the scene's analytic surfaces) of one walk forth, both ways, and of the same walk on the noise-free depth.

--plain leaves the option's argument away altogether and reports the off numbers only: the same script then runs on a tree
from before the option existed.

  python tools/probe/bilateral.py [--frames 60] [--passes 6] [--repeats 3] [--stamped 20] [--plain] [--fps-only] [--out probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from gps_slam_amd import geom_eval
from gps_slam_amd._lib import lib
from gps_slam_amd.tsdf_engine import TsdfEngine
from tests import synth

W, H, WARMUP = 640, 480, 20
FILTER_DEPTH = 15   # GPS_TIMED_FILTER_DEPTH


def noisy(depth_mm, seed):
    z = depth_mm.astype(np.float64) / 1000.0
    sigma = 0.0012 + 0.0019 * (z - 0.4) ** 2 + 0.0001 / np.sqrt(np.maximum(z, 1e-3)) * 0.25
    d = np.rint(depth_mm + np.random.default_rng(seed).normal(size=z.shape) * sigma * 1000.0)
    return np.where(depth_mm > 0, np.clip(d, 1, 32767), 0).astype(np.int16)


def engine(seq, option):
    kw = {} if option is None else dict(use_bilateral_filter=option)
    eng = TsdfEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.005, 0.02, device="cuda:0", **kw)
    eng.turnOnTracking()
    return eng


def timed_run(seq, frames, order, option):
    eng = engine(seq, option)
    for i in order[:WARMUP]:
        eng.ProcessFrameTracked(*frames[i])
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in order[WARMUP:]:
        eng.ProcessFrameTracked(*frames[i])
    torch.cuda.synchronize()
    return (len(order) - WARMUP) / (time.perf_counter() - t)


def scene_points(n_wall, n_sphere, seed):
    """points on the analytic surfaces of tests/synth.py's scene: the room's six walls and the two spheres"""
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
    pts = [geom_eval.sample_surface(torch.as_tensor(np.stack(tris).astype(np.float32)).cuda(), n_wall, seed)[0]]
    rng = np.random.default_rng(seed)
    for sx, sy, sz, sr in ((0.4, 0.2, 0.3, 0.45), (-0.8, 0.5, -0.4, 0.35)):
        d = rng.normal(size=(n_sphere, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts.append(torch.as_tensor((np.array([sx, sy, sz]) + sr * d).astype(np.float32)).cuda())
    return torch.cat(pts)


def quality_run(seq, frames, n, option, gt_points):
    """one walk forth -> trajectory error and mesh scores (the tracker starts at the identity: its map lives in the first
    camera's frame, c2w[0] takes it to the scene's)"""
    eng = engine(seq, option)
    for i in range(n):
        eng.ProcessFrameTracked(*frames[i])
    est = np.stack([np.asarray(invM, np.float64).reshape(4, 4).T for _, invM in eng.camPoses])
    gt = np.stack([np.linalg.inv(seq["c2w"][0].astype(np.float64)) @ seq["c2w"][i].astype(np.float64) for i in range(n)])
    ate = geom_eval.ate(est, gt)
    r = eng.EvalMesh(gt_points, transform=seq["c2w"][0].astype(np.float64), dist_thres=(0.01, 0.03))
    r = r if isinstance(r, dict) else {k: getattr(r, k) for k in ("accuracy_cm", "completion_cm", "accuracy_ratio", "completion_ratio", "f1")}
    return dict(ate_mean_cm=float(ate["ate_mean_cm"]), ate_rmse_cm=float(ate["ate_rmse_cm"]), accuracy_cm=float(r["accuracy_cm"]),
                completion_cm=float(r["completion_cm"]), accuracy_ratio_1cm=float(r["accuracy_ratio"][0]), f1_1cm=float(r["f1"][0]))


def stamped_filter_us(seq, frames, n):
    """device microseconds of the five passes of each of n frames"""
    eng = engine(seq, True)
    for i in range(5):
        eng.ProcessFrameTracked(*frames[i])
    torch.cuda.synchronize()
    us = []
    for i in range(5, 5 + n):
        assert lib.gps_launch_timing_start(1 << 16) == 0
        try:
            eng.ProcessFrameTracked(*frames[i % len(frames)])
            torch.cuda.synchronize()
        finally:
            rc = lib.gps_launch_timing_stop()
        assert rc == 0
        tot, totf, mx = C.c_double(), C.c_double(), C.c_double()
        cnt, nf, dropped = C.c_int64(), C.c_int64(), C.c_int64()
        assert lib.gps_launch_timing_read(FILTER_DEPTH, C.byref(tot), C.byref(cnt), C.byref(totf), C.byref(nf), C.byref(mx), C.byref(dropped)) == 0
        assert cnt.value == 5 and dropped.value == 0, (cnt.value, dropped.value)
        us.append(tot.value)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--step-deg", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stamped", type=int, default=20)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--fps-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    seq = synth.make_sequence(W, H, a.frames, step_deg=a.step_deg)
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda().contiguous()
    clean = [(up(rgba[i]), up(seq["depth"][i].astype(np.int16))) for i in range(a.frames)]
    frames = [(clean[i][0], up(noisy(seq["depth"][i], 1000 + i))) for i in range(a.frames)]
    forth = list(range(a.frames))
    order = ((forth + forth[-2:0:-1]) * ((a.passes + 1) // 2))[:a.passes * a.frames]
    settings = [None] if a.plain else [False, True]
    for s in settings:
        timed_run(seq, frames, order[:WARMUP + 5], s)   # code objects, allocator
    fps = {str(s): [] for s in settings}
    for _ in range(a.repeats):
        for s in settings:
            fps[str(s)].append(timed_run(seq, frames, order, s))
    out = dict(width=W, height=H, frames=a.frames, passes=a.passes, timed_frames=len(order) - WARMUP, warmup=WARMUP, step_deg=a.step_deg,
               fps={k: v for k, v in fps.items()}, fps_median={k: float(np.median(v)) for k, v in fps.items()})
    if not a.plain and not a.fps_only:
        us = stamped_filter_us(seq, frames, a.stamped)
        out["filter_us_per_frame"] = dict(median=float(np.median(us)), min=float(min(us)), max=float(max(us)), frames=len(us))
        gt_points = scene_points(400000, 20000, 9)
        out["quality"] = {"noisy_off": quality_run(seq, frames, a.frames, False, gt_points),
                          "noisy_on": quality_run(seq, frames, a.frames, True, gt_points),
                          "clean_off": quality_run(seq, clean, a.frames, False, gt_points),
                          "clean_on": quality_run(seq, clean, a.frames, True, gt_points)}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
