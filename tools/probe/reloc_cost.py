"""What the device relocaliser costs per frame (csrc/reloc_fern.hip), two ways:

  alone     gps_reloc_process_frame back to back on one stream (device events around 200 frames) at 640 x 480, 500 ferns of 4
            decisions, with 0 / 64 / 1,024 / 4,096 / 16,384 / 65,536 stored keyframes (imported random codes; harvesting off, so the
            count stays): the search is num_ferns bytes per keyframe, the other three launches do not depend on the count
  in-loop   per-launch times of the four kernels inside the tracked schedule (gps_launch_timing_*), and frames/s of the C++ engine's tracked ProcessFrame on a synthetic 640 x 480 sequence with failure mode IGNORE (the
            default: no relocaliser exists) against RELOCALISE (the relocaliser sees every frame, nothing is forced, every frame
            fuses), in alternating runs of the same process -- the spread of the IGNORE runs is the yardstick

One process; ends itself after --limit seconds.   usage (GPU box): python tools/probe/reloc_cost.py"""
import argparse
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from gps_slam_amd import relocaliser as RL
from tests import synth

DEV = "cuda:0"


def alone(counts, W, H, reps):
    depth = (torch.rand((H, W), device=DEV) * 4.0 + 0.3).contiguous()
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    for n in counts:
        r = RL.FernRelocaliser(W, H, depth_range=(0.2, 5.0), capacity=max(n, 1))
        if n:
            rng = np.random.default_rng(n)
            r.import_database(rng.integers(0, 16, (n, r.num_ferns), dtype=np.uint8), np.tile(np.concatenate([eye, eye]), (n, 1)),
                              np.zeros(n, np.int32))
        for _ in range(20):
            r.process_frame(depth, eye, eye, k=1, harvest=False)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            r.process_frame(depth, eye, eye, k=1, harvest=False)
        ev[1].record()
        torch.cuda.synchronize()
        res = r.read_result()
        print("alone  %4d x %d, %6d keyframes: %7.1f us per frame (4 launches, back to back; nearest id %d at %.3f)"
              % (W, H, n, ev[0].elapsed_time(ev[1]) / reps * 1e3, res["ids"][0], float(res["distances"][0])), flush=True)
        r.close()


def in_loop(W, H, n_frames, rounds):
    import gps_slam_amd._host as h
    seq = synth.make_sequence(W, H, n_frames, step_deg=0.2)
    rgba = torch.as_tensor(np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)).to(DEV)
    depth = torch.as_tensor(seq["depth"].astype(np.int16)).to(DEV)

    def run(mode):
        eng = h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
        eng.setFailureMode(mode)
        eng.ProcessFrame(rgba[0], depth[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(1, n_frames):
            eng.ProcessFrame(rgba[f], depth[f])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return (n_frames - 1) / dt, eng.relocaliserEntries()

    run(h.FailureMode.FAILUREMODE_IGNORE)   # warm-up: code objects, allocator
    rates = {"ignore": [], "relocalise": []}
    for _ in range(rounds):
        rates["ignore"].append(run(h.FailureMode.FAILUREMODE_IGNORE)[0])
        fps, kf = run(h.FailureMode.FAILUREMODE_RELOCALISE)
        rates["relocalise"].append(fps)
    for name, v in rates.items():
        print("in-loop %4d x %d, %d tracked frames, %-10s: %s frames/s  (median %.1f, spread %.1f)"
              % (W, H, n_frames - 1, name, " ".join("%.1f" % x for x in v), float(np.median(v)), max(v) - min(v)), flush=True)
    print("in-loop keyframes harvested by the RELOCALISE runs: %d" % kf, flush=True)
    # the four launches inside that schedule, each by its own stamps (gps_launch_timing_*: first wave start .. last wave end)
    import ctypes as C
    from gps_slam_amd._lib import lib
    assert lib.gps_launch_timing_start(1 << 20) == 0
    run(h.FailureMode.FAILUREMODE_RELOCALISE)
    assert lib.gps_launch_timing_stop() == 0
    for kind, name in ((9, "pyramid"), (10, "blur + code"), (11, "search"), (12, "finish"), (6, "integrate"), (7, "raycast")):
        tot, n, mx = C.c_double(), C.c_int64(), C.c_double()
        assert lib.gps_launch_timing_read(kind, C.byref(tot), C.byref(n), None, None, C.byref(mx), None) == 0
        print("in-loop launch %-12s: %4d launches, %7.2f us each (max %.2f)" % (name, n.value, tot.value / max(n.value, 1), mx.value), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", type=int, nargs="+", default=[0, 64, 1024, 4096, 16384, 65536])
    ap.add_argument("--size", type=int, nargs=2, default=[640, 480])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300)
    a = ap.parse_args()
    signal.alarm(a.limit)
    alone(a.counts, a.size[0], a.size[1], a.reps)
    in_loop(a.size[0], a.size[1], a.frames, a.rounds)


if __name__ == "__main__":
    main()
