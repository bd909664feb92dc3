"""What the refinement pass (SLAMPipeline::gesTrainCams) buys on the detail workload -- the one behind bench.py's whole_run_gain_db
(bench.detail_run: the room scaled to 0.4 with the `fine` texture, 640 x 480, SLAMTrainCams from an empty model, sequential
schedule) -- with both pose sources.  Per repeat and pose source ONE whole run; from its final model (restored before each) the
pass with --iterations (1,000 and 5,000) over `keyframes` (keyframe_cam_list + the live window) and over `all` cameras but the
held-out ones.  The
comparison is the same run without the pass.  Reported: held-out PSNR (the frames of the last three keyframe periods that are
never optimise cameras, rendered from their estimated poses) before and after, the gain over the TSDF colour, refinement iterations
per second (host clock around a device synchronise, base-layer raycasts included and alone) next to the rate of the iteration body
of localOptimize in the same process (the last update's view set, round robin, run-ahead forward on), and the cache size.
Medians over --repeats; the pose sources and the configurations alternate inside every repeat.

  python tools/probe/refine.py [--frames 300] [--iterations 1000,5000] [--repeats 3] [--out bench_logs/refine_probe.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

import bench

DEV = "cuda:0"
NAMES = ("getMeans", "getScales", "getQuats", "getFeaturesDc", "getFeaturesRest", "getOpacities")


def psnr(a, b):
    return float(-10.0 * torch.log10(((a.clamp(0, 1) - b) ** 2).mean()))


def held_out(sc, model, cams, seq, frames):
    """-> (render dB, TSDF colour dB), means over `frames`, each rendered from its estimated pose (cams[j].c2w_slam)"""
    r, t = [], []
    with torch.no_grad():
        for j in frames:
            cam = cams[j]
            rc = sc.pipe.runRaycastByCam(cam, False)
            r.append(psnr(model.forward(cam, rc["depth_map"], rc["color_map"])["rgb"], cam.image))
            t.append(psnr(rc["color_map"], cam.image))
    return float(np.mean(r)), float(np.mean(t))


def body_rate(sc, model, iters=200):
    """iterations per second of localOptimize's iteration body on the last update's views (fresh optimiser, run-ahead forward on)"""
    views = list(zip(sc.pipe.optCams(), sc.pipe.optRaycasts()))
    model.initOptimizers(-1, sc.pipe.scene_scale)
    step = lambda k: model.trainStep(views[k % len(views)][0], views[k % len(views)][1]["depth_map"], views[k % len(views)][1]["color_map"],
                                     views[k % len(views)][1]["depth_map_clamped"], views[(k + 1) % len(views)][0])
    for k in range(20):
        step(k)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for k in range(20, 20 + iters):
        step(k)
    torch.cuda.synchronize()
    return iters / (time.perf_counter() - t), len(views)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--iterations", default="1000,5000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join("bench_logs", "refine_probe.json"))
    args = ap.parse_args()
    counts = [int(x) for x in args.iterations.split(",")]
    n, seed = args.frames, args.seed
    torch.cuda.set_device(0)
    seq = bench.synthetic_sequence_device(640, 480, n, seed, DEV, texture="fine", world_scale=0.4)
    bench.prime(DEV)
    last_kf = (n - 1) // bench.PERIOD * bench.PERIOD
    held = [k for p0 in range(max(bench.PERIOD, last_kf - 2 * bench.PERIOD), last_kf + 1, bench.PERIOD) for k in (p0 + 3, p0 + 7) if k < n]
    rows = []
    for rep in range(args.repeats):
        for gt_pose in ((False, True) if rep % 2 == 0 else (True, False)):
            sc = bench.Scene(seq, None, seed, gt_pose, overlap=False, n_frames=n, keyframe_theta=1.0, keyframe_trans=0.02)
            torch.cuda.synchronize()
            cams = sc.pipe.SLAMTrainCamsModel(sc.model, sc.cams)     # (copies: with the estimated poses in c2w_slam)
            for j, cam in enumerate(cams):
                cam.image = torch.as_tensor(seq["rgb"][j]).to(DEV).float() / 255.0
                cam.toGPU()
            torch.cuda.synchronize()
            p = sc.model.getGaussianParms()
            final = [getattr(p, name)().clone() for name in NAMES]
            before, tsdf = held_out(sc, sc.model, cams, seq, held)
            rate, n_views = body_rate(sc, sc.model)
            base = dict(repeat=rep, use_gt_pose=gt_pose, gaussians=int(final[0].shape[0]), keyframes=int(sc.pipe.keyframeCount()),
                        held_out_frames=len(held), tsdf_colour_psnr_db=tsdf, psnr_before_db=before, local_optimize_body_its_per_s=rate,
                        local_optimize_views=n_views)
            configs = [(which, c) for which in ("keyframes", "all") for c in counts]
            for which, count in (configs if rep % 2 == 0 else configs[::-1]):
                model = sc.H_.SLAMGaussianModel()
                model.loadConfig(dict(capacity=1 << 19, isect_capacity=8 << 20))
                model.getGaussianParms().add([t.clone() for t in final])
                model.reserveWorkspace(640, 480)
                sc.pipe.setModel(model)
                sc.pipe.curr_iter = 0
                # (`all`: every camera but the held-out frames, so that those stay held out; no keyframe is one of them)
                sel = sc.pipe.refineKeyframeCams() if which == "keyframes" else [c for j, c in enumerate(cams) if j not in held]
                assert not any(c.id in held for c in sel)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sc.pipe.gesTrainCams(sel, 0, seed)                  # the base layers alone (no iteration)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                done = sc.pipe.gesTrainCams(sel, count, seed)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                after, _ = held_out(sc, model, cams, seq, held)
                row = dict(base, cams=which, n_cams=len(sel), iterations=done, psnr_after_db=after, delta_db=after - before,
                           gain_over_tsdf_before_db=before - tsdf, gain_over_tsdf_after_db=after - tsdf,
                           base_layers_s=t1 - t0, refine_its_per_s=done / (t2 - t1), cache_mb=sc.pipe.refineCacheBytes(sel) / 2.0 ** 20,
                           final_loss=sc.pipe.refineLog()[-1][1])
                rows.append(row)
                print(json.dumps(row), flush=True)
                del model
            sc.pipe.setModel(sc.model)
            sc.close()
            del sc
            torch.cuda.empty_cache()
    med = lambda xs: float(np.median(xs))
    table = []
    for gt_pose in (False, True):
        for which in ("keyframes", "all"):
            for count in counts:
                sel = [r for r in rows if r["use_gt_pose"] == gt_pose and r["cams"] == which and r["iterations"] == count]
                if sel:
                    table.append(dict(use_gt_pose=gt_pose, cams=which, n_cams=sel[0]["n_cams"], iterations=count, runs=len(sel),
                                      **{k: med([r[k] for r in sel]) for k in ("tsdf_colour_psnr_db", "psnr_before_db", "psnr_after_db", "delta_db",
                                                                               "gain_over_tsdf_before_db", "gain_over_tsdf_after_db", "refine_its_per_s",
                                                                               "local_optimize_body_its_per_s", "base_layers_s", "cache_mb", "gaussians")}))
    print("| poses | cameras | iterations | held-out PSNR before -> after (dB) | gain over TSDF colour before -> after (dB) | refine it/s | localOptimize body it/s | base layers s | cache MiB |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in table:
        print("| %s | %s (%d) | %d | %.2f -> %.2f (%+.2f) | %+.2f -> %+.2f | %.0f | %.0f | %.3f | %.0f |" % (
            "given" if r["use_gt_pose"] else "tracked", r["cams"], r["n_cams"], r["iterations"], r["psnr_before_db"], r["psnr_after_db"], r["delta_db"],
            r["gain_over_tsdf_before_db"], r["gain_over_tsdf_after_db"], r["refine_its_per_s"], r["local_optimize_body_its_per_s"], r["base_layers_s"],
            r["cache_mb"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(dict(frames=n, held_out=held, rows=rows, medians=table), open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
