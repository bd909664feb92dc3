"""One optimise iteration with loss terms (ssim_weight 0.2, depth_weight 0.1) in the C++ host at 640x480 (~200 k Gaussians, the
bench scene): the autograd route (forward -> computeLoss -> backward -> optimizersStep -> optimizersZeroGrad, what SLAMPipeline
runs with fused_loss_terms off) against trainStep with the weights (fused_loss_terms on), and the plain L1 trainStep for scale.
Timed alternately in one process: HIP events around blocks of 50 iterations, 5 windows per route; median and spread (max - min).
usage: python tools/probe/loss_terms_ab.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench
from gps_slam_amd.dist_util import cap_host_threads

W, H, NG, BLOCK, WINDOWS = 640, 480, 200000, 50, 5
WEIGHTS = dict(ssim_weight=0.2, depth_weight=0.1)
cap_host_threads()
seq = bench.synthetic_sequence(W, H, 31, 1234)
seeds = bench.seed_gaussians(seq, NG, 1234, "cuda:0")
scene = bench.Scene(seq, seeds, 1234, True, False, 31, 1.0, 0.02)
scene.run(0, 31)
import gps_slam_amd._host as host

cp = scene.model.getGaussianParms()
tensors = [cp.getMeans(), cp.getScales(), cp.getQuats(), cp.getFeaturesDc(), cp.getFeaturesRest(), cp.getOpacities()]
cam, rc = scene.pipe.optCams()[-1], scene.pipe.optRaycasts()[-1]
if cam.depth is None or cam.depth.numel() == 0:   # the depth term needs a sensor depth: the raycast's stands in
    cam.depth = rc["depth_map"].clone()
models = {}
for name in ("autograd", "fused", "l1"):
    m = host.SLAMGaussianModel()
    m.loadConfig(dict(capacity=1 << 19, isect_capacity=8 << 20))
    m.getGaussianParms().add([t.clone() for t in tensors])
    m.initOptimizers(-1, 1.0)
    models[name] = m
args = (cam, rc["depth_map"], rc["color_map"], rc["depth_map_clamped"])


def step(name):
    m = models[name]
    if name == "autograd":
        res = m.forward(cam, rc["depth_map"], rc["color_map"])
        m.computeLoss(res, cam, WEIGHTS)["total"].backward()
        m.optimizersStep()
        m.optimizersZeroGrad()
    elif name == "fused":
        m.trainStep(*args, None, WEIGHTS)
    else:
        m.trainStep(*args)


for name in models:   # warm-up
    for _ in range(20):
        step(name)
torch.cuda.synchronize()
times = {k: [] for k in models}
order = list(models)
for r in range(WINDOWS):
    for name in (order if r % 2 == 0 else order[::-1]):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BLOCK):
            step(name)
        b.record()
        torch.cuda.synchronize()
        times[name].append(1e3 * a.elapsed_time(b) / BLOCK)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print("N %d, %dx%d, weights %s" % (models["fused"].getGaussianNum(), W, H, WEIGHTS))
print("loss terms of the last fused step {total, l1, 1 - ssim, depth}: %s" % [round(float(x), 5) for x in models["fused"].lossTerms()])
for k in order:
    print("%-8s us/iter: median %.1f  spread %.1f  windows %s" % (k, med[k], max(times[k]) - min(times[k]), " ".join("%.1f" % t for t in times[k])))
print("fused - autograd: %+.1f us/iter;  added launches (fused - l1): %+.1f us/iter" % (med["fused"] - med["autograd"], med["fused"] - med["l1"]))
