"""One optimise iteration with loss terms (ssim_weight 0.2, depth_weight 0.1) for a camera WITH an exposure row in the C++ host at
640x480 (~200 k Gaussians, the bench scene): the autograd route (forward -> computeLoss -> backward -> optimizersStep ->
optimizersZeroGrad, what SLAMPipeline runs for a use_exposure model with fused_loss_terms off) against trainStep with the weights
(gps_splat_step::exposure_terms, fused_loss_terms on), and trainStep with the weights on a model without exposure as the floor.
Timed alternately in one process: HIP events around blocks of 50 iterations, 5 windows per route; median and spread (max - min).
usage: python tools/probe/loss_terms_exposure_ab.py"""
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
rows = max(int(cam.id), 0) + 1
gen = torch.Generator().manual_seed(7)
table = (torch.eye(3, 4).repeat(rows, 1, 1) + 0.1 * (torch.rand((rows, 3, 4), generator=gen) - 0.5)).to("cuda:0")
models = {}
for name in ("autograd_exposure", "fused_exposure", "fused_plain"):
    m = host.SLAMGaussianModel()
    m.loadConfig(dict(capacity=1 << 19, isect_capacity=8 << 20, use_exposure=0 if name == "fused_plain" else 1))
    m.getGaussianParms().add([t.clone() for t in tensors])
    if name != "fused_plain":
        m.getGaussianParms().setExposure(table)
    m.initOptimizers(-1, 1.0)
    models[name] = m
args = (cam, rc["depth_map"], rc["color_map"], rc["depth_map_clamped"])


def step(name):
    m = models[name]
    if name == "autograd_exposure":
        res = m.forward(cam, rc["depth_map"], rc["color_map"])
        m.computeLoss(res, cam, WEIGHTS)["total"].backward()
        m.optimizersStep()
        m.optimizersZeroGrad()
    else:
        m.trainStep(*args, None, WEIGHTS)


for name in models:   # warm-up
    for _ in range(20):
        step(name)
torch.cuda.synchronize()
assert models["fused_exposure"].exposureStep() == 20 == models["autograd_exposure"].exposureStep() and models["fused_plain"].exposureStep() == 0
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
print("N %d, %dx%d, weights %s, camera row %d of %d" % (models["fused_exposure"].getGaussianNum(), W, H, WEIGHTS, int(cam.id), rows))
print("loss terms of the last fused step {total, l1, 1 - ssim, depth}: %s" % [round(float(x), 5) for x in models["fused_exposure"].lossTerms()])
for k in order:
    print("%-18s us/iter: median %.1f  spread %.1f  windows %s" % (k, med[k], max(times[k]) - min(times[k]), " ".join("%.1f" % t for t in times[k])))
print("fused - autograd (exposure): %+.1f us/iter;  exposure on top of the fused terms step: %+.1f us/iter"
      % (med["fused_exposure"] - med["autograd_exposure"], med["fused_exposure"] - med["fused_plain"]))
