"""Cost of per-frame exposure compensation (use_exposure) in the C++ host's trainStep: the bench scene's optimise iteration at
640x480 (~200 k Gaussians), one model with exposure on (the camera has a row) and one with it off, timed alternately in one
process (HIP events around blocks of 50 iterations, 6 rounds; both models start from the same Gaussians).
usage: python tools/probe/exposure_ab.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench
from gps_slam_amd.dist_util import cap_host_threads

W, H, NG, BLOCK, ROUNDS = 640, 480, 200000, 50, 6
cap_host_threads()
seq = bench.synthetic_sequence(W, H, 31, 1234)
seeds = bench.seed_gaussians(seq, NG, 1234, "cuda:0")
scene = bench.Scene(seq, seeds, 1234, True, False, 31, 1.0, 0.02)
scene.run(0, 31)
import gps_slam_amd._host as host

cp = scene.model.getGaussianParms()
tensors = [cp.getMeans(), cp.getScales(), cp.getQuats(), cp.getFeaturesDc(), cp.getFeaturesRest(), cp.getOpacities()]
cam, rc = scene.pipe.optCams()[-1], scene.pipe.optRaycasts()[-1]
models = {}
for name, on in (("off", 0), ("on", 1)):
    m = host.SLAMGaussianModel()
    m.loadConfig(dict(capacity=1 << 19, isect_capacity=8 << 20, use_exposure=on))
    m.getGaussianParms().add([t.clone() for t in tensors])
    m.getGaussianParms().setExposure(torch.eye(3, 4, device="cuda:0").repeat(max(cam.id, 0) + 1, 1, 1))
    m.initOptimizers(-1, 1.0)
    models[name] = m
args = (cam, rc["depth_map"], rc["color_map"], rc["depth_map_clamped"])
for m in models.values():   # warm-up
    for _ in range(20):
        m.trainStep(*args)
torch.cuda.synchronize()
times = {k: [] for k in models}
for r in range(ROUNDS):
    for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
        m = models[name]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(BLOCK):
            m.trainStep(*args)
        b.record()
        torch.cuda.synchronize()
        times[name].append(1e3 * a.elapsed_time(b) / BLOCK)
assert models["on"].exposureStep() > 0 and models["off"].exposureStep() == 0
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print("N %d, cam.id %d" % (models["on"].getGaussianNum(), cam.id))
for k in ("off", "on"):
    print("%-3s us/iter: median %.1f  blocks %s" % (k, med[k], " ".join("%.1f" % t for t in times[k])))
print("exposure cost: %+.1f us/iter (median of %d blocks of %d)" % (med["on"] - med["off"], ROUNDS, BLOCK))
