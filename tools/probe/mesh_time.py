"""Device time of gps_tsdf_mesh_scene at 640 x 480 after a fused orbit of tests/synth: median / min / max of N calls (device
events around each call, buffers allocated once).  Run from the repository root of the tree to be timed:
    python tools/probe/mesh_time.py [--frames 8] [--calls 30]
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from gps_slam_amd._lib import lib, check  # noqa: E402
from gps_slam_amd.tsdf_engine import TsdfEngine  # noqa: E402
from tests import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()

W, H = 640, 480
dev = torch.device("cuda:0")
seq = synth.make_sequence(W, H, a.frames, step_deg=1.0)
eng = TsdfEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.005, 0.02, 0.2, 10.0)
for f in range(a.frames):
    eng.ProcessFrame(torch.as_tensor(seq["rgb"][f]).to(dev), torch.as_tensor(seq["depth"][f].astype(np.int16)).to(dev), seq["c2w"][f])
max_tri = 1 << 23
tri = torch.empty((max_tri, 7, 3), dtype=torch.float32, device=dev)
counts = torch.zeros(2, dtype=torch.int64, device=dev)
nbytes = int(lib.gps_tsdf_mesh_workspace_bytes(C.byref(eng.state)))
ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
ms = []
for k in range(a.warmup + a.calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.gps_tsdf_mesh_scene(C.byref(eng.state), max_tri, tri.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, eng._stream()),
          "gps_tsdf_mesh_scene")
    e1.record()
    e1.synchronize()
    if k >= a.warmup:
        ms.append(e0.elapsed_time(e1))
ms.sort()
print(json.dumps({"probe": "mesh_time", "frames": a.frames, "calls": a.calls, "triangles": int(counts[0]), "workspace_bytes": nbytes,
                  "median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}))
