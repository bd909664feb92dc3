"""Device time of every render pass behind GetImage on a fused 640 x 480 orbit of tests/synth, by the library's launch stamps
(gps_launch_timing_*: the kernel's own execution interval, no host clock): the median over CALLS calls of each type of
gps_tsdf_render_image on the live ray image of the last frame and on a free view's ray image, with the colour-from-volume
kernel (8 voxel reads per pixel against the 32 of the shading kernels) on the same ray images beside them as the yardstick, and
of the false-colour depth's colour pass.  One stamped window per call.

  python tools/probe/get_image.py [--frames 40] [--calls 20] [--out probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from gps_slam_amd._lib import check, lib
from gps_slam_amd.tsdf_engine import TsdfEngine, pose_from_c2w
from tests import synth

W, H = 640, 480
RENDER_IMAGE, RENDER_COLOUR = 13, 14   # GPS_TIMED_RENDER_IMAGE, GPS_TIMED_RENDER_COLOUR
TYPES = {"shaded_greyscale": 0, "shaded_greyscale_imagenormals": 1, "colour_from_volume": 2, "colour_from_normal": 3,
         "colour_from_confidence": 4}   # gps_render_type


def stamped_us(kind, call):
    """device microseconds of the launches of `kind` inside one call"""
    assert lib.gps_launch_timing_start(1 << 14) == 0
    try:
        call()
        torch.cuda.synchronize()
    finally:
        rc = lib.gps_launch_timing_stop()
    assert rc == 0
    tot, totf, mx = C.c_double(), C.c_double(), C.c_double()
    n, nf, dropped = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.gps_launch_timing_read(kind, C.byref(tot), C.byref(n), C.byref(totf), C.byref(nf), C.byref(mx), C.byref(dropped)) == 0
    assert n.value == 1 and dropped.value == 0, (kind, n.value, dropped.value)
    return tot.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    seq = synth.make_sequence(W, H, a.frames, step_deg=0.4)
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    eng = TsdfEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.005, 0.02, device="cuda:0")
    for i in range(a.frames):
        eng.ProcessFrame(torch.from_numpy(rgba[i]).cuda().contiguous(), torch.from_numpy(seq["depth"][i].astype(np.int16)).cuda().contiguous(),
                         seq["c2w"][i])
    M, invM = eng.camPoses[-1]
    fM, fInvM = pose_from_c2w(seq["c2w"][a.frames // 2])   # a free view: the middle of the orbit
    eng.runRaycast(pose=(fM, fInvM))
    out_img = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    scratch = torch.zeros(int(lib.gps_tsdf_depth_to_rgba8_scratch_bytes()), dtype=torch.uint8, device="cuda:0")
    state, st = C.byref(eng.state), eng._stream()
    res = dict(width=W, height=H, frames=a.frames, calls=a.calls, found_share_live=float((eng.raycast.view(-1, 4)[:, 3] > 0).float().mean()),
               found_share_free=float((eng.fv_raycast.view(-1, 4)[:, 3] > 0).float().mean()), median_us={}, min_us={}, max_us={})
    for view, rays, inv in (("live", eng.raycast, invM), ("free", eng.fv_raycast, fInvM)):
        for name, t in TYPES.items():
            kind = RENDER_COLOUR if name == "colour_from_volume" else RENDER_IMAGE
            call = lambda: check(lib.gps_tsdf_render_image(state, rays.data_ptr(), W, H, inv.ctypes.data, t, out_img.data_ptr(), st), name)
            call(); torch.cuda.synchronize()   # code object, caches
            us = sorted(stamped_us(kind, call) for _ in range(a.calls))
            key = view + "/" + name
            res["median_us"][key], res["min_us"][key], res["max_us"][key] = float(np.median(us)), us[0], us[-1]
    call = lambda: check(lib.gps_tsdf_depth_to_rgba8(eng.depth.data_ptr(), W * H, scratch.data_ptr(), out_img.data_ptr(), st), "depth")
    call(); torch.cuda.synchronize()
    us = sorted(stamped_us(RENDER_IMAGE, call) for _ in range(a.calls))
    res["median_us"]["depth_colour_pass"], res["min_us"]["depth_colour_pass"], res["max_us"]["depth_colour_pass"] = float(np.median(us)), us[0], us[-1]
    for view in ("live", "free"):
        c = res["median_us"][view + "/colour_from_volume"]
        res[view + "_shading_over_colour"] = {k: res["median_us"][view + "/" + k] / c for k in ("shaded_greyscale", "colour_from_normal", "colour_from_confidence")}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
