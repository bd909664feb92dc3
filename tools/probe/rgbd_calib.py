"""What the RGB-D calibration's launches cost at 640 x 480 on the synthetic room (tests/synth):

  * the integration launch by the library's launch stamps (gps_launch_timing_*): the one-camera kernel (gps_tsdf_integrate) and
    the instantiation with a colour camera of its own (gps_tsdf_integrate_rgb; a 640 x 480 colour camera 2.5 cm beside the
    depth camera), median over --launches launches on the same visible list;
  * the calibrated conversion (affine 1 / 5000 + 0.01, and Kinect) and the colour registration, averaged over back-to-back
    launches between two events.

--plain times the one-camera integration only: the same script then runs on a tree from before the calibration existed.

  python tools/probe/rgbd_calib.py [--frames 3] [--launches 20] [--plain] [--out probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from gps_slam_amd._lib import check, lib  # noqa: E402
from gps_slam_amd.tsdf_engine import TsdfEngine  # noqa: E402
from tests import synth  # noqa: E402

INTEGRATE = 6   # GPS_TIMED_INTEGRATE
DEV = "cuda:0"


def stamped_us(fn, n):
    """median device time (us) of n launches of fn(), each in a timing window of its own"""
    us = []
    for _ in range(n):
        assert lib.gps_launch_timing_start(1 << 16) == 0
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            rc = lib.gps_launch_timing_stop()
        assert rc == 0
        tot, totf, mx = C.c_double(), C.c_double(), C.c_double()
        cnt, nf, dropped = C.c_int64(), C.c_int64(), C.c_int64()
        assert lib.gps_launch_timing_read(INTEGRATE, C.byref(tot), C.byref(cnt), C.byref(totf), C.byref(nf), C.byref(mx), C.byref(dropped)) == 0
        assert cnt.value == 1 and dropped.value == 0, (cnt.value, dropped.value)
        us.append(tot.value)
    return float(np.median(us))


def event_us(fn, n=200):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(n):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = 640, 480
    seq = synth.make_sequence(W, H, a.frames, step_deg=0.4)
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    rgb, dep = torch.as_tensor(rgba).to(DEV), torch.as_tensor(seq["depth"].astype(np.int16)).to(DEV)
    eng = TsdfEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], device=DEV)
    for f in range(a.frames):
        M, invM = eng.ProcessFrame(rgb[f], dep[f], seq["c2w"][f])
    torch.cuda.synchronize()
    res = {"width": W, "height": H, "visible_blocks": int(eng.counters_host()[2])}
    st = eng._stream()
    res["integrate_us"] = stamped_us(lambda: check(lib.gps_tsdf_integrate(C.byref(eng.state), M.ctypes.data, st), "gps_tsdf_integrate"), a.launches)
    if not a.plain:
        from gps_slam_amd._lib import DepthCalib
        from gps_slam_amd.rgbd_calib import TRAFO_AFFINE, TRAFO_KINECT, RGBDCalib
        calib = RGBDCalib()
        calib.intrinsics_d.SetFrom(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"])
        calib.intrinsics_rgb.SetFrom(W, H, seq["fx"] * 1.1, seq["fy"] * 1.1, seq["cx"] + 3.0, seq["cy"] - 2.0)
        ext = np.eye(4, dtype=np.float32)
        ext[0, 3] = 0.025
        calib.trafo_rgb_to_depth.SetFrom(np.ascontiguousarray(ext.T).reshape(16))
        cam = calib.colour_camera(rgb[-1].data_ptr())
        res["integrate_rgb_us"] = stamped_us(lambda: check(lib.gps_tsdf_integrate_rgb(C.byref(eng.state), M.ctypes.data, C.byref(cam), st),
                                                           "gps_tsdf_integrate_rgb"), a.launches)
        for name, dc in (("convert_affine_us", DepthCalib(TRAFO_AFFINE, 0.0002, 0.01)), ("convert_kinect_us", DepthCalib(TRAFO_KINECT, 1090.0, 3.0))):
            res[name] = event_us(lambda: check(lib.gps_tsdf_convert_depth_calib(C.byref(eng.state), dep[-1].data_ptr(), C.byref(dc), st), name))
        res["convert_standard_us"] = event_us(lambda: check(lib.gps_tsdf_convert_depth(C.byref(eng.state), dep[-1].data_ptr(), st), "gps_tsdf_convert_depth"))
        out = torch.empty((H, W, 4), dtype=torch.uint8, device=DEV)
        res["register_colour_us"] = event_us(lambda: check(lib.gps_tsdf_register_colour(C.byref(eng.state), C.byref(cam), out.data_ptr(), st),
                                                           "gps_tsdf_register_colour"))
        res["registered_share"] = float((out[..., 3] == 255).float().mean().item())
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    main()
