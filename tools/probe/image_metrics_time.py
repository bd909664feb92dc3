"""gps_image_metrics at 640 x 480 with K = 1 and K = 16 uint8 views, with and without a depth mask, against the same numbers from
plain torch ops on the device: to_tensor's convert + divide, the mask multiply, five grouped conv2d with the 11 x 11 window and
the means (what scripts/metric_general.py runs per view, batched over K here, which favours torch).

Per leg: call time from device events around `reps` back-to-back calls after a warm-up of every shape (the window is sized to
~0.5 s of work), both versions alternated `rounds` times in the same process, median and spread over the rounds; the two
versions' PSNR / SSIM are compared before anything is timed.  The C-ABI leg times the entry point alone (workspace and outputs
allocated once), the host leg image_eval.image_metrics as a user calls it (allocations, PSNR and the two means: it ends in a
device -> host read).  No GPU, no number: the probe fails without a device.
One process, one line per leg; ends itself after --limit seconds.   usage (GPU box): python tools/probe/image_metrics_time.py"""
import argparse
import ctypes as C
import math
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import torch.nn.functional as F

from gps_slam_amd import image_eval
from gps_slam_amd._lib import check, lib

DEV = "cuda:0"


def views(K, H, W, seed):
    """smooth uint8 images (sinusoids + noise of ~6 levels), render = gt + noise of ~9 levels, depth with a hole per view"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    gt = np.empty((K, H, W, 3), np.float32)
    for k in range(K):
        for c in range(3):
            fy, fx = rng.uniform(0.01, 0.05, size=2)
            gt[k, ..., c] = 128.0 + 100.0 * np.sin(fy * y + rng.uniform(0, 6.28)) * np.sin(fx * x + rng.uniform(0, 6.28))
    gt += rng.normal(scale=6.0, size=gt.shape).astype(np.float32)
    gt8 = np.clip(np.rint(gt), 0, 255).astype(np.uint8)
    r8 = np.clip(np.rint(gt8 + rng.normal(scale=9.0, size=gt.shape)), 0, 255).astype(np.uint8)
    depth = rng.uniform(0.5, 4.0, size=(K, H, W)).astype(np.float32)
    depth[:, H // 3:H // 2, W // 4:W // 2] = 0.0
    return torch.as_tensor(r8).to(DEV), torch.as_tensor(gt8).to(DEV), torch.as_tensor(depth).to(DEV)


def window():
    g = torch.tensor([math.exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).expand(3, 1, 11, 11).contiguous().to(DEV)


def torch_metrics(r8, g8, depth, w):
    a = r8.permute(0, 3, 1, 2).float().div(255)
    b = g8.permute(0, 3, 1, 2).float().div(255)
    if depth is not None:
        m = (depth > 0).unsqueeze(1)
        a, b = a * m, b * m
    mse = ((a - b) ** 2).flatten(1).mean(1)
    psnr = 20 * torch.log10(1.0 / torch.sqrt(mse))
    conv = lambda t: F.conv2d(t, w, padding=5, groups=3)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    ssim = ((2 * mu1 * mu2 + 0.0001) * (2 * s12 + 0.0009)) / ((mu1 * mu1 + mu2 * mu2 + 0.0001) * (s1 + s2 + 0.0009))
    return psnr, ssim.flatten(1).mean(1)


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    ap.add_argument("--views", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420)
    a = ap.parse_args()
    signal.alarm(a.limit)
    if not torch.cuda.is_available():
        sys.exit("image_metrics_time: no GPU -- nothing measured")
    H, W = a.size
    w = window()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("build flags: %r" % lib.gps_build_flags().decode(), flush=True)
    for K in a.views:
        r8, g8, depth = views(K, H, W, K)
        wb = int(lib.gps_image_metrics_workspace_bytes(K, H, W))
        ws = torch.empty(wb, dtype=torch.uint8, device=DEV)
        mse, ssim = torch.empty(K, dtype=torch.float64, device=DEV), torch.empty(K, dtype=torch.float64, device=DEV)
        sse = torch.empty(K, dtype=torch.int64, device=DEV)
        for masked in (False, True):
            d = depth if masked else None
            abi = lambda: check(lib.gps_image_metrics(K, H, W, 0, r8.data_ptr(), g8.data_ptr(), d.data_ptr() if masked else None,
                                                      ws.data_ptr(), wb, mse.data_ptr(), ssim.data_ptr(), sse.data_ptr(), st), "gps_image_metrics")
            host = lambda: image_eval.image_metrics(r8, g8, d)
            ref = lambda: torch_metrics(r8, g8, d, w)
            # the same numbers first (and the warm-up of every shape)
            ours, (tp, ts) = host(), ref()
            dp = float((ours["psnr"] - tp.double()).abs().max())
            ds = float((ours["ssim"] - ts.double()).abs().max())
            legs = {"c-abi": abi, "host": host, "torch": ref}
            reps = {}
            for name, fn in legs.items():
                fn()
                once = timed(fn, 5)
                reps[name] = max(10, min(20000, int(0.5e6 / max(once, 1.0))))
            times = {name: [] for name in legs}
            for _ in range(a.rounds):
                for name, fn in legs.items():   # alternated: A B C A B C ...
                    times[name].append(timed(fn, reps[name]))
            med = {n: statistics.median(t) for n, t in times.items()}
            line = "K = %2d %dx%d %s: " % (K, W, H, "masked  " if masked else "unmasked")
            line += "  ".join("%s %9.1f us [%.1f .. %.1f, %d reps x %d]" % (n, med[n], min(times[n]), max(times[n]), reps[n], a.rounds)
                              for n in legs)
            line += "  | torch / c-abi %.1fx  | max |psnr diff| %.2e dB, |ssim diff| %.2e (float32 torch)" % (med["torch"] / med["c-abi"], dp, ds)
            print(line, flush=True)


if __name__ == "__main__":
    main()
