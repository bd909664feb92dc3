"""What the bilateral-filter fixture (tests/golden/bilateral.npz), its generator and its tests share (data and numpy only): the
kernel cases' millimetre images, the engine sequence with its seeded noise and holes, and a float32 transcription of
DepthFiltering / filterDepth (ITMViewBuilder_CPU.cpp:118-129, ITMViewBuilder_Shared.h:38-67) with the exponential computed in
double and rounded once -- the rule the fixture's reference is pinned to and the device follows."""
import numpy as np

from tests import synth

VOXEL, MU, VF_MIN, VF_MAX = 0.02, 0.08, 0.2, 10.0
# kernel cases (W, H): ragged in both directions and 4 x 7 tiles of the kernel's 32 x 8 (at least 3 x 2 of any tile up to
# 32 x 16); one interior pixel; no interior at all
KERNEL_CASES = {"k100x52": (100, 52), "k5x5": (5, 5), "k4x7": (4, 7)}
# engine runs -> (W, H, frames, step_deg, useApproximateRaycast, mode)
RUNS = {"g": (64, 48, 4, 0.8, False, "given"), "f": (64, 48, 4, 0.8, True, "given"), "t": (160, 120, 4, 0.4, False, "track"),
        "r": (64, 48, 4, 0.8, False, "reloc")}
NOISE_MM = 4   # uniform integer noise in [-NOISE_MM, NOISE_MM]


def kernel_depth(tag):
    """-> int16 [H, W] millimetres: a tilted plane with seeded noise; the large case also has a 2 m step (weights that are
    exactly 0), a comb of 24..46 mm steps (weights in the denormal range), holes -- one touching the two-pixel ring from the
    inside, one inside the ring, a sparse lattice -- and single pixels at 0.2 m, 10 m, 1 mm, a negative value and 32767"""
    W, H = KERNEL_CASES[tag]
    rng = np.random.default_rng(1000 + W * 100 + H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = 1000 + 6 * xs + 3 * ys + rng.integers(-NOISE_MM, NOISE_MM + 1, (H, W))
    if tag == "k100x52":
        d[:, 60:] += 2000
        comb = (ys >= 20) & (ys < 32) & (xs >= 28) & (xs < 44) & (xs % 2 == 1)
        d[comb] += (24 + 2 * (ys - 20))[comb]
        d[10:14, 2:6] = 0                       # touches the ring from the inside
        d[0:2, 0:2] = 0                         # inside the ring
        d[H - 3, W - 3] = 0                     # the last interior pixel
        d[(xs * 7 + ys * 13) % 31 == 0] = 0
        d[5, 10], d[5, 13], d[5, 16], d[5, 19], d[5, 22] = 200, 10000, 1, -5, 32767
        d[40, 70], d[40, 71] = 200, 10000       # the two extremes side by side
    elif tag == "k5x5":
        d[1, 1] = 0
        d[0, 0] = 10000
    else:
        d[3, 1] = 0
    return d.astype(np.int16)


def sequence(tag):
    """-> synth sequence dict of an engine run: depth with seeded integer noise and holes (a rectangle that moves with the frame and
    touches the ring in frame 0, a sparse lattice)"""
    W, H, n, step, _, _ = RUNS[tag]
    seq = synth.make_sequence(W, H, n, step_deg=step)
    rng = np.random.default_rng(77)
    d = seq["depth"].astype(np.int64) + rng.integers(-NOISE_MM, NOISE_MM + 1, seq["depth"].shape)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for f in range(n):
        x0, y0 = 2 + 3 * f, H // 2 + f
        d[f, y0:y0 + H // 8, x0:x0 + W // 10] = 0
        d[f][(xs * 7 + ys * 13 + f * 3) % 97 == 0] = 0
    seq["depth"] = np.clip(d, 0, 32767).astype(seq["depth"].dtype)
    return seq


def convert(mm):
    """convertDepthAffineToFloat with the standard calibration (1 / 1000, 0), float32"""
    f = np.float32
    mm = np.asarray(mm, np.int16)
    return np.where(mm <= 0, f(-1.0), mm.astype(f) * (f(1.0) / f(1000.0)) + f(0.0)).astype(f)


def filter_pass(a, stats=None):
    """DepthFiltering: the cleared output, filterDepth over the interior; float32 operation for operation, the weight
    (float) exp((double) e).  stats (a dict): counts of denormal weights and of weights that are exactly 0 (the centre's own
    weight is 1, so each of those sits beside a non-zero one)."""
    f = np.float32
    a = np.asarray(a, f)
    H, W = a.shape
    out = np.zeros((H, W), f)
    if H < 5 or W < 5:
        return out
    z = a[2:H - 2, 2:W - 2]
    L = f(1.2232)
    with np.errstate(all="ignore"):
        sigma = f(1.0) / (f(0.0012) + f(0.0019) * (z - f(0.4)) * (z - f(0.4)) + f(0.0001) / np.sqrt(z) * f(0.25))
        fd, ws = np.zeros_like(z), np.zeros_like(z)
        n_den = n_zero = 0
        for i in range(-2, 3):
            for j in range(-2, 3):
                t = a[2 + i:H - 2 + i, 2 + j:W - 2 + j]
                use = (t >= 0) & (z >= 0)
                dz = t - z
                dz = dz * dz
                e = f(-0.5) * (f(abs(i) + abs(j)) * L * L + dz * sigma * sigma)
                w = np.exp(e.astype(np.float64)).astype(f)
                w = np.where(use, w, f(0.0))
                n_den += int((use & (w > 0) & (w < f(2.0) ** -126)).sum())
                n_zero += int((use & (w == 0)).sum())
                ws = ws + w
                fd = fd + np.where(use, w * t, f(0.0))
        out[2:H - 2, 2:W - 2] = np.where(z < 0, f(-1.0), fd / ws)
    if stats is not None:
        stats["denormal_weights"] = stats.get("denormal_weights", 0) + n_den
        stats["zero_weights"] = stats.get("zero_weights", 0) + n_zero
    return out


def filter5(mm, stats=None):
    """UpdateView with useBilateralFilter: conversion + five passes -> float32 [H, W]"""
    a = convert(mm)
    for _ in range(5):
        a = filter_pass(a, stats)
    return a


def ring_mask(H, W):
    m = np.ones((H, W), bool)
    if H >= 5 and W >= 5:
        m[2:H - 2, 2:W - 2] = False
    return m
