"""Densification on an MI355X: three measurements for LABBOOK section 33 (they gate nothing).

  1. gps_densify_accumulate at 200 k Gaussians against the tensor-op sequence of updateDensifyGrad (raw_gs_model.cpp:459-500,
     without max2DSize).
  2. One densification at 200 k with about 10 % clones and 5 % splits: gps_densify_plan + the host's read of the counts +
     gps_densify_apply (parameters and both moments), against an index / cat / index_select formulation of the same result.
  3. An offline raw run (SLAMPipeline::rawTrainCams) on a tests/synth orbit seeded with too few Gaussians, with and without
     densification: Gaussian count and PSNR on held-out views.

Run from the repository root on a GPU box:  python tools/probe/densify.py [--iters 600]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def timed(fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), float(np.min(out))


def accumulate(lib, N=200_000, W=640, H=480):
    g = torch.randn(N, 2, device=DEV) * 1e-4
    radii = torch.randint(-1, 30, (N,), device=DEV, dtype=torch.int32)
    gs, vc = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    kernel = lambda: lib.gps_densify_accumulate(N, g.data_ptr(), radii.data_ptr(), W, H, gs.data_ptr(), vc.data_ptr(), st)
    gs2, vc2 = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)

    def ops():
        mask = (radii > 0).flatten()
        raw = g.detach().clone()
        norm = (raw * torch.tensor([W, H], device=DEV, dtype=raw.dtype) / 2).norm(2, -1)
        vc2.index_put_((mask,), vc2[mask] + 1.0)
        gs2.index_put_((mask,), norm[mask] + gs2[mask])

    return timed(kernel), timed(ops)


def densify_once(lib, N=200_000, K=16):
    rng = np.random.default_rng(0)
    rows = (3, 3, 4, 3, 3 * (K - 1), 1)
    cls = rng.random(N)
    high, large = cls < 0.15, (cls < 0.05)
    ls = np.where(large[:, None], np.log(0.03), np.log(0.004)) + rng.uniform(-0.2, 0.2, (N, 3))
    params = [torch.randn(N, r, device=DEV) for r in rows]
    params[1] = torch.as_tensor(ls.astype(np.float32)).to(DEV)
    params[5] = torch.full((N, 1), 1.0, device=DEV)
    m = [torch.randn(N, r, device=DEV) for r in rows]
    v = [torch.rand(N, r, device=DEV) for r in rows]
    gs = torch.as_tensor(np.where(high, 6e-4, 1e-5).astype(np.float32)).to(DEV)
    vc = torch.full((N,), 3.0, device=DEV)
    thres = (2e-4 * 1.0, 0.01, 0.005, 0.1)
    dst_src = torch.empty(2 * N, dtype=torch.int32, device=DEV)
    dst_sample = torch.empty(2 * N, dtype=torch.int32, device=DEV)
    counts = torch.empty(5, dtype=torch.int32, device=DEV)
    host = torch.zeros(16, dtype=torch.int32).pin_memory()
    ws = torch.empty(int(lib.gps_densify_plan_workspace_bytes(N)), dtype=torch.uint8, device=DEV)
    out = [[torch.empty(2 * N, r, device=DEV) for r in rows] for _ in range(3)]
    samples = torch.randn(2 * N, 3, device=DEV)
    six = lambda ts: (C.c_void_p * 6)(*[t.data_ptr() for t in ts])
    ptrs = [six(params), six(out[0]), six(m), six(out[1]), six(v), six(out[2])]
    st = torch.cuda.current_stream().cuda_stream
    stats = {}

    def kernels():
        assert lib.gps_densify_plan(N, gs.data_ptr(), vc.data_ptr(), params[1].data_ptr(), params[5].data_ptr(), *thres, dst_src.data_ptr(),
                                    dst_sample.data_ptr(), 2 * N, counts.data_ptr(), host.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
        torch.cuda.current_stream().synchronize()
        M, n_split, n_ss, n_ds, n_keep = host[:5].tolist()
        stats["counts"] = (M, n_split, n_ss, n_ds, n_keep)
        assert lib.gps_densify_apply(N, K, M, n_split, n_ss, n_ds, n_keep, dst_src.data_ptr(), dst_sample.data_ptr(), samples.data_ptr(),
                                     *ptrs, st) == 0

    def ops():
        avg = gs / vc.clamp_min(1)
        hi = avg > thres[0]
        smax = params[1].exp().max(1)[0]
        big = smax > thres[1]
        dup, split = hi & ~big, hi & big
        n_split = int(split.sum())
        z = samples[:2 * n_split]
        q = params[2][split]
        q = q / q.norm(dim=-1, keepdim=True)
        w, x, y, zz = q.unbind(-1)
        R = torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y), 2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz),
                         2 * (y * zz - w * x), 2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3).repeat(2, 1, 1)
        child_means = torch.bmm(R, (params[1][split].repeat(2, 1).exp() * z)[..., None])[..., 0] + params[0][split].repeat(2, 1)
        child_scales = torch.log(params[1][split].exp() / 1.6).repeat(2, 1)
        new = []
        for k, p in enumerate(params):
            child = child_means if k == 0 else child_scales if k == 1 else p[split].repeat(2, 1)
            new.append(torch.cat([p, child, p[dup]], 0))
        n_new = new[0].shape[0] - N
        prune = (torch.sigmoid(new[5]) < thres[2]).squeeze(-1) | (new[1].exp().max(-1)[0] > thres[3])
        prune[:N] |= split
        keep = (~prune).nonzero().squeeze(-1)
        res = [torch.index_select(t, 0, keep) for t in new]
        for mom in (m, v):
            res += [torch.index_select(torch.cat([t, torch.zeros(n_new, t.shape[1], device=DEV)], 0), 0, keep) for t in mom]
        return res

    a, b = timed(kernels, reps=15), timed(ops, reps=15)
    return a, b, stats["counts"]


def offline_run(iters):
    from gps_slam_amd import _lib
    _lib.load_library()
    import gps_slam_amd._host as h
    from tests import synth
    W, H, n_cams = 160, 120, 12
    seq = synth.make_sequence(W, H, n_cams, step_deg=2.0)
    cams = []
    for i in range(n_cams):
        c = h.Camera(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], True, torch.as_tensor(seq["c2w"][i].astype(np.float32)))
        c.id = i
        c.image = torch.as_tensor(seq["rgb"][i].astype(np.float32) / 255.0).to(DEV)
        cams.append(c)
    held = [cams[i] for i in (3, 8)]
    train = [c for i, c in enumerate(cams) if i not in (3, 8)]
    # too few Gaussians: every 24th pixel of the first camera's depth
    depth = seq["depth"][0].astype(np.float64) / 1000.0
    ys, xs = np.divmod(np.arange(0, W * H, 24), W)
    d = depth[ys, xs]
    ok = d > 0
    ys, xs, d = ys[ok], xs[ok], d[ok]
    pc = np.stack([(xs - seq["cx"]) / seq["fx"] * d, (ys - seq["cy"]) / seq["fy"] * d, d], -1)
    c2w = seq["c2w"][0].astype(np.float64)
    n = len(d)
    f32 = np.float32
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a.astype(f32))).to(DEV)
    rgb = seq["rgb"][0][ys, xs].astype(np.float64) / 255.0
    tensors = [T(pc @ c2w[:3, :3].T + c2w[:3, 3]), T(np.log(np.repeat((d / seq["fx"] * 2.5)[:, None], 3, 1))),
               T(np.tile([1.0, 0, 0, 0], (n, 1))), T((rgb - 0.5) / 0.28209479177387814), T(np.zeros((n, 15, 3))), T(np.zeros((n, 1)))]
    out = {}
    for densify in (False, True):
        m = h.SLAMGaussianModel()
        m.loadConfig(dict(render_method="raw", capacity=1 << 16, sh_degree=3, sh_degree_interval=100, densify_start_iter=50,
                          densify_end_iter=iters, densify_interval=50, reset_opacity_interval=300, densify_grad_thres=0.0002,
                          densify_large_thres=0.01, prune_opacity_thres=0.005))
        m.getGaussianParms().add([t.clone() for t in tensors])
        pipe = h.SLAMPipeline(3)
        pipe.scene_scale = 3.0
        pipe.setModel(m)
        t0 = time.perf_counter()
        done = pipe.rawTrainCams(train, iters, 3, densify)
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        psnr = []
        with torch.no_grad():
            for c in held:
                img = m.rawForward(c)["rgb"].clamp(0, 1)
                psnr.append(float(-10 * torch.log10(((img - c.image) ** 2).mean())))
        out[densify] = dict(iterations=done, start=n, gaussians=m.getGaussianNum(), events=m.densify_events, psnr=float(np.mean(psnr)), seconds=secs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=600)
    args = ap.parse_args()
    from gps_slam_amd import _lib
    lib = _lib.load_library()
    (k_med, k_min), (o_med, o_min) = accumulate(lib)
    print("accumulate, 200 k Gaussians: kernel %.1f us median (%.1f min), tensor ops %.1f us median (%.1f min)" % (k_med, k_min, o_med, o_min))
    (k_med, k_min), (o_med, o_min), counts = densify_once(lib)
    print("one densification, 200 k Gaussians, counts (M, n_split, n_split_surviving, n_dup_surviving, n_keep) = %s:" % (counts,))
    print("  plan + count read + apply %.1f us median (%.1f min), index / cat / index_select %.1f us median (%.1f min)" % (k_med, k_min, o_med, o_min))
    for densify, r in offline_run(args.iters).items():
        print("offline raw run, densify %s: %d iterations in %.1f s, %d -> %d Gaussians (%d events), held-out PSNR %.2f dB" %
              ("on" if densify else "off", r["iterations"], r["seconds"], r["start"], r["gaussians"], r["events"], r["psnr"]))


if __name__ == "__main__":
    main()
