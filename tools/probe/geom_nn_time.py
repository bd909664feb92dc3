"""gps_nn_index_build / gps_nn_query on surface samples of the synthetic room (tests/synth.py's walls and spheres): index build,
query and fallback times at 10^5 and 10^6 points per side, against the reference's own way of getting these distances --
scipy.spatial.cKDTree build + query on the host's CPUs (skipped with a note when scipy is not importable).

Legs per size:  near = two independent samples of the same surfaces (every query ends in the ring search);
                far  = the same with 10 % of the queries displaced by 1 m (those end in the brute-force fallback);
                fallback = a call over the displaced queries alone.
One process, one line per size; ends itself after --limit seconds.   usage (GPU box): python tools/probe/geom_nn_time.py"""
import argparse
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch

from gps_slam_amd import geom_eval
from gps_slam_amd._lib import check, lib

DEV = "cuda:0"


def room_points(n, seed):
    half = [3.0, 1.5, 2.5]
    tris = []
    for ax, (u, v) in ((0, (1, 2)), (1, (0, 2)), (2, (0, 1))):
        for sgn in (-1.0, 1.0):
            c = np.zeros((4, 3))
            c[:, ax] = sgn * half[ax]
            c[:, u] = np.array([-1, 1, 1, -1]) * half[u]
            c[:, v] = np.array([-1, -1, 1, 1]) * half[v]
            tris += [c[[0, 1, 2]], c[[0, 2, 3]]]
    n_sph = n // 20
    walls = geom_eval.sample_surface(torch.as_tensor(np.stack(tris).astype(np.float32)).to(DEV), n - 2 * n_sph, seed)[0]
    rng = np.random.default_rng(seed)
    pts = [walls]
    for sx, sy, sz, sr in ((0.4, 0.2, 0.3, 0.45), (-0.8, 0.5, -0.4, 0.35)):
        d = rng.normal(size=(n_sph, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pts.append(torch.as_tensor((np.array([sx, sy, sz]) + sr * d).astype(np.float32)).to(DEV))
    p = torch.cat(pts)
    return p[torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(seed)).to(DEV)].contiguous()


def timed(fn, reps):
    fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    signal.alarm(a.limit)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    print("ring cap build flags: %r" % lib.gps_build_flags().decode(), flush=True)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in a.sizes:
        ref, qry = room_points(n, 1), room_points(n, 2)
        far = qry.clone()
        k = n // 10
        far[:k] += torch.tensor([0.6, 0.64, 0.48], device=DEV)   # |.| = 1 m
        ib, qb = int(lib.gps_nn_index_workspace_bytes(n)), int(lib.gps_nn_query_workspace_bytes(n))
        iws, qws = torch.empty(ib, dtype=torch.uint8, device=DEV), torch.empty(qb, dtype=torch.uint8, device=DEV)
        d2, idx = torch.empty(n, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
        stats = torch.zeros(2, dtype=torch.int32, device=DEV)
        build = lambda: check(lib.gps_nn_index_build(n, ref.data_ptr(), iws.data_ptr(), ib, st), "build")
        query = lambda q, m: (lambda: check(lib.gps_nn_query(n, iws.data_ptr(), m, q.data_ptr(), d2.data_ptr(), idx.data_ptr(),
                                                            stats.data_ptr(), qws.data_ptr(), qb, st), "query"))
        t_build = timed(build, 10)
        t_near = timed(query(qry, n), 10)
        s_near = stats.cpu().tolist()
        t_far = timed(query(far, n), 2)
        s_far = stats.cpu().tolist()
        t_fb = timed(query(far, k), 2)
        s_fb = stats.cpu().tolist()
        line = ("n = %8d: build %9.1f us  query(near) %9.1f us [grid %d / fallback %d]  query(10%% at 1 m) %11.1f us [%d / %d]  "
                "fallback alone (%d queries) %11.1f us [%d / %d]" % (n, t_build, t_near, s_near[0], s_near[1], t_far, s_far[0], s_far[1],
                                                                     k, t_fb, s_fb[0], s_fb[1]))
        if cKDTree is not None and not a.no_scipy:
            r64, q64 = ref.cpu().numpy().astype(np.float64), far.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            tree = cKDTree(r64)
            t1 = time.perf_counter()
            tree.query(q64, workers=16)
            t2 = time.perf_counter()
            line += "  | cKDTree build %.0f us  query(10%% at 1 m, 16 workers) %.0f us" % ((t1 - t0) * 1e6, (t2 - t1) * 1e6)
        else:
            line += "  | cKDTree: scipy not importable here, skipped"
        print(line, flush=True)


if __name__ == "__main__":
    main()
