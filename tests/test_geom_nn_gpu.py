"""gps_nn_index_build / gps_nn_query through the C-ABI: exact nearest neighbour between two point sets, against the float64
distances of tests/golden/geo_eval_ref.npz (scipy's cKDTree on the same float32 points, written by
tests/golden/make_geo_eval_golden.py) and, for the edge shapes, against a float64 brute force computed here.

Bound on a distance d = sqrt(dist2): |d - d_ref| <= 2^-21 d_ref.  Each coordinate difference is one float subtraction of
float32 inputs (relative error 2^-24), the fma chain and the square root add about three more roundings of that size, and the
factor two covers the selection of a different neighbour that is as near within that error.  d_ref = 0 must give exactly 0."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL = 2.0 ** -21
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geo_eval_ref.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def nn(ref, query, want_index=True, keep_index_ws=False):
    """-> dist2 float32[Q], index int32[Q] (or None), stats int32[2], all numpy"""
    from gps_slam_amd._lib import check, lib
    ref_d = torch.as_tensor(np.ascontiguousarray(ref, np.float32)).to(DEV)
    q_d = torch.as_tensor(np.ascontiguousarray(query, np.float32)).to(DEV)
    R, Q = ref_d.shape[0], q_d.shape[0]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ib, qb = int(lib.gps_nn_index_workspace_bytes(R)), int(lib.gps_nn_query_workspace_bytes(Q))
    # garbage, not zeros: the workspaces need no initialisation
    iws = torch.full((ib,), 0xA5, dtype=torch.uint8, device=DEV)
    qws = torch.full((qb,), 0x5A, dtype=torch.uint8, device=DEV)
    d2 = torch.full((max(Q, 1),), -1.0, dtype=torch.float32, device=DEV)
    idx = torch.full((max(Q, 1),), -7, dtype=torch.int32, device=DEV)
    stats = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    check(lib.gps_nn_index_build(R, ref_d.data_ptr(), iws.data_ptr(), ib, st), "gps_nn_index_build")
    check(lib.gps_nn_query(R, iws.data_ptr(), Q, q_d.data_ptr(), d2.data_ptr(), idx.data_ptr() if want_index else None,
                           stats.data_ptr(), qws.data_ptr(), qb, st), "gps_nn_query")
    torch.cuda.synchronize()
    out = (d2.cpu().numpy()[:Q], idx.cpu().numpy()[:Q] if want_index else None, stats.cpu().numpy())
    return out + (iws,) if keep_index_ws else out


def brute64(ref, query):
    """float64 brute force on the float32 values -> (distance, lowest index of the minimum)"""
    r, q = np.asarray(ref, np.float32).astype(np.float64), np.asarray(query, np.float32).astype(np.float64)
    d = np.empty(len(q))
    i = np.empty(len(q), np.int64)
    for s in range(0, len(q), 512):
        dd = np.sqrt(((q[s:s + 512, None, :] - r[None, :, :]) ** 2).sum(-1))
        i[s:s + 512] = dd.argmin(1)
        d[s:s + 512] = dd.min(1)
    return d, i


def check_against(ref, query, d2, idx, d_ref):
    d = np.sqrt(d2).astype(np.float64)   # float32 square root, as the hosts return it
    err = np.abs(d - d_ref)
    worst = int(np.argmax(err - REL * d_ref))
    assert np.all(err <= REL * d_ref), (worst, d[worst], d_ref[worst])
    assert np.all(d[d_ref == 0] == 0)
    if idx is not None:
        assert idx.min() >= 0 and idx.max() < len(ref)
        r, q = np.asarray(ref, np.float32).astype(np.float64), np.asarray(query, np.float32).astype(np.float64)
        d_idx = np.sqrt(((q - r[idx]) ** 2).sum(-1))   # the neighbour named is as near as the reference's
        assert np.all(np.abs(d_idx - d_ref) <= REL * d_ref)


def test_fixture_sets_agree_with_the_float64_reference_on_both_paths(gold):
    gt, rec = gold["gt"], gold["rec"]
    # accuracy direction: the reconstruction's far blob is tens of metres from the ground truth -> ring search AND fallback
    d2, idx, stats = nn(gt, rec)
    print("accuracy: stats", stats, "max rel err", float(np.max(np.abs(np.sqrt(d2) - gold["d_acc"]) / np.maximum(gold["d_acc"], 1e-30))))
    check_against(gt, rec, d2, idx, gold["d_acc"])
    assert stats[0] > 0 and stats[1] > 0 and stats[0] + stats[1] == len(rec), stats
    assert stats[1] >= int(gold["param_n_blob"])
    # completion direction: distances up to most of a metre where the reconstruction has a hole
    d2c, idxc, statsc = nn(rec, gt)
    print("completion: stats", statsc, "max rel err", float(np.max(np.abs(np.sqrt(d2c) - gold["d_comp"]) / np.maximum(gold["d_comp"], 1e-30))))
    check_against(rec, gt, d2c, idxc, gold["d_comp"])
    assert statsc[0] + statsc[1] == len(gt) and statsc[0] > 0, statsc
    # two runs: bit-identical in both outputs (the scatter's atomic order differs, the tie rule makes the index reproducible)
    d2b, idxb, statsb = nn(gt, rec)
    assert np.array_equal(d2.view(np.uint32), d2b.view(np.uint32)) and np.array_equal(idx, idxb) and np.array_equal(stats, statsb)
    # the index output is optional, the distances do not depend on it
    d2n, none, _ = nn(gt, rec, want_index=False)
    assert none is None and np.array_equal(d2.view(np.uint32), d2n.view(np.uint32))


def test_query_set_equal_to_the_reference_set_never_leaves_the_grid(gold):
    gt = gold["gt"]
    d2, idx, stats = nn(gt, gt)
    assert np.all(d2 == 0) and stats[1] == 0 and stats[0] == len(gt), stats
    assert np.array_equal(idx, brute64(gt, gt)[1])   # itself, or the lowest-indexed exact duplicate of itself


def test_exact_duplicates_resolve_to_the_lowest_index(gold):
    rng = np.random.default_rng(3)
    ref = gold["gt"][:3000].copy()
    src = rng.choice(1000, size=400, replace=False)            # 400 of the first 1000 points ...
    for k, s in enumerate(src):                                # ... each duplicated twice at higher indices
        ref[1000 + k] = ref[s]
        ref[2000 + 2 * k] = ref[s]
    far = np.array([[50.0, 0.0, 0.0]], np.float32)
    ref[2900:2950] = far[0]                                    # and 50 coincident points, reached only by the fallback
    query = np.concatenate([ref[1000:1400], ref[2000:2800:2], far + np.array([[0.0, 30.0, 0.0]], np.float32)])   # 30 m off the box
    d2, idx, stats = nn(ref, query)
    d_ref, i_ref = brute64(ref, query)
    assert np.all(d2[:800] == 0)
    assert np.array_equal(idx[:400], src) and np.array_equal(idx[400:800], idx[:400])
    assert np.array_equal(idx, i_ref)
    assert idx[800] == 2900 and stats[1] >= 1                  # the lowest of the 50, on the fallback path too
    for _ in range(2):                                         # run to run
        d2b, idxb, _s = nn(ref, query)
        assert np.array_equal(idx, idxb) and np.array_equal(d2.view(np.uint32), d2b.view(np.uint32))


def _edge_sets():
    rng = np.random.default_rng(17)
    box = lambda n: rng.uniform(-1.0, 1.0, size=(n, 3)).astype(np.float32)
    planar = box(300)
    planar[:, 1] = 0.25
    return {
        "R=1": (box(1), box(130)),
        "coincident reference": (np.repeat(box(1), 64, 0), box(70)),
        "planar reference": (planar, box(200)),
        "Q=1": (box(500), box(1)),
        "Q=65 R=257": (box(257), box(65)),
        "one block and a bit": (box(4100), np.concatenate([box(2049), 3.0 * box(200)])),
    }


@pytest.mark.parametrize("name", ["R=1", "coincident reference", "planar reference", "Q=1", "Q=65 R=257", "one block and a bit"])
def test_edge_shapes_against_a_float64_brute_force(name):
    ref, query = _edge_sets()[name]
    d2, idx, stats = nn(ref, query)
    d_ref, i_ref = brute64(ref, query)
    check_against(ref, query, d2, idx, d_ref)
    assert stats[0] + stats[1] == len(query) and stats.min() >= 0
    if name == "coincident reference":
        assert np.all(idx == 0)


def test_queries_exactly_on_cell_faces(gold):
    ref = gold["rec"][:-int(gold["param_n_blob"])]   # the box without the far blob: cells of a few centimetres
    d2, idx, stats, iws = nn(ref, ref[:1], keep_index_ws=True)
    head = iws[:64].cpu().numpy()
    mn, h = head[:12].view(np.float32).astype(np.float64), float(head[16:20].view(np.float32)[0])
    g = head[20:32].view(np.int32)
    assert h > 0 and g.min() >= 1
    rng = np.random.default_rng(23)
    k = np.stack([rng.integers(0, g[a] + 1, size=600) for a in range(3)], 1)
    on_faces = (mn + k * h).astype(np.float32)                              # grid corners: on three faces at once
    on_one = on_faces.copy()
    on_one[:, 1:] += rng.uniform(0, h, size=(600, 2)).astype(np.float32)    # on an x face only
    ext = (ref.max(0) - ref.min(0)).astype(np.float64)
    nudged = (ref[:600].astype(np.float64) + 0.5 * ext / 1024.0).astype(np.float32)
    query = np.concatenate([on_faces, on_one, nudged])
    d2, idx, stats = nn(ref, query)
    d_ref, _ = brute64(ref, query)
    check_against(ref, query, d2, idx, d_ref)
    assert stats[0] + stats[1] == len(query)


def test_far_and_non_finite_queries_return_in_bounded_time(gold):
    gt = gold["gt"]
    finite = np.array([[1e6, 0.5, 0.5], [-1e6, 1e6, 1e6], [0.3, 0.4, 1e6], [0.0, 0.0, 0.0]], np.float32)
    finite[3] = gt[0] + np.array([0.004, -0.003, 0.002], np.float32)   # millimetres from the surface: the ring search finishes it
    bad = np.array([[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    # the reference set carries non-finite points too: they are nobody's neighbour
    ref = np.concatenate([gt, np.array([[np.nan, 0.5, 0.5], [np.inf, 0.5, 0.5], [1.0, 0.7, np.nan]], np.float32)])
    query = np.concatenate([finite, bad])
    t0 = time.perf_counter()
    d2, idx, stats = nn(ref, query)
    elapsed = time.perf_counter() - t0
    d_ref, _ = brute64(gt, finite)
    check_against(gt, finite, d2[:4], idx[:4], d_ref)
    assert np.all(np.isposinf(d2[4:])) and np.all(idx[4:] == -1)
    # the three far queries cannot finish within the ring cap: the fallback took them; the non-finite ones never walked the grid
    assert stats[1] == 3 and stats[0] == 5, stats
    assert elapsed < 10.0, elapsed
    # every query far away (a caller's wrong transform): all of them on the fallback, still exact
    moved = gt[:700] + np.array([40.0, -25.0, 10.0], np.float32)
    d2m, idxm, statsm = nn(gt, moved)
    d_refm, _ = brute64(gt, moved)
    check_against(gt, moved, d2m, idxm, d_refm)
    assert statsm[1] == 700 and statsm[0] == 0, statsm


def test_q_zero_is_a_no_op_and_small_workspaces_are_refused():
    from gps_slam_amd._lib import lib
    ref = torch.rand((100, 3), device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ib = int(lib.gps_nn_index_workspace_bytes(100))
    iws = torch.empty(ib, dtype=torch.uint8, device=DEV)
    assert lib.gps_nn_index_build(100, ref.data_ptr(), iws.data_ptr(), ib - 1, st) == -3
    assert lib.gps_nn_index_build(100, ref.data_ptr(), iws.data_ptr(), ib, st) == 0
    assert lib.gps_nn_query(100, iws.data_ptr(), 0, None, None, None, None, None, 0, st) == 0
    qb = int(lib.gps_nn_query_workspace_bytes(10))
    qws = torch.empty(qb, dtype=torch.uint8, device=DEV)
    d2 = torch.empty(10, device=DEV)
    assert lib.gps_nn_query(100, iws.data_ptr(), 10, ref.data_ptr(), d2.data_ptr(), None, None, qws.data_ptr(), qb - 1, st) == -3
    assert lib.gps_nn_query(100, iws.data_ptr(), 10, ref.data_ptr(), d2.data_ptr(), None, None, qws.data_ptr(), qb, st) == 0
    torch.cuda.synchronize()
    assert torch.all(d2 == 0)
