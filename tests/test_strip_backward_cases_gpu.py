"""The strip backward (gps_raster_ges_bwd_strips) on cases built on purpose, through the C ABI with caller-made class lists.

tests/strip_cases.py holds the cases and the float64 reference; tests/test_strip_cases_cpu.py vets that every case family
really holds the situations it is named for.  Here, per family:
  parity      the strip kernel's rows and the group kernel's outputs, each against the float64 reference, every element within
              2e-5 sum|terms| + SIG (sigma-weighted sum|terms|) + 1e-30 + 1.001 (borderline contribution) -- the constants of
              test_raster_ges_fwd_bwd -- and no more Gaussians needing the last term than the reference lists;
  rows        `rows` starts as a NaN sentinel: exactly the listed ids are written, a listed Gaussian without a contributing
              pixel gets zeros, every other row (row 0 included) keeps the sentinel's bits;
  identities  bit-equal rows under permutations inside the class lists, with the residency reserve on, run twice, and for a
              Gaussian launched alone (a row does not depend on its task neighbours: the file header's "any order gives the
              same rows"; the row arithmetic runs on exact half-integers, padding rows add +0);
  passes      the columns at offsets 63 / 64 / 127 / 128 of each half box (the last of a pass of the 64-lane class, the first of
              the next) must be IN the row: the row differs from (reference - that column pair's share) by more than the bound.
"""
import types

import numpy as np
import pytest
import torch

from tests import strip_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF   # a quiet NaN with a payload
FAMS = list(sc.FAMILIES)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(_dev())


_STATE = {}


def _state(case):
    """device copies of a case: records (gps_raster_pack_records), the pair image, radii, the pixel gradients"""
    from gps_slam_amd import gsplat_ops as ops
    if case["name"] not in _STATE:
        st = types.SimpleNamespace()
        st.radii = T(case["radii"])
        st.recs = ops.raster_pack_records(T(case["m2"]), T(case["conics"]), T(case["colors"]), T(case["opac"]), st.radii)
        st.v_rc = T(case["v_rc"])
        st.pix2 = ops.raster_pair_image(T(case["v_ra"]), T(case["ref_depth"]), case["W"], case["H"], case["delta"])
        _STATE[case["name"]] = st
    return _STATE[case["name"]]


def _launch(case, lists=None):
    """-> rows[N,12] (device), prefilled with the sentinel, after one launch on `lists` (default: the case's own)"""
    from gps_slam_amd import gsplat_ops as ops
    st = _state(case)
    lists = case["lists"] if lists is None else lists
    N = case["radii"].size
    stride = max(len(L) for L in lists) + 5          # (not N, and more than any count: the padding is never read)
    ids = np.zeros((5, stride), np.int32)
    counts = np.zeros(8, np.int32)
    for k, L in enumerate(lists):
        ids[k, :len(L)] = L
        counts[k] = len(L)
    rows = torch.full((N, 12), SENTINEL, dtype=torch.int32, device=_dev()).view(torch.float32)
    out = ops.raster_ges_bwd_strips_lists(st.recs, st.radii, T(ids), T(counts), st.v_rc, st.pix2, case["W"], case["H"], rows)
    assert out.data_ptr() == rows.data_ptr()
    return rows


def _bits(rows):
    return rows.view(torch.int32)


def _listed(case):
    return np.sort(np.concatenate(case["lists"])).astype(np.int64)


def _groups(case):
    """the group kernel (rasterize_to_pixels_bwd_ges_gs_parallel) on the same inputs, group table from the oracle -> [N,10]"""
    from gps_slam_amd import gsplat_ops as ops
    from oracle import splat_ref as orc
    W, H, TS = case["W"], case["H"], 16
    tw, th = (W + TS - 1) // TS, (H + TS - 1) // TS
    tpg, _, flat, ggs, gst, _ = orc.isect_tiles(case["m2"], case["radii"], TS, tw, th)
    assert ggs.size > 0
    isect = types.SimpleNamespace(group_gs_ids=T(ggs), group_starts=T(gst),
                                  counts=torch.tensor([flat.size, ggs.size, 0, 0], dtype=torch.int64, device=_dev()))
    N = case["radii"].size
    o = ops.rasterize_to_pixels_bwd_ges_gs_parallel(T(case["m2"])[None], T(case["conics"])[None], T(case["colors"])[None],
                                                    T(case["opac"])[:, None], T(case["radii"])[None], T(case["ref_depth"])[None, ..., None],
                                                    W, H, isect, case["delta"], T(case["v_rc"])[None], T(case["v_ra"])[None, ..., None])
    n = lambda t: t.detach().cpu().numpy()
    return np.concatenate([n(o[2]).reshape(N, 4), n(o[1]).reshape(N, 3), n(o[0]).reshape(N, 2), n(o[3]).reshape(N, 1)], 1).astype(np.float64)


@pytest.mark.parametrize("fam", FAMS)
def test_strip_and_group_kernels_match_the_float64_reference(fam):
    worst = {"strips": 0.0, "groups": 0.0}
    for case in sc.family(fam):
        ref = case["ref"]
        base, tol = sc.tolerance(ref)
        listed = _listed(case)
        rows = _launch(case).cpu().numpy().astype(np.float64)
        for name, got, sel in (("strips", rows[:, :10], listed), ("groups", _groups(case), np.arange(case["radii"].size))):
            d = np.abs(got[sel] - ref["sums"][sel])
            if sel.size:
                worst[name] = max(worst[name], float((d / (sc.REL * ref["scale"][sel] + 1e-30)).max()))
            bad = d > tol[sel]
            assert not bad.any(), (case["name"], name, [(int(sel[i]), int(e), float(d[i, e]), float(tol[sel][i, e])) for i, e in np.argwhere(bad)[:8]])
            flipped = int((d > base[sel]).any(1).sum())
            assert flipped <= len(ref["flip_gauss"]), (case["name"], name, flipped, ref["flip_gauss"])
    print("%s: largest error / (2e-5 sum|terms|): strips %.4f, groups %.4f" % (fam, worst["strips"], worst["groups"]))


@pytest.mark.parametrize("fam", FAMS)
def test_exactly_the_listed_rows_are_written(fam):
    for case in sc.family(fam):
        ref = case["ref"]
        N = case["radii"].size
        listed = _listed(case)
        unlisted = np.setdiff1d(np.arange(N), listed)
        assert 0 in unlisted
        rows = _launch(case)
        bits = _bits(rows).cpu().numpy()
        vals = rows.cpu().numpy()
        assert (bits[unlisted] == SENTINEL).all(), (case["name"], "a row no list names was written", unlisted[(bits[unlisted] != SENTINEL).any(1)][:8].tolist())
        assert np.isfinite(vals[listed]).all(), (case["name"], "a listed row was not written", listed[~np.isfinite(vals[listed]).all(1)][:8].tolist())
        assert (vals[listed][:, 10:] == 0).all()
        empty = listed[(ref["scale"][listed] == 0).all(1) & (ref["flip"][listed] == 0).all(1)]
        assert (vals[empty] == 0).all(), (case["name"], "no contributing pixel: a row of zeros", empty[(vals[empty] != 0).any(1)][:8].tolist())
        if fam in ("edges", "spans", "mixed", "values"):
            assert empty.size > 0


def _solo_picks(case, per_class):
    picks = []
    for k, L in enumerate(case["lists"]):
        for g in ([] if L.size == 0 else sorted({int(L[0]), int(L[-1])})[:per_class]):
            picks.append((k, g))
    return picks


@pytest.mark.parametrize("fam", FAMS)
def test_rows_are_bit_identical_under_list_order_reserve_rerun_and_solo_launch(fam):
    from gps_slam_amd import _lib
    cases = sc.family(fam)
    per_class = 2 if len(cases) <= 2 else 1
    n_solo = 0
    for case in cases:
        base = _bits(_launch(case)).clone()
        assert torch.equal(_bits(_launch(case)), base), (case["name"], "two runs")
        rng = np.random.default_rng(case["seed"] + 77)
        for n in range(3):
            perm = [L[::-1].copy() if n == 0 else rng.permutation(L) for L in case["lists"]]
            assert torch.equal(_bits(_launch(case, perm)), base), (case["name"], "permutation %d inside the class lists" % n)
        _lib.load_library().gps_set_frame_chain_reserve(1)
        try:
            reserved = _bits(_launch(case))
        finally:
            _lib.load_library().gps_set_frame_chain_reserve(0)
        assert torch.equal(reserved, base), (case["name"], "residency reserve")
        for k, g in _solo_picks(case, per_class):
            n_solo += 1
            lists = [np.array([g], np.int32) if c == k else np.zeros(0, np.int32) for c in range(5)]
            solo = _bits(_launch(case, lists))
            assert torch.equal(solo[g], base[g]), (case["name"], "Gaussian %d of class %d alone" % (g, k))
            others = torch.ones(solo.shape[0], dtype=torch.bool, device=solo.device)
            others[g] = False
            assert bool((solo[others] == SENTINEL).all()), (case["name"], "solo launch of %d wrote another row" % g)
    assert n_solo <= 64
    assert n_solo > 0


def test_columns_on_both_sides_of_a_pass_boundary_are_in_the_row():
    (case,) = sc.family("ladder")
    ref = case["ref"]
    base, tol = sc.tolerance(ref)
    rows = _launch(case).cpu().numpy().astype(np.float64)[:, :10]
    checked = 0
    for r in (64, 65, 128, 129):
        for shape in ("wide", "narrow", "aniso"):
            (g,) = case["tags"]["r%d_%s" % (r, shape)]
            for offset in (63, 64, 127, 128):
                if offset >= r:
                    continue
                share, n_px = sc.column_share_f64(case, g, offset)
                if n_px == 0:       # (an ellipse-limited shape does not reach every offset; the wide one reaches them all)
                    assert shape != "wide"
                    continue
                without = ref["sums"][g] - share
                assert (np.abs(rows[g] - without) > tol[g]).any(), ("r=%d %s: columns %d and %d are missing from the row" % (r, shape, offset, offset + r))
                assert (np.abs(rows[g] - ref["sums"][g]) <= tol[g]).all()
                checked += 1
    assert checked >= 24   # every radius at its offsets for the wide shape, the centre columns of the others
