"""The strip-backward case set (tests/strip_cases.py), vetted without a GPU.

On every case the float64 reference of the operation (box_backward_f64: numpy, one Gaussian at a time over its box, exp) and
the C oracle's restatement of the reference kernel (orc.raster_ges_bwd_gs: float32, 32-pixel groups, expf) must agree within
    2e-5 sum|terms| + SIG (sigma-weighted sum|terms|) + 1.001 (contribution of the borderline pairs),
both must regard the same (Gaussian, pixel) pairs as borderline up to the band, and every family must really hold a Gaussian
in each situation it is named for.  At most 10 % of the Gaussians of any case may have a borderline pair: a condition on the
case set (the seeds in strip_cases.py are chosen so that the reference alone meets it), not a tolerance.
"""
import numpy as np
import pytest

from tests import strip_cases as sc


def _oracle(case):
    from oracle import splat_ref as orc
    W, H, TS = case["W"], case["H"], 16
    tw, th = (W + TS - 1) // TS, (H + TS - 1) // TS
    _, _, _, ggs, gst, _ = orc.isect_tiles(case["m2"], case["radii"], TS, tw, th)
    args = (case["m2"], case["conics"], case["colors"], case["opac"], case["radii"], case["ref_depth"], W, H, ggs, gst, case["delta"],
            case["v_rc"], case["v_ra"])
    e = orc.raster_ges_bwd_gs(*args)
    budget, n_pairs, n_g = orc.raster_ges_bwd_gs_flip_budget(*args, rel_band=sc.BAND)
    return np.concatenate([e[2], e[1], e[0], e[3][:, None]], 1).astype(np.float64), budget, n_pairs


@pytest.mark.parametrize("fam", list(sc.FAMILIES))
def test_float64_reference_agrees_with_the_oracle_on_every_case(fam):
    worst, share = 0.0, 0.0
    for case in sc.family(fam):
        ref = case["ref"]
        got, budget, n_pairs = _oracle(case)
        base, tol = sc.tolerance(ref)
        d = np.abs(got - ref["sums"])
        worst = max(worst, float((d / (sc.REL * ref["scale"] + 1e-30)).max()))
        assert (d <= tol).all(), (case["name"], np.argwhere(d > tol)[:5].tolist(), float((d / tol).max()))
        assert int((d > base).any(1).sum()) <= len(ref["flip_gauss"]), case["name"]
        # the same borderline pairs up to the band: what the reference lists in half the band the oracle lists too, and what the
        # oracle lists the reference lists in twice the band (float32 sigma and expf move o vis by a few 1e-7 relative)
        inner, outer = sc.borderline_pairs(case, 0.5 * sc.BAND), sc.borderline_pairs(case, 2.0 * sc.BAND)
        assert sc.borderline_pairs(case, sc.BAND) == ref["pairs"]
        orc_gauss = set(np.nonzero(budget.any(1))[0].tolist())
        assert {p[0] for p in inner} <= orc_gauss <= {p[0] for p in outer}, (case["name"], sorted(orc_gauss), ref["flip_gauss"])
        assert len(inner) <= n_pairs <= len(outer), (case["name"], len(inner), n_pairs, len(outer))
        # a condition on the case set
        N = case["radii"].size
        share = max(share, len(ref["flip_gauss"]) / N)
        assert 10 * len(ref["flip_gauss"]) <= N, (case["name"], ref["flip_gauss"], N)
    print("%s: largest share of Gaussians with a borderline pair %.1f %%, oracle error / (2e-5 sum|terms|) <= %.3f" % (fam, 100 * share, worst))


def _tag(case, name):
    ids = case["tags"].get(name, [])
    assert ids, (case["name"], name)
    return ids


def test_ladder_holds_every_radius_in_three_shapes_and_the_pass_boundaries():
    (case,) = sc.family("ladder")
    ref, radii = case["ref"], case["radii"]
    assert sorted(set(radii[1:].tolist())) == list(sc.LADDER) and radii[0] == 0
    listed = np.concatenate(case["lists"])
    assert sorted(listed.tolist()) == list(range(1, radii.size))
    for r in sc.LADDER:
        (gw,), (gn,), (ga,) = (_tag(case, "r%d_%s" % (r, s)) for s in ("wide", "narrow", "aniso"))
        cw, cn, ca = (sc.contributing_columns(case, g) for g in (gw, gn, ga))
        x0 = int(case["m2"][gw, 0]) - r + 1
        assert x0 >= 0 and x0 + 2 * r <= case["W"], "the box fits between the left and right edge"
        assert cw.tolist() == list(range(2 * r)), ("box-limited", r)
        assert ref["rows"][gw] == min(2 * r, case["H"]) or r > 150, r
        if r >= 3:
            assert 0 < cn.size < 2 * r and 0 < ref["rows"][gn] < 2 * r, ("ellipse-limited", r)
        assert case["conics"][ga, 1] != 0
        a, b, c = (float(v) for v in case["conics"][ga])   # half extents of {alpha >= 1/255}: sqrt(2 tau c / det), sqrt(2 tau a / det)
        assert max(c / a, a / c) >= 9 and b != 0, ("x and y extents differ by 3x or more", r)
        # passes of the 64-lane class: pass p holds the offsets 64 p .. 64 p + 63 of each half box
        for p in range(1, 4):
            if r > 64 * p:
                for g, cols in ((gw, cw), (gn, cn), (ga, ca)):
                    assert ((cols < r) & (cols >= 64 * p)).any(), (r, p, "left half")
                assert (cw >= r + 64 * p).any(), (r, p, "right half")
    for r in (129, 193):
        for s in ("wide", "narrow", "aniso"):
            cols = sc.contributing_columns(case, _tag(case, "r%d_%s" % (r, s))[0])
            assert ((cols % r) >= 128).any()


def test_edges_hold_every_placement_at_both_image_sizes():
    big, small = sc.family("edges")
    assert (big["W"], big["H"], small["W"], small["H"]) == (448, 320, 33, 17)
    for case in (big, small):
        ref, W, H = case["ref"], case["W"], case["H"]
        wide_ids = set(_tag(case, "wide"))
        for tag in ("left", "right", "top", "bottom", "corner_tl", "corner_tr", "corner_bl", "corner_br", "neg_x_03", "neg_x_17",
                    "neg_y_03", "neg_y_17", "neg_xy", "neg_yx", "past_right", "past_bottom", "on_integer", "on_half"):
            ids = _tag(case, tag)
            assert sorted(set(case["radii"][ids].tolist())) == list(sc.EDGE_RADII)
            assert sum(ref["rows"][g] > 0 for g in ids if g not in wide_ids) >= 2, (tag, "the anisotropic shape contributes too")
            for g in ids:
                r = int(case["radii"][g])
                assert ref["rows"][g] > 0 or g not in wide_ids, (tag, g)
                x0, y0 = int(case["m2"][g, 0]) - r + 1, int(case["m2"][g, 1]) - r + 1
                assert x0 < 0 or y0 < 0 or x0 + 2 * r > W or y0 + 2 * r > H or tag.startswith("on_"), "the box crosses an edge"
                if g in wide_ids:   # the wide shape reaches every box pixel inside the image (depth permitting)
                    cols = sc.contributing_columns(case, g)
                    assert cols.size == min(x0 + 2 * r, W) - max(x0, 0), (tag, g)
        for tag in ("outside_left", "outside_below", "outside_corner"):
            for g in _tag(case, tag):
                assert ref["rows"][g] == 0 and not ref["scale"][g].any()
        # truncation toward zero: the last box column of a centre at -0.3 / -1.7 is r / r - 1 (floor: one less)
        for tag, last in (("neg_x_03", 0), ("neg_x_17", -1)):
            for g in _tag(case, tag):
                r = int(case["radii"][g])
                if g in wide_ids and last + r < W:
                    cols = sc.contributing_columns(case, g)
                    x0 = int(case["m2"][g, 0]) - r + 1
                    assert x0 == last - r + 1 and cols.max() + x0 == last + r, (tag, g)
        for tag in ("on_integer", "on_half"):
            f = case["m2"][_tag(case, tag), :] % 1.0
            assert (f == (0.0 if tag == "on_integer" else 0.5)).all()
    assert all(2 * r > 33 for r in sc.EDGE_RADII if r >= 17)


def test_span_gaussians_have_exactly_their_number_of_contributing_rows():
    (case,) = sc.family("spans")
    ref = case["ref"]
    for k in sc.SPANS:
        ids = _tag(case, "span%d" % k)
        assert sorted(set(case["radii"][ids].tolist())) == [40, 70]
        assert (ref["rows"][ids] == k).all(), (k, ref["rows"][ids].tolist())
        if k:
            assert {int(ref["row_lo"][g]) for g in ids} == {0, case["H"] - k}, "top and bottom edge"
            assert all(sc.contributing_columns(case, g).size >= 8 for g in ids)
    assert any(k % 4 == 1 and k > 5 for k in sc.SPANS)


def test_mixed_tasks_pair_disjoint_rows_different_radii_and_empty_spans():
    (case,) = sc.family("mixed")
    ref, radii = case["ref"], case["radii"]
    for k in range(4):
        L = case["lists"][k].tolist()
        assert len(L) == 8 and len(L) % sc.PER_TASK[k] in (0, len(L)), "whole tasks, pairs never split"
        top, bottom, r_lo, r_hi, empty, mid, empty2, mid2 = L
        assert top in case["tags"]["mixed_top"] and bottom in case["tags"]["mixed_bottom"]
        assert ref["rows"][top] > 0 and ref["rows"][bottom] > 0 and ref["row_hi"][top] < ref["row_lo"][bottom]
        assert ref["row_lo"][top] == 0 and ref["row_hi"][bottom] == case["H"] - 1
        assert radii[r_lo] < radii[r_hi] and sc.bwd_class(radii[r_lo]) == sc.bwd_class(radii[r_hi]) == k
        assert ref["rows"][r_lo] > 0 and ref["rows"][r_hi] > 0 and ref["rows"][mid] > 0 and ref["rows"][mid2] > 0
        assert ref["rows"][empty] == 0 and ref["rows"][empty2] == 0 and case["opac"][empty2] == 0


def test_list_shapes_hold_every_count_and_the_unlisted_rows_would_not_be_zero():
    cases = sc.family("lists")
    assert len(cases) == 9 and [L.size for L in cases[7]["lists"]] == list(sc.SKEWED_COUNTS)
    tasks = [-(-n // p) for n, p in zip(sc.SKEWED_COUNTS, sc.PER_TASK)]
    assert min(tasks) == 1 and max(tasks) > 16, "XCDs 1-7 are past the end of one list and inside another"
    for kind, case in enumerate(cases[:7]):
        assert [L.size for L in case["lists"]] == [(0, 1, p - 1, p, p + 1, 8 * p + 1, 8 * 3 * p - 1)[kind] for p in sc.PER_TASK]
    big = cases[8]
    assert [L.size for L in big["lists"]] == [0, 0, 0, 0, 1545] and (big["W"], big["H"]) == (640, 480)
    assert 1545 > 1536 and (1545 + 7) // 8 > 1536 // 8, "a workgroup of the launch takes a second task"
    r = big["radii"][big["lists"][4]]
    assert r.min() == 33 and r.max() == 40
    for case in cases:
        assert case["radii"][0] == 0 and 0 not in np.concatenate(case["lists"]).tolist()
        for g in _tag(case, "unlisted"):
            assert case["ref"]["scale"][g].all() and g not in np.concatenate(case["lists"]).tolist()


def test_values_hold_both_opacity_guards_and_one_clamped_pixel():
    (case,) = sc.family("values")
    ref = case["ref"]
    for g in _tag(case, "opac0"):
        assert case["opac"][g] == 0 and not ref["scale"][g].any()
    for g in _tag(case, "opac_below_cut"):
        assert 0 < case["opac"][g] < 1 / 255 and not ref["scale"][g].any()
    for g in _tag(case, "opac_half"):
        assert case["opac"][g] == 0.5 and ref["scale"][g].all()
    for g in _tag(case, "opac1"):
        x, y = case["m2"][g]
        assert case["opac"][g] == 1.0 and sc.clamped_pixels(case, g) == [(int(y), int(x))]
        assert ref["scale"][g].all() and ref["rows"][g] >= 3
        ca = float(case["conics"][g, 0])
        assert np.exp(-0.5 * ca) <= 0.97, "the neighbours are clearly below the clamp"
    # the depth test varies inside a box: a Gaussian behind the near cut contributes on the far cells only
    near = case["ref_depth"] < 10
    assert 0.3 < near.mean() < 0.7 and (near[:, :-1] != near[:, 1:]).any() and (near[:-1] != near[1:]).any()
    for fam in sc.FAMILIES:
        for c in sc.family(fam):
            d = c["colors"][1:, 3]
            assert (np.abs(d - np.float32(sc.NEAR + sc.DELTA)) >= 1e-3).all()
            if c["radii"].size > 20 and fam not in ("spans", "mixed"):   # (those two: all in front, so that a row count is a row count)
                assert (d < sc.NEAR).any() and (d > sc.NEAR + sc.DELTA).any(), c["name"]
            det = c["conics"][:, 0].astype(np.float64) * c["conics"][:, 2] - c["conics"][:, 1].astype(np.float64) ** 2
            assert (det > 0).all()
