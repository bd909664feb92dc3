"""The degree case set (tests/degree_cases.py), vetted without a GPU: the reference alone meets the conditions the GPU tests of
tests/test_preprocess_degrees_gpu.py lean on.

Per (degree, K) pair: both arms of clamp_min(sh + 0.5, 0) are well populated in every colour channel, few rows fall into the
exclusion band around the clamp, the oracle itself keeps the bands above the degree out of everything (zeros in the gradient,
coefficients it never reads), and -- for degrees up to 2 -- the oracle's colours and colour adjoint agree with a float64
formulation written from the closed-form real spherical harmonics.  This is what keeps the GPU file from passing vacuously.
"""
import numpy as np
import pytest
import torch

from tests import degree_cases as dc
from tests import scenes

CASES = [(96, 64, d, k) for d, k in dc.PAIRS] + [(50, 37, d, k) for d, k in dc.SMALL_PAIRS]


def test_pairs_cover_every_degree_and_every_row_stride():
    """the pairs are the issue's: degrees 0..2 on their own K and on K = 16, degree 0 and 3 on K = 25"""
    assert dc.PAIRS == [(0, 1), (1, 4), (2, 9), (0, 16), (1, 16), (2, 16), (0, 25), (3, 25)]
    assert all(k >= dc.num_bases(d) for d, k in dc.PAIRS)
    assert dc.ks_of_degree(0) == [1, 16, 25] and dc.ks_of_degree(1) == [4, 16] and dc.ks_of_degree(2) == [9, 16]


def test_the_sh_draw_is_the_issues():
    case = dc.degree_case(96, 64)
    assert case.sh.shape == (4000, 25, 3) and case.sh.dtype == np.float32
    colour0 = case.sh[:, 0] * dc.Y0 + 0.5
    assert colour0.min() >= -0.45 - 1e-6 and colour0.max() <= 1.25 + 1e-6 and colour0.min() < -0.4 and colour0.max() > 1.2
    assert abs(case.sh[:, 1:].std() - 0.15) < 0.003
    # the geometry and the forward state are the wide scene's, untouched
    from tests import wide_cases as wc
    assert case.wide is wc.wide_case(96, 64) and case.vis[0]


@pytest.mark.parametrize("W,H,deg,K", CASES)
def test_both_arms_of_the_colour_clamp_are_populated(W, H, deg, K):
    p = dc.degree_pair(W, H, deg, K)
    vis = p.vis
    for c in range(3):
        lo, hi = int((vis & (p.raw[:, c] < -dc.EDGE)).sum()), int((vis & (p.raw[:, c] > dc.EDGE)).sum())
        print("%dx%d deg %d K %d channel %d: %d clamped, %d unclamped of %d visible" % (W, H, deg, K, c, lo, hi, int(vis.sum())))
        assert lo >= 400 and hi >= 1000, (c, lo, hi)
    excluded = int((vis & p.near_clamp).sum())
    print("%dx%d deg %d K %d: %d visible rows within %g of the clamp" % (W, H, deg, K, excluded, dc.EDGE))
    assert excluded <= 0.01 * vis.sum()
    scenes.assert_wide_scene_reaches_every_branch(p.case.wide.cls, p.case.wide.r0, big=(W, H) == (96, 64))
    assert p.cmp.sum() >= 0.98 * vis.sum()
    # the colours are the clamp of raw, and a clamped channel is exactly 0
    assert np.array_equal(p.col[vis, :3], np.maximum(p.raw[vis], np.float32(0)))


@pytest.mark.parametrize("W,H,deg,K", CASES)
def test_oracle_keeps_the_bands_above_the_degree_out(W, H, deg, K):
    from oracle import splat_ref as orc
    p = dc.degree_pair(W, H, deg, K)
    case, NB, vis = p.case, p.NB, p.vis
    assert p.v_sh.shape == (case.N, K, 3)
    assert not p.v_sh[:, NB:].any()
    assert not p.v_sh[~vis].any() and not p.v_dirs[~vis].any()
    for k in (0, 1, 2, 3, 4):   # every gradient but the opacities' is zero on a row the forward culled
        assert not p.e[k][~vis].any(), k
    if deg == 0:
        assert not p.v_dirs.any()
    else:
        assert p.v_dirs[vis].any()
    assert p.v_sh[vis, :NB].any()
    # coefficients above the degree are never read
    sh = np.ascontiguousarray(case.sh[:, :K])
    bad = sh.copy()
    bad[:, NB:] = 1e30
    assert np.array_equal(orc.sh_fwd(deg, case.dirs, sh, vis), orc.sh_fwd(deg, case.dirs, bad, vis))
    # a clamped channel passes nothing on, an unclamped one passes Y0 * v_col to the DC term
    for c in range(3):
        lo, hi = vis & (p.raw[:, c] < -dc.EDGE), vis & (p.raw[:, c] > dc.EDGE)
        assert not p.v_sh[lo][:, :, c].any()
        np.testing.assert_allclose(p.v_sh[hi, 0, c], dc.Y0 * case.v_col[hi, c], rtol=1e-6)


@pytest.mark.parametrize("W,H,deg,K", [c for c in CASES if c[2] <= 2])
def test_oracle_colour_chain_against_float64(W, H, deg, K):
    """the oracle's SH colour and its adjoint against float64 autograd of the closed-form bases: colours at the tolerance the GPU
    tests hold the kernel to, v_sh and v_dirs of every compared row within the colour adjoint's own condition budget"""
    p = dc.degree_pair(W, H, deg, K)
    case, NB, vis = p.case, p.NB, p.vis
    means, cf, raw, col = dc.colour_chain64(case, deg)
    np.testing.assert_allclose(p.col[vis, :3], col.detach().numpy()[vis], rtol=1e-4, atol=2e-5)
    # float64 and the oracle agree on the arm of every row outside the band
    away = vis & ~p.near_clamp
    assert np.array_equal(raw.detach().numpy()[away] >= 0, p.raw[away] >= 0)
    mask = torch.tensor(vis)
    loss = (col * torch.tensor(case.v_col[:, :3], dtype=torch.float64))[mask].sum()
    g_cf, g_means = torch.autograd.grad(loss, (cf, means), allow_unused=True)   # (degree 0: the colour does not depend on the direction)
    ref_sh, ref_dirs = g_cf.numpy(), np.zeros((case.N, 3)) if g_means is None else g_means.numpy()
    assert (g_means is None) == (deg == 0)
    for name, got, ref, bud in (("v_sh", p.v_sh[:, :NB], ref_sh, p.sh_budget[0]), ("v_dirs", p.v_dirs, ref_dirs, p.sh_budget[1])):
        err = np.abs(got.reshape(case.N, -1).astype(np.float64) - ref.reshape(case.N, -1)).max(1)
        ratio = err / (bud + 1e-300)
        print("%dx%d deg %d K %d oracle vs float64 %s: max error / budget %.3f" % (W, H, deg, K, name, ratio[p.cmp].max()))
        assert (err[p.cmp] <= bud[p.cmp]).all(), (name, int((err[p.cmp] > bud[p.cmp]).sum()), float(ratio[p.cmp].max()))
