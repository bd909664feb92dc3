"""preprocess_fwd_kernel<DEG> / preprocess_bwd_kernel<DEG> (gps_slam_amd/csrc/splat_fused.hip) per SH degree, K and colour clamp.

The kernels have one instance per degree 0..4; the run-time K (coefficients per Gaussian) sets the sh_rest row stride (K - 1) * 3
and, in the fused backward + Adam, the workgroup size.  The SH schedule runs degrees 0, 1, 2 on K = 16 models, MODEL.sh_degree below
3 gives K = 1, 4, 9 models.  Every (degree, K) pair of tests/degree_cases.py is held to the CPU oracle here, on a scene whose SH
coefficients put a quarter of the rows of every colour channel on the clamped arm of clamp_min(sh + 0.5, 0)
(tests/test_degree_cases_cpu.py vets the reference itself):

  a  the forward per pair: bit-equal projection, the state against the oracle chain, exact zeros on the clamped arm
  b  the forward across K and with the bands above the degree poisoned: same bits
  c  the backward per pair: every compared row within its condition budget, exact zeros above the degree and on the clamped arm
  d  backward + Adam in the kernel against backward, then gps_adam_step: same bits; and a degree rising on one Adam state
  e  models of sh_degree 0, 1, 2: the train step's buffers against the oracle, the three Adam modes, no prefetch
  f  the degree changes under an armed prefetch: the forward run ahead with the old degree is discarded
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import degree_cases as dc
from tests.test_train_step_full_gpu import N_, T, _check_preprocess_state_against_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(96, 64, d, k) for d, k in dc.PAIRS] + [(50, 37, d, k) for d, k in dc.SMALL_PAIRS]
PREFIXES = (4000, 257, 256, 255, 1)   # the forward's 256-row workgroup (and the plain backward's): one more, one less, one row
# the fused backward + Adam works on 128 rows per workgroup at K <= 16 and 64 at K = 25: a row on both sides of every tile boundary
ADAM_PREFIXES = (1, 63, 64, 65, 127, 128, 129, 257, 1000)
GRADS = ("means", "scales", "quats", "featuresDc", "featuresRest", "opacities")   # the oracle's order
OPS_TO_ORACLE = (0, 1, 2, 4, 5, 3)   # ops order: v_means, v_log_scales, v_quats, v_opac_logit, v_sh_dc, v_sh_rest


def _cam(wide):
    return T(wide.vm), T(wide.K), T(wide.cam_pos)


def _fwd(Pt, deg, cam, W, H, **kw):
    from gps_slam_amd import gsplat_ops as ops
    return ops.gauss_preprocess_fwd(Pt[0], Pt[1], Pt[2], Pt[5].view(-1), Pt[3], Pt[4], deg, *cam, W, H, **kw)


def _bwd(Pt, deg, cam, W, H, radii, conics, V):
    from gps_slam_amd import gsplat_ops as ops
    return ops.gauss_preprocess_bwd(Pt[0], Pt[1], Pt[2], Pt[5].view(-1), Pt[3], Pt[4], deg, *cam, W, H, 0.3, radii, conics, *V)


def _cotangents(case, n):
    return tuple(T(np.ascontiguousarray(v[:n])) for v in (case.v_m2, case.v_con, case.v_col, case.v_op))


# ----------------------------------------------------------------------------- a. forward per pair
@pytest.mark.parametrize("W,H,deg,K", CASES)
def test_preprocess_fwd_per_degree_and_k(W, H, deg, K):
    from gps_slam_amd import gsplat_ops as ops
    pair = dc.degree_pair(W, H, deg, K)
    case, wide = pair.case, pair.case.wide
    cam = _cam(wide)
    for n in PREFIXES:
        P = dc.params(case, K, n)
        Pt = [T(a) for a in P]
        pr, pm, pd, pc = ops.fully_fused_projection_fwd(Pt[0], Pt[2], torch.exp(Pt[1]), cam[0][None], cam[1][None], W, H)
        for max_radii in (100, 0):
            out = _fwd(Pt, deg, cam, W, H, max_gs_radii=max_radii)
            radii, m2, depths, conics, colors, opac = out
            want_r = pr[0].clamp_max(max_radii) if max_radii > 0 else pr[0]
            assert torch.equal(radii, want_r), (n, max_radii, int((radii != want_r).sum()))
            assert torch.equal(m2, pm[0]) and torch.equal(depths, pd[0]) and torch.equal(conics, pc[0]), (n, max_radii)
            got = [N_(t) for t in out]
            r0, both = _check_preprocess_state_against_oracle(P, wide, W, H, deg, got, max_radii=max_radii)
            r1, col1 = got[0], got[4]
            assert not col1[r1 <= 0, :3].any(), (n, max_radii)
            for c in range(3):
                lo, hi = both & (pair.raw[:n, c] < -dc.EDGE), both & (pair.raw[:n, c] > dc.EDGE)
                assert (col1[lo, c] == 0.0).all() and (col1[hi, c] > 0).all(), (n, max_radii, c)
                if n == case.N:
                    assert lo.sum() >= 400 and hi.sum() >= 1000
            rec = torch.empty((n, 12), dtype=torch.float32, device=DEV)
            out_r = _fwd(Pt, deg, cam, W, H, max_gs_radii=max_radii, records=rec)
            for a, b in zip(out, out_r):
                assert torch.equal(a, b), (n, max_radii)
            if n == case.N:
                assert both.sum() > 0.5 * n


# ----------------------------------------------------------------------------- b. forward across K, poisoned bands
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_preprocess_fwd_k_and_the_bands_above_the_degree_change_nothing(deg):
    """one degree at every K it runs with: only addresses differ; coefficients above the degree are never read (1e30 there)"""
    W, H = 96, 64
    case = dc.degree_case(W, H)
    cam = _cam(case.wide)
    for n in (4000, 257, 1):
        first = None
        for K in dc.ks_of_degree(deg):
            P = dc.params(case, K, n)
            out = [t.clone() for t in _fwd([T(a) for a in P], deg, cam, W, H)]
            first = first or out
            for a, b in zip(first, out):
                assert torch.equal(a, b), (n, K)
            if K > dc.num_bases(deg):
                Pp = P[:4] + (dc.poisoned(P[4], deg),) + P[5:]
                for a, b in zip(first, _fwd([T(a) for a in Pp], deg, cam, W, H)):
                    assert torch.equal(a, b), (n, K, "poisoned")
        assert torch.isfinite(first[4]).all()


# ----------------------------------------------------------------------------- c. backward per pair
@pytest.mark.parametrize("W,H,deg,K", CASES)
def test_preprocess_bwd_per_degree_and_k(W, H, deg, K):
    """on the oracle's own forward state (r0, c0), so that every row's arm and visibility are the oracle's"""
    pair = dc.degree_pair(W, H, deg, K)
    case, wide, NB = pair.case, pair.case.wide, pair.NB
    cam = _cam(wide)
    for n in PREFIXES:
        P = dc.params(case, K, n)
        Pt = [T(a) for a in P]
        out = _bwd(Pt, deg, cam, W, H, T(wide.r0[:n]), T(wide.c0[:n]), _cotangents(case, n))
        g_hip = [N_(out[k]) for k in OPS_TO_ORACLE]
        vis, cmp_ = pair.vis[:n], pair.cmp[:n]
        for name, got_g, ref_g, bud in zip(GRADS, g_hip, pair.e, pair.budget):
            got_g = got_g.reshape(n, -1)
            assert name == "opacities" or not got_g[~vis].any(), (n, name)
            if got_g.shape[1] == 0:
                continue
            err = np.abs(got_g.astype(np.float64) - ref_g[:n].reshape(n, -1)).max(1)
            ratio = err / (bud[:n] + 1e-300)
            if n == case.N:
                print("degrees %dx%d deg %d K %d preprocess bwd %s: max error / budget %.3f" % (W, H, deg, K, name, ratio[cmp_].max()))
            assert (err[cmp_] <= bud[:n][cmp_]).all(), (n, name, int((err[cmp_] > bud[:n][cmp_]).sum()), float(ratio[cmp_].max()))
        v_dc, v_rest = g_hip[3], g_hip[4]
        assert v_rest.shape == (n, K - 1, 3) and not v_rest[:, NB - 1:].any(), n
        for c in range(3):
            lo, hi = vis & (pair.raw[:n, c] < -dc.EDGE), vis & (pair.raw[:n, c] > dc.EDGE)
            assert not v_dc[lo, c].any() and not v_rest[lo][:, :, c].any(), (n, c)
            np.testing.assert_allclose(v_dc[hi, c], dc.Y0 * case.v_col[:n][hi, c], rtol=1e-6)
        if n == case.N and NB > 1:
            assert v_rest[vis, :NB - 1].any()


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_preprocess_bwd_k_and_the_bands_above_the_degree_change_nothing(deg):
    """the gradients of the bands a degree uses are the same bits at every K it runs with and with 1e30 above the degree; at
    degree 0 that includes v_means, which carries no SH term there"""
    W, H = 96, 64
    case = dc.degree_case(W, H)
    wide, NB = case.wide, dc.num_bases(deg)
    cam = _cam(wide)
    for n in (4000, 257, 1):
        V = _cotangents(case, n)
        r0, c0 = T(wide.r0[:n]), T(wide.c0[:n])
        first = None
        for K in dc.ks_of_degree(deg):
            P = dc.params(case, K, n)
            runs = [("plain", P)]
            if K > NB:
                runs.append(("poisoned", P[:4] + (dc.poisoned(P[4], deg),) + P[5:]))
            for what, Pk in runs:
                out = [t.clone() for t in _bwd([T(a) for a in Pk], deg, cam, W, H, r0, c0, V)]
                assert torch.isfinite(out[5]).all() and not out[5][:, NB - 1:].any(), (n, K, what)
                out[5] = out[5][:, :NB - 1]
                first = first or out
                for k, (a, b) in enumerate(zip(first, out)):
                    assert torch.equal(a, b), (n, K, what, k)
        assert first[0].any() and first[4].any()


# ----------------------------------------------------------------------------- d. backward + Adam in the kernel
def _g(case, K, n):
    g = case.wide.g
    return dict(means=g["means"][:n].copy(), log_scales=g["log_scales"][:n].copy(), quats=g["quats"][:n].copy(),
                opac_logit=g["opac_logit"][:n].copy(), sh=np.ascontiguousarray(case.sh[:n, :K]))


@pytest.mark.parametrize("deg,K", [p for p in dc.PAIRS if p[1] > 1])
def test_fused_adam_is_bit_identical_per_degree_and_k(deg, K):
    from tests.test_splat_gpu import _fused_adam_against_separate_step
    W, H = 96, 64
    case = dc.degree_case(W, H)
    wide = case.wide
    for n in ADAM_PREFIXES:
        _fused_adam_against_separate_step(n, W, H, _g(case, K, n), wide.vm, wide.K, wide.cam_pos, deg=deg, Ksh=K)


@pytest.mark.parametrize("n", [1000, 129])
def test_fused_adam_under_a_rising_degree(n):
    """what the SH schedule runs on a K = 16 model: degrees 0, 1, 1, 2, 3 over steps 1..5 of ONE Adam state.  A band above the
    degree in use keeps its bits and has both moments exactly 0; at the first step of its degree it moves -- from step 2 on the
    kernel reads those zero moments from memory (AdamScalars::fresh supplies them at step 1 only)."""
    from tests.test_splat_gpu import _fused_adam_against_separate_step
    W, H, K = 96, 64, 16
    case = dc.degree_case(W, H)
    wide = case.wide
    degs = [0, 1, 1, 2, 3]
    seen = []

    def after_step(fuse_small, step, deg, P0, A, mA, vA):
        top = dc.num_bases(max(degs[:step])) - 1        # sh_rest bands in use so far
        assert torch.equal(A["rest"][:, top:], P0["rest"][:, top:]), (fuse_small, step)
        assert not mA["rest"][:, top:].any() and not vA["rest"][:, top:].any(), (fuse_small, step)
        if step == 1 or deg > degs[step - 2]:           # the first step of this degree: its own band moves
            band = slice(dc.num_bases(deg - 1) - 1 if deg else 0, dc.num_bases(deg) - 1)
            if deg:
                assert (A["rest"][:, band] != P0["rest"][:, band]).any() and mA["rest"][:, band].any(), (fuse_small, step)
        seen.append((fuse_small, step, deg))

    _fused_adam_against_separate_step(n, W, H, _g(case, K, n), wide.vm, wide.K, wide.cam_pos, deg=degs, Ksh=K, after_step=after_step)
    assert seen == [(f, s, d) for f in (False, True) for s, d in enumerate(degs, 1)]


# ----------------------------------------------------------------------------- e. models of sh_degree 0, 1, 2
def _images(W, H, seed=7):
    gen = torch.Generator().manual_seed(seed)
    gt, base = torch.rand((H, W, 3), generator=gen).to(DEV), torch.rand((H, W, 3), generator=gen).to(DEV)
    ref = (torch.rand((H, W, 1), generator=gen) * 3.5 + 0.5).to(DEV)
    ref[torch.rand((H, W, 1), generator=gen).to(DEV) < 0.1] = 0.0
    return gt, base, ref


def _model(P, cfg):
    from gps_slam_amd.gs_model import SLAMGaussianModel
    m = SLAMGaussianModel(dict(dict(strip_backward=True, capacity=1 << 13), **cfg), device=DEV)
    m.add_params(dict(means=T(P[0]), scales=T(P[1]), quats=T(P[2]), featuresDc=T(P[3]), featuresRest=T(P[4]), opacities=T(P[5])))
    m.initOptimizers(-1, 3.3)
    return m


def _state(m, N):
    """the six parameters and the twelve moments"""
    return [t.clone() for t in m.opt_gs_params.tensors()] + [t[:N].clone() for t in m._opt["m"] + m._opt["v"]]


@pytest.mark.parametrize("d", [0, 1, 2])
def test_model_of_a_low_sh_degree_trains(d):
    from gps_slam_amd._lib import lib
    from gps_slam_amd.gs_model import Camera
    W, H = 96, 64
    K = dc.num_bases(d)
    case = dc.degree_case(W, H)
    wide, N, Km = case.wide, case.N, case.wide.K
    P = dc.params(case, K)
    gt, base, ref = _images(W, H)
    cam = Camera(0, W, H, float(Km[0, 0]), float(Km[1, 1]), float(Km[0, 2]), float(Km[1, 2]), wide.c2w, image=gt, device=DEV)
    ends = []
    for mode in (0, 1, 2):
        m = _model(P, dict(sh_degree=d, fuse_sh_rest_adam=mode))
        assert m.opt_gs_params.featuresRest.shape == (N, K - 1, 3) and m.degreesToUse == d
        m.train_step(cam, ref, base, gt)
        torch.cuda.synchronize()
        B = m._B
        assert int(B["counts"][2]) == 0, "binning capacity overflow"
        r1, m1, c1, col1, op1 = (N_(B[k][:N]) for k in ("radii", "means2d", "conics", "colors", "opacities"))
        _, both = _check_preprocess_state_against_oracle(P, wide, W, H, d, (r1, m1, col1[:, 3], c1, col1, op1))
        assert both.sum() > 0.5 * N
        for _ in range(2):
            m.train_step(cam, ref, base, gt)
        torch.cuda.synchronize()
        assert int(m._step.K) == K and int(m._step.sh_degree) == d and int(B["counts"][2]) == 0
        end = _state(m, N)
        assert all(torch.isfinite(t).all() for t in end)
        for k, (t, p0) in enumerate(zip(end[:6], P)):
            assert t.numel() == 0 or (t != T(p0)).any(), k
        ends.append(end)
    for other in ends[1:]:
        for k, (a, b) in enumerate(zip(ends[0], other)):
            assert torch.equal(a, b), (d, k)
    # next_cam on a model that cannot prefetch is ignored
    a = _model(P, dict(sh_degree=d, fuse_sh_rest_adam=2))
    for _ in range(3):
        a.train_step(cam, ref, base, gt, next_cam=cam)
        assert lib.gps_splat_can_prefetch(C.byref(a._step)) == 0 and a._prefetched is None and int(a._step.preprocessed) == 0
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(_state(a, N), ends[2])):
        assert torch.equal(x, y), (d, k)


# ----------------------------------------------------------------------------- f. the degree changes under an armed prefetch
def test_degree_change_discards_the_forward_run_ahead():
    """sh_degree_interval 2 on a K = 16 model, every Adam step in the kernel, the next camera's forward run in the kernel's tail:
    that forward used the degree of the step it ran in, so at iterations 2, 4 and 6 (the degree has just grown) it is discarded
    and the step preprocesses itself; the twin that never runs ahead ends every iteration with the same bits."""
    from gps_slam_amd._lib import lib
    from tests import scenes
    from tests.test_model_gpu import _two_cameras
    N, W, H = 4000, 160, 120
    g = scenes.random_gaussians(N, seed=21, scale_range=(0.004, 0.03))
    sh = dc.degree_case(96, 64).sh[:, :16]      # (rows of the clamp-populating draw; the geometry here is the default camera's)
    P = (g["means"], g["log_scales"], g["quats"], sh[:, 0].copy(), sh[:, 1:].copy(), g["opac_logit"])
    a, b = (_model(P, dict(sh_degree=3, sh_degree_interval=2, fuse_sh_rest_adam=2)) for _ in range(2))
    cams = _two_cameras(W, H, seed=4)
    gen = torch.Generator().manual_seed(9)
    gts = [torch.rand((H, W, 3), generator=gen).to(DEV) for _ in range(2)]
    base = torch.rand((H, W, 3), generator=gen).to(DEV)
    ref = (torch.rand((H, W, 1), generator=gen) * 4).to(DEV)
    iters = 8
    for it in range(iters):
        k, nxt = it % 2, cams[(it + 1) % 2] if it + 1 < iters else None
        for m in (a, b):
            m.updateSH(it)
            assert m.degreesToUse == min(3, it // 2)
        a.train_step(cams[k], ref, base, gts[k], next_cam=nxt)
        if nxt is not None:
            assert a._prefetched is not None and lib.gps_splat_can_prefetch(C.byref(a._step)) == 1
        b.train_step(cams[k], ref, base, gts[k])
        torch.cuda.synchronize()
        assert int(a._step.preprocessed) == (0 if it in (0, 2, 4, 6) else 1), it
        assert int(b._step.preprocessed) == 0 and int(a._step.sh_degree) == min(3, it // 2)
        for j, (x, y) in enumerate(zip(_state(a, N), _state(b, N))):
            assert torch.equal(x, y), (it, j)
    assert int(a._B["counts"][2]) == 0 and int(b._B["counts"][2]) == 0
    rest = a.opt_gs_params.featuresRest
    assert torch.isfinite(rest).all() and (rest[:, 8:] != T(P[4])[:, 8:]).any()   # the degree-3 band moved in the last two steps
