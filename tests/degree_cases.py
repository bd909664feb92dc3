"""The fused preprocess per SH degree, K and colour clamp: the wide-camera scene (tests/wide_cases.py) with SH coefficients that
reach BOTH arms of clamp_min(sh + 0.5, 0) in every colour channel, and what the CPU oracle and a float64 formulation make of it at
every (degree, K) pair the product runs -- computed once per size and pair, shared by tests/test_degree_cases_cpu.py (the reference
alone meets its conditions) and tests/test_preprocess_degrees_gpu.py (the kernels against it).  Nothing here touches a GPU; callers
must not modify what they get.

The oracle chain (oracle_preprocess / oracle_preprocess_bwd) lives here in its one copy; the chain tests import it."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import splat_ref as orc
from tests import scenes
from tests import wide_cases as wc

Y0 = 0.28209479177387814
K_MAX = 25
SEED_SH, SEED_COT = 29, 2
# (degree, K): K = (degree + 1)^2 models of MODEL.sh_degree 0..2, the SH schedule's degrees 0..2 on a K = 16 model, and degree 0 / 3
# on the 72-float row of K = 25 (its own workgroup size in the fused backward + Adam)
PAIRS = [(0, 1), (1, 4), (2, 9), (0, 16), (1, 16), (2, 16), (0, 25), (3, 25)]
SMALL_PAIRS = [(1, 4), (2, 16)]     # the pairs also run at 50x37
EDGE = 1e-3   # |sh + 0.5| <= EDGE: the row is left out (about 100x the rounding of a sum of <= 25 terms of size <= 1: whether the
              # float32 sum lands on the side of 0 the exact sum is on cannot be told there) -- an exclusion band, not a tolerance


def num_bases(deg):
    return (deg + 1) ** 2


def ks_of_degree(deg):
    """every K the degree appears with in PAIRS"""
    return [k for d, k in PAIRS if d == deg]


# ----------------------------------------------------------------------------- the oracle chain
def oracle_preprocess(P, vm, K, cam_pos, W, H, max_radii=100, deg=3):
    """RawGaussianModel::gesForward up to the binning (raw_gs_model.cpp:207-286) with the oracle operators."""
    means, ls, quats, dc, rest, ol = P
    scales = np.exp(ls)
    radii, m2, depths, conics = orc.proj_fwd(means, quats, scales, vm, K, W, H)
    radii = np.minimum(radii, max_radii)
    dirs = means - cam_pos[None]
    sh = np.concatenate([dc[:, None], rest], 1)
    rgb = np.maximum(orc.sh_fwd(deg, dirs, sh, radii > 0) + np.float32(0.5), np.float32(0.0))
    colors = np.concatenate([rgb, depths[:, None]], 1).astype(np.float32)
    opac = (np.float32(1.0) / (np.float32(1.0) + np.exp(-ol[:, 0]))).astype(np.float32)
    return radii, m2, depths, conics, colors, opac, scales, dirs, sh


def oracle_preprocess_bwd(P, vm, K, cam_pos, W, H, radii, conics, v_m2, v_con, v_col, v_op, deg=3):
    """adjoint of the chain above: clamp_min mask -> SH bwd (v_dirs -> v_means) -> projection bwd -> exp / sigmoid."""
    means, ls, quats, dc, rest, ol = P
    scales = np.exp(ls)
    dirs = means - cam_pos[None]
    sh = np.concatenate([dc[:, None], rest], 1)
    vis = radii > 0
    raw = orc.sh_fwd(deg, dirs, sh, vis) + np.float32(0.5)
    v_rgb = np.where(raw >= 0, v_col[:, :3], 0).astype(np.float32)
    v_sh, v_dirs = orc.sh_bwd(deg, dirs, sh, vis, v_rgb)
    v_means, v_quats, v_scales = orc.proj_bwd(means, quats, scales, vm, K, W, H, radii, conics, v_m2,
                                              np.ascontiguousarray(v_col[:, 3]), v_con)
    v_means = v_means + v_dirs
    o = 1.0 / (1.0 + np.exp(-ol[:, 0].astype(np.float64)))
    v_ol = (v_op.astype(np.float64) * o * (1 - o)).astype(np.float32)[:, None]
    return v_means, (v_scales * scales).astype(np.float32), v_quats, v_sh[:, 0], v_sh[:, 1:], v_ol


# ----------------------------------------------------------------------------- the scene
@functools.lru_cache(maxsize=None)
def degree_case(W, H):
    """wide_case(W, H) -- geometry, camera, the oracle's forward state r0 / c0, the clamp classes, a visible row 0 -- with ONE draw
    of SH coefficients at K = 25 in place of the scene's: DC colour in [-0.45, 1.25] and a rest of sigma 0.15, so that sh + 0.5 is
    negative for roughly a quarter of the rows in every channel at every degree.  Tests slice [:, :K]: every K shares its leading
    coefficients.  The cotangents are drawn as test_wide_camera_gauss_preprocess_bwd draws them."""
    wide = wc.wide_case(W, H)
    N = wide.N
    rng = np.random.default_rng(SEED_SH)
    sh = np.zeros((N, K_MAX, 3), np.float32)
    sh[:, 0] = (rng.uniform(-0.45, 1.25, (N, 3)) - 0.5) / Y0
    sh[:, 1:] = rng.normal(0, 0.15, (N, K_MAX - 1, 3))
    rng = np.random.default_rng(SEED_COT)
    v_m2 = rng.normal(size=(N, 2)).astype(np.float32)
    v_con = (rng.normal(size=(N, 3)) * 0.1).astype(np.float32)
    v_col = rng.normal(size=(N, 4)).astype(np.float32)
    v_op = rng.normal(size=N).astype(np.float32)
    assert wide.r0[0] > 0, "row 0 is visible: the prefix of one Gaussian runs the whole chain"
    return SimpleNamespace(wide=wide, N=N, W=W, H=H, sh=sh, vis=wide.r0 > 0, v_m2=v_m2, v_con=v_con, v_col=v_col, v_op=v_op,
                           dirs=(wide.g["means"] - wide.cam_pos[None]).astype(np.float32))


def params(case, K, n=None):
    """(means, log_scales, quats, sh_dc, sh_rest [n, K - 1, 3], opac_logit) of the first n rows, as fresh arrays"""
    g, n = case.wide.g, case.N if n is None else n
    return (g["means"][:n].copy(), g["log_scales"][:n].copy(), g["quats"][:n].copy(), case.sh[:n, 0].copy(), case.sh[:n, 1:K].copy(),
            g["opac_logit"][:n].copy())


def poisoned(rest, deg, value=1e30):
    """sh_rest with every band above the degree set to `value` (NaN would do for a forward, but Adam would carry it)"""
    out = rest.copy()
    out[:, num_bases(deg) - 1:] = value
    return out


# ----------------------------------------------------------------------------- float64 formulation of the colour chain (degree <= 2)
def sh_basis64(deg, d):
    """the real spherical harmonics up to degree 2 on unit vectors d [N, 3] in closed form (the sign convention of the splatting
    papers: Y_1 = c1 (-y, z, -x)) -> [N, (deg + 1)^2]"""
    assert 0 <= deg <= 2
    x, y, z = d.unbind(1)
    pi = math.pi
    Y = [torch.full_like(x, 0.5 * math.sqrt(1.0 / pi))]
    if deg >= 1:
        c1 = math.sqrt(3.0 / (4.0 * pi))
        Y += [-c1 * y, c1 * z, -c1 * x]
    if deg >= 2:
        c2 = 0.5 * math.sqrt(15.0 / pi)
        Y += [c2 * x * y, -c2 * y * z, 0.25 * math.sqrt(5.0 / pi) * (3.0 * z * z - 1.0), -c2 * x * z, 0.5 * c2 * (x * x - y * y)]
    return torch.stack(Y, 1)


def colour_chain64(case, deg, coeffs=None):
    """clamp_min(SH_deg(normalize(means - cam_pos)) @ coeffs[:, :NB] + 0.5, 0) in float64 on the case's float32 inputs
    -> (means leaf, coeffs leaf [N, NB, 3], raw [N, 3], colours [N, 3])"""
    NB = num_bases(deg)
    means = torch.tensor(case.wide.g["means"], dtype=torch.float64, requires_grad=True)
    cf = torch.tensor(case.sh[:, :NB] if coeffs is None else coeffs[:, :NB], dtype=torch.float64, requires_grad=True)
    dirs = means - torch.tensor(case.wide.cam_pos, dtype=torch.float64)
    Y = sh_basis64(deg, dirs / dirs.norm(dim=1, keepdim=True))
    raw = torch.einsum("nk,nkc->nc", Y, cf) + 0.5
    return means, cf, raw, torch.clamp_min(raw, 0.0)


# ----------------------------------------------------------------------------- one (degree, K) pair
def _colour_adjoint(deg, dirs, sh, vis, v_rgb_in):
    """the oracle's colour adjoint alone: mask of clamp_min -> SH bwd -> (v_sh [N, K, 3], v_dirs [N, 3])"""
    raw = orc.sh_fwd(deg, dirs, sh, vis) + np.float32(0.5)
    return orc.sh_bwd(deg, dirs, sh, vis, np.where(raw >= 0, v_rgb_in, 0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def degree_pair(W, H, deg, K):
    """The oracle chain and its adjoint on the oracle's own forward state (r0, c0) for one (degree, K):
      raw [N, 3]        the oracle's sh + 0.5 (0.5 on invisible rows)
      col [N, 4]        the oracle's colours | depth
      near_clamp [N]    any channel with |raw| <= EDGE
      cmp [N]           visible & ~on_limit & ~near_clamp: the rows whose gradients are compared
      e                 the six gradients (means, scales, quats, featuresDc, featuresRest, opacities)
      v_sh, v_dirs      the colour adjoint's own outputs ([N, K, 3], [N, 3])
      budget            per-row condition budgets of the six gradients (scenes.condition_budget, trials = 2, default factor and
                        floor; + 4 * 2^-23 * |v_op * o| on the opacities), on all N rows: rows are independent, a prefix test
                        takes slices
      sh_budget         (degree <= 2) the same for (v_sh, v_dirs) of the colour adjoint alone, for the float64 comparison"""
    case = degree_case(W, H)
    wide = case.wide
    assert K >= num_bases(deg) and K <= K_MAX
    P = params(case, K)
    vm, Km, cam_pos = wide.vm, wide.K, wide.cam_pos
    sh = np.ascontiguousarray(case.sh[:, :K])
    vis = case.vis
    raw = orc.sh_fwd(deg, case.dirs, sh, vis) + np.float32(0.5)
    col = oracle_preprocess(P, vm, Km, cam_pos, W, H, deg=deg)[4]
    near = (np.abs(raw) <= EDGE).any(1)
    cmp_ = vis & ~wide.cls["on_limit"] & ~near
    V = (case.v_m2, case.v_con, case.v_col, case.v_op)
    e = oracle_preprocess_bwd(P, vm, Km, cam_pos, W, H, wide.r0, wide.c0, *V, deg=deg)
    fn = lambda pm, pls, pq, pdc, prest, pol, cc, a, b, c, d: oracle_preprocess_bwd(
        (pm, pls, pq, pdc, prest, pol), vm, Km, cam_pos, W, H, wide.r0, cc, a, b, c, d, deg=deg)
    if K > 1:
        budget = scenes.condition_budget(fn, P + (wide.c0,) + V, e, trials=2)
    else:   # featuresRest is [N, 0, 3]: nothing to take a row maximum of, nothing to compare
        keep = (0, 1, 2, 3, 5)
        budget = scenes.condition_budget(lambda *a: [fn(*a)[k] for k in keep], P + (wide.c0,) + V, [e[k] for k in keep], trials=2)
        budget.insert(4, np.zeros(case.N))
    o64 = 1.0 / (1.0 + np.exp(-P[5][:, 0].astype(np.float64)))
    budget[5] = budget[5] + 4 * 2.0 ** -23 * np.abs(case.v_op.astype(np.float64) * o64)
    v_rgb = np.ascontiguousarray(case.v_col[:, :3])
    v_sh, v_dirs = _colour_adjoint(deg, case.dirs, sh, vis, v_rgb)
    sh_budget = None
    if deg <= 2:
        sh_budget = scenes.condition_budget(lambda dd, cc, vv: _colour_adjoint(deg, dd, cc, vis, vv), (case.dirs, sh, v_rgb),
                                            (v_sh, v_dirs), trials=2)
    return SimpleNamespace(case=case, deg=deg, K=K, NB=num_bases(deg), raw=raw, col=col, near_clamp=near, cmp=cmp_, vis=vis, e=e,
                           v_sh=v_sh, v_dirs=v_dirs, budget=budget, sh_budget=sh_budget)
