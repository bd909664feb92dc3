"""Cases and oracle of the densification kernels (gps_densify_accumulate / _plan / _apply, include/gps_slam_hip.h).

A case is a model of N Gaussians at SH width K with Adam moments, densification statistics, the four thresholds of
gps_densify_plan and a pool of normal samples.  Rows are built class by class, so that every class of densifiyGs occurs where a
case asks for it:

    plain       low gradient, small, opaque                      kept
    clone       high gradient, small                             kept + cloned
    split       high gradient, large                             two children, parent pruned
    low         opacity below prune_opac                         pruned
    clone_low   clone whose parent is below prune_opac           parent and clone pruned
    split_low   split parent below prune_opac                    parent and both children pruned
    huge        low gradient, largest scale above prune_scale    pruned while the scale criterion is on, kept otherwise
    split_huge  split parent above prune_scale whose children (scale / 1.6) are below it: the children survive
    split_giant split parent so large that the children are above prune_scale too: pruned while the criterion is on
    vis0        vis_count 0 with a gradient sum above the threshold: high through max(vis_count, 1)
    vis0_zero   vis_count 0, gradient sum 0: not high

The oracle is a float64 restatement, written twice and independently: `oracle_index` evaluates the index formulas of the header
per row; `oracle_cat` runs the reference's op order in CPU torch (cat the three groups, build the prune mask over the
concatenated VALUES, index).  tests/test_densify_abi_cpu.py requires that both agree on every case.

No decision quantity of a case lies within a relative 1e-4 of its threshold (`check_margins`, float64 on the float32 inputs):
three orders of magnitude above the error of float32 exp / log, so the device decides every row as float64 does.  A draw that
fails the check is drawn again with the next seed.
"""
import numpy as np

SIZE_FAC = float(np.float32(1.6))      # sizeFac of densifiyGs, the float the reference divides by
GRAD_THRES = float(np.float32(0.0002))
SPLIT_SCALE = float(np.float32(0.01))  # densify_large_thres * scene_scale
PRUNE_OPAC = float(np.float32(0.005))
PRUNE_SCALE = float(np.float32(0.1))   # 0.1 * scene_scale while curr_iter > reset_opacity_interval, +inf before
MARGIN = 1e-4
BLOCK = 256                            # GPS_DENSIFY_PLAN_BLOCK
CLASSES = ("plain", "clone", "split", "low", "clone_low", "split_low", "huge", "split_huge", "split_giant", "vis0", "vis0_zero")
ROWS = lambda K: (3, 3, 4, 3, 3 * (K - 1), 1)   # means, log_scales, quats, featuresDc, featuresRest, opacities


class Case:
    def __init__(self, name, K, labels, scale_prune, seed):
        self.name, self.K, self.labels, self.scale_prune, self.seed = name, K, list(labels), scale_prune, seed
        self.N = len(self.labels)
        self.grad_thres, self.split_scale, self.prune_opac = GRAD_THRES, SPLIT_SCALE, PRUNE_OPAC
        self.prune_scale = PRUNE_SCALE if scale_prune else float("inf")

    def __repr__(self):
        return "Case(%s, N=%d, K=%d)" % (self.name, self.N, self.K)


def _draw(case, seed):
    rng = np.random.default_rng(seed)
    N, K = case.N, case.K
    f32 = np.float32
    high = np.zeros(N, bool); smax = np.zeros(N); opac = np.zeros(N); vis = np.zeros(N); gsum = np.zeros(N)
    for i, lab in enumerate(case.labels):
        hi = lab in ("clone", "split", "clone_low", "split_low", "split_huge", "split_giant", "vis0")
        high[i] = hi
        if lab in ("split", "split_low"):
            smax[i] = rng.uniform(0.015, 0.05)
        elif lab in ("huge", "split_huge"):
            smax[i] = rng.uniform(0.11, 0.15)       # / 1.6 -> 0.069 .. 0.094: below prune_scale
        elif lab == "split_giant":
            smax[i] = rng.uniform(0.18, 0.3)        # / 1.6 -> 0.11 .. 0.19: above it
        else:
            smax[i] = rng.uniform(0.001, 0.007)
        opac[i] = rng.uniform(0.001, 0.004) if lab in ("low", "clone_low", "split_low") else rng.uniform(0.05, 0.95)
        vis[i] = 0 if lab in ("vis0", "vis0_zero") else rng.integers(1, 20)
        avg = GRAD_THRES * (rng.uniform(1.5, 4.0) if hi else rng.uniform(0.1, 0.7))
        gsum[i] = 0.0 if lab == "vis0_zero" else avg * max(vis[i], 1)
    scales = smax[:, None] * rng.uniform(0.2, 1.0, (N, 3))
    scales[np.arange(N), rng.integers(0, 3, N)] = smax
    case.log_scales = np.log(scales).astype(f32)
    case.opac = np.log(opac / (1 - opac)).astype(f32)[:, None]
    case.grad_sum, case.vis_count = gsum.astype(f32), vis.astype(f32)
    case.means = rng.uniform(-2, 2, (N, 3)).astype(f32)
    case.quats = (rng.normal(size=(N, 4)) * rng.uniform(0.3, 3.0, (N, 1))).astype(f32)   # un-normalised, as the optimiser leaves them
    case.dc = rng.normal(size=(N, 3)).astype(f32)
    case.rest = rng.normal(size=(N, K - 1, 3)).astype(f32)
    case.params = [case.means, case.log_scales, case.quats, case.dc, case.rest, case.opac]
    # moments: distinct values everywhere, so that a shifted row or column shows
    case.m, case.v = [], []
    base = 1.0
    for p in case.params:
        n = p.size
        case.m.append((base + np.arange(n, dtype=np.float64)).astype(f32).reshape(p.shape)); base += n
        case.v.append((base + np.arange(n, dtype=np.float64)).astype(f32).reshape(p.shape)); base += n
    assert base < 2 ** 24   # exact in float32
    case.sample_pool = rng.normal(size=(2 * max(N, 1), 3)).astype(f32)


def check_margins(case):
    """every decision quantity at least a relative MARGIN away from its threshold, in float64"""
    def clear(x, thres):
        return np.all(np.abs(x - thres) > MARGIN * abs(thres)) if np.isfinite(thres) else True
    avg = case.grad_sum.astype(np.float64) / np.maximum(case.vis_count.astype(np.float64), 1.0)
    smax = np.exp(case.log_scales.astype(np.float64)).max(1) if case.N else np.zeros(0)
    child = np.exp(np.log(np.exp(case.log_scales.astype(np.float64)) / SIZE_FAC)).max(1) if case.N else np.zeros(0)
    sig = 1.0 / (1.0 + np.exp(-case.opac.astype(np.float64)[:, 0]))
    return (clear(avg, case.grad_thres) and clear(smax, case.split_scale) and clear(smax, case.prune_scale) and
            clear(child, case.prune_scale) and clear(sig, case.prune_opac))


def make_case(name, K, labels, scale_prune=True, seed=0):
    case = Case(name, K, labels, scale_prune, seed)
    for attempt in range(100):   # regenerated, never skipped
        _draw(case, 1000 * seed + attempt)
        if check_margins(case):
            return case
    raise AssertionError("no draw of %r clears the margins" % case)


def case_from_arrays(name, params, m, v, grad_sum, vis_count, grad_thres, split_scale, prune_opac, prune_scale, samples):
    """a snapshot of a live model as a case (float32 arrays; samples: the [2 n_split, 3] draws the densification used, or None)"""
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    K = params[4].shape[1] + 1
    case = Case(name, K, ["?"] * params[0].shape[0], np.isfinite(prune_scale), 0)
    case.params = [f32(p) for p in params]
    case.means, case.log_scales, case.quats, case.dc, case.rest, case.opac = case.params
    case.m, case.v = [f32(t) for t in m], [f32(t) for t in v]
    case.grad_sum, case.vis_count = f32(grad_sum), f32(vis_count)
    case.grad_thres, case.split_scale, case.prune_opac, case.prune_scale = (float(np.float32(x)) for x in (grad_thres, split_scale, prune_opac, prune_scale))
    case.sample_pool = f32(samples) if samples is not None else np.zeros((0, 3), np.float32)
    return case


def margin_report(case):
    """the smallest relative distance of each decision quantity from its threshold (what check_margins tests)"""
    def dist(x, thres):
        return float(np.min(np.abs(x - thres)) / abs(thres)) if np.isfinite(thres) and x.size else float("inf")
    avg = case.grad_sum.astype(np.float64) / np.maximum(case.vis_count.astype(np.float64), 1.0)
    smax = np.exp(case.log_scales.astype(np.float64)).max(1)
    child = np.exp(np.log(np.exp(case.log_scales.astype(np.float64)) / SIZE_FAC)).max(1)
    sig = 1.0 / (1.0 + np.exp(-case.opac.astype(np.float64)[:, 0]))
    return dict(grad=dist(avg, case.grad_thres), split_scale=dist(smax, case.split_scale), prune_scale=dist(smax, case.prune_scale),
                child_prune_scale=dist(child, case.prune_scale), opacity=dist(sig, case.prune_opac))


def _mixed(n, seed, classes=CLASSES):
    rng = np.random.default_rng(seed)
    labels = [classes[k % len(classes)] for k in range(n)]   # every class present when n allows it
    rng.shuffle(labels)
    return labels


def all_cases():
    """the cases of the issue, each at SH degree 0 (K 1) and 3 (K 16)"""
    out = []
    for K in (1, 16):
        t = "k%d_" % K
        for lab in ("plain", "clone", "split", "low"):
            out.append(make_case(t + "one_" + lab, K, [lab], seed=len(out)))
        for missing in ("plain", "clone", "split", "low"):
            kinds = [c for c in ("plain", "clone", "split", "low") if c != missing]
            out.append(make_case(t + "no_" + missing, K, _mixed(37, len(out), kinds), seed=len(out)))
        out.append(make_case(t + "all_split", K, ["split"] * 41, seed=len(out)))
        out.append(make_case(t + "all_pruned", K, _mixed(45, len(out), ("low", "clone_low", "split_low")), seed=len(out)))
        for n in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1):
            out.append(make_case(t + "n%d" % n, K, _mixed(n, len(out)), seed=len(out)))
        out.append(make_case(t + "split_low", K, _mixed(19, len(out), ("plain", "split_low", "split", "clone")), seed=len(out)))
        out.append(make_case(t + "clone_low", K, _mixed(19, len(out), ("plain", "clone_low", "clone", "split")), seed=len(out)))
        labels = _mixed(67, len(out))
        out.append(make_case(t + "scale_prune_off", K, labels, scale_prune=False, seed=len(out)))
        out.append(make_case(t + "scale_prune_on", K, labels, scale_prune=True, seed=len(out)))
        out.append(make_case(t + "vis0", K, _mixed(23, len(out), ("vis0", "vis0_zero", "plain", "split")), seed=len(out)))
    return out


class Expected:
    """layout (exact): counts, src[M], kind[M] (0 kept, 1 child, 2 clone), sample[M] (row of the samples, -1 unless a child);
    values (float64): the six parameter tensors of the new model"""

    def __init__(self, counts, src, kind, sample, params):
        self.counts, self.src, self.kind, self.sample, self.params = counts, src, kind, sample, params
        self.M = int(counts[0])


def _rot(q):
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def oracle_index(case, samples=None):
    """the index formulas of the header, row by row"""
    N = case.N
    P = [p.astype(np.float64) for p in case.params]
    ls, op = P[1], P[5][:, 0]
    avg = case.grad_sum.astype(np.float64) / np.maximum(case.vis_count.astype(np.float64), 1.0)
    high = avg > case.grad_thres
    smax = np.exp(ls).max(1) if N else np.zeros(0)
    large = smax > case.split_scale
    split, dup = high & large, high & ~large
    low = 1.0 / (1.0 + np.exp(-op)) < case.prune_opac
    pruned = low | (smax > case.prune_scale)
    child_ls = np.log(np.exp(ls) / SIZE_FAC)
    child_pruned = low | ((np.exp(child_ls).max(1) if N else np.zeros(0)) > case.prune_scale)
    keep = ~split & ~pruned
    ss, ds = split & ~child_pruned, dup & ~pruned
    n_keep, n_split, n_ss, n_ds = int(keep.sum()), int(split.sum()), int(ss.sum()), int(ds.sum())
    M = n_keep + 2 * n_ss + n_ds
    r_all = np.cumsum(split) - split
    r_surv = np.cumsum(ss) - ss
    r_keep = np.cumsum(keep) - keep
    r_dup = np.cumsum(ds) - ds
    src = np.full(M, -1, np.int64); kind = np.full(M, -1, np.int64); sample = np.full(M, -1, np.int64)
    for i in range(N):
        if keep[i]:
            src[r_keep[i]], kind[r_keep[i]] = i, 0
        if ss[i]:
            for s in (0, 1):
                d = n_keep + s * n_ss + r_surv[i]
                src[d], kind[d], sample[d] = i, 1, s * n_split + r_all[i]
        if ds[i]:
            d = n_keep + 2 * n_ss + r_dup[i]
            src[d], kind[d] = i, 2
    assert (src >= 0).all()
    if samples is None:
        samples = case.sample_pool[:2 * n_split]
    z = samples.astype(np.float64)
    out = [p[src] for p in P]
    c = kind == 1
    if c.any():
        pc = src[c]
        out[0][c] = np.einsum("nij,nj->ni", _rot(P[2][pc]), np.exp(ls[pc]) * z[sample[c]]) + P[0][pc]
        out[1][c] = child_ls[pc]
    return Expected(np.array([M, n_split, n_ss, n_ds, n_keep]), src, kind, sample, out)


def oracle_cat(case, samples=None):
    """the reference's op order in CPU torch (float64): cat {originals, split children, clones}, the prune mask over the
    concatenated values, index with its complement"""
    import torch
    N = case.N
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    means, scales, quats, dc, rest, opacities = [T(p) for p in case.params]
    grads = T(case.grad_sum) / torch.clamp_min(T(case.vis_count), 1)
    is_grad_high = grads > case.grad_thres
    max_scales = torch.exp(scales).max(1)[0] if N else torch.zeros(0).double()
    is_scale_large = max_scales > case.split_scale
    is_dupli, is_split = is_grad_high & ~is_scale_large, is_grad_high & is_scale_large
    n_splits = int(is_split.sum())
    z = T(case.sample_pool[:2 * n_splits] if samples is None else samples).reshape(2 * n_splits, 3)
    scaled = torch.exp(scales[is_split].repeat(2, 1)) * z
    qs = quats[is_split] / torch.linalg.vector_norm(quats[is_split], 2, -1, True)
    rots = torch.from_numpy(_rot(qs.repeat(2, 1).numpy())) if n_splits else torch.zeros(0, 3, 3).double()
    split_means = torch.bmm(rots, scaled[..., None])[..., 0] + means[is_split].repeat(2, 1)
    split_scales = torch.log(torch.exp(scales[is_split]) / SIZE_FAC).repeat(2, 1)
    ids = torch.arange(N)
    cat = lambda a, b, c: torch.cat([a, b, c], 0)
    all_means = cat(means, split_means, means[is_dupli])
    all_scales = cat(scales, split_scales, scales[is_dupli])
    all_quats = cat(quats, quats[is_split].repeat(2, 1), quats[is_dupli])
    all_dc = cat(dc, dc[is_split].repeat(2, 1), dc[is_dupli])
    all_rest = cat(rest, rest[is_split].repeat(2, 1, 1), rest[is_dupli])
    all_opac = cat(opacities, opacities[is_split].repeat(2, 1), opacities[is_dupli])
    n_dup = int(is_dupli.sum())
    all_src = cat(ids, ids[is_split].repeat(2), ids[is_dupli])
    all_kind = cat(torch.zeros(N), torch.ones(2 * n_splits), torch.full((n_dup,), 2.0)).long()
    all_sample = cat(torch.full((N,), -1), torch.arange(2 * n_splits), torch.full((n_dup,), -1)).long()
    splits_mask = cat(is_split, torch.zeros(2 * n_splits, dtype=torch.bool), torch.zeros(n_dup, dtype=torch.bool))
    is_prune = (torch.sigmoid(all_opac) < case.prune_opac).squeeze(-1) | splits_mask
    if np.isfinite(case.prune_scale):
        is_prune = is_prune | (torch.exp(all_scales).max(-1)[0] > case.prune_scale)
    keep = ~is_prune
    kind = all_kind[keep].numpy()
    n_keep, n_child, n_ds = int((kind == 0).sum()), int((kind == 1).sum()), int((kind == 2).sum())
    assert n_child % 2 == 0   # both samples of a parent share the decision: same opacity, same scales
    counts = np.array([int(keep.sum()), n_splits, n_child // 2, n_ds, n_keep])
    params = [t[keep].numpy() for t in (all_means, all_scales, all_quats, all_dc, all_rest, all_opac)]
    return Expected(counts, all_src[keep].numpy(), kind, all_sample[keep].numpy(), params)


def expected_moments(case, exp):
    """moments of the new model: the survivors' own, zero for new rows"""
    out = []
    for mom in (case.m, case.v):
        rows = []
        for t in mom:
            r = t[exp.src].copy()
            r[exp.kind != 0] = 0
            rows.append(r)
        out.append(rows)
    return out


def child_bounds(case, exp, samples=None):
    """per child row: the bound on its log-scales, 4 * 2^-24 * max(1, |s|) per element, and on its mean,
    64 * 2^-24 * (|exp(s) * z|_2 + |mean_p|_inf)"""
    c = exp.kind == 1
    pc = exp.src[c]
    if samples is None:
        samples = case.sample_pool[:2 * int(exp.counts[1])]
    ls = case.log_scales.astype(np.float64)[pc]
    z = samples.astype(np.float64)[exp.sample[c]]
    scale_bound = 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(ls))
    mean_bound = 64 * 2.0 ** -24 * (np.linalg.norm(np.exp(ls) * z, axis=1) + np.abs(case.means.astype(np.float64)[pc]).max(1))
    return scale_bound, mean_bound[:, None]
