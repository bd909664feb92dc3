"""Densification on the device: gps_densify_accumulate / _plan / _apply through ctypes and RawGaussianModel::densifiyGs /
resetOpacities through the C++ host, against the float64 oracle of tests/densify_cases.py.

The layout (counts, source row, kind and sample row of every new row) is compared exactly; copied values bit for bit; computed
values against float64 within bounds that follow from the operation count:
    accumulated norm   2^-22 relative (two rounded products, their squares' sum, a square root: 3 half-ulps on the result)
    child log-scale    4 * 2^-24 * max(1, |s|)
    child mean         64 * 2^-24 * (|exp(s) * z|_2 + |mean|_inf)
    moments            new rows exactly zero, survivors bit-equal (the cases fill them with distinct integers)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import densify_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = dc.all_cases()
BY_NAME = {c.name: c for c in CASES}
_EXPECTED = {}
SENTINEL = float(np.float32(-77.25))


def expected(case):
    if case.name not in _EXPECTED:   # computed once, shared, never modified
        _EXPECTED[case.name] = dc.oracle_index(case)
    return _EXPECTED[case.name]


def _lib():
    from gps_slam_amd import _lib
    return _lib.load_library()


def _host():
    _lib()
    import gps_slam_amd._host as h
    return h


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def six(tensors):
    return (C.c_void_p * 6)(*[(t.data_ptr() or None) if t.numel() else None for t in tensors])


def run_abi(case, moments=True):
    """plan, one read of the counts, apply into sentinel-filled buffers of M + 3 rows"""
    lib = _lib()
    st = torch.cuda.current_stream().cuda_stream
    N = case.N
    src = [T(p) for p in case.params]
    sm, sv = [T(p) for p in case.m], [T(p) for p in case.v]
    gs, vc = T(case.grad_sum), T(case.vis_count)
    dst_src = torch.full((2 * N + 2,), -5, dtype=torch.int32, device=DEV)
    dst_sample = torch.full((2 * N + 2,), -5, dtype=torch.int32, device=DEV)
    counts = torch.full((5,), -1, dtype=torch.int32, device=DEV)
    host_counts = torch.full((16,), -1, dtype=torch.int32).pin_memory()
    ws = torch.empty(int(lib.gps_densify_plan_workspace_bytes(N)), dtype=torch.uint8, device=DEV)
    rc = lib.gps_densify_plan(N, gs.data_ptr(), vc.data_ptr(), src[1].data_ptr(), src[5].data_ptr(), case.grad_thres, case.split_scale,
                              case.prune_opac, case.prune_scale, dst_src.data_ptr(), dst_sample.data_ptr(), 2 * N, counts.data_ptr(),
                              host_counts.data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert rc == 0
    torch.cuda.synchronize()
    hc = host_counts[:5].tolist()
    assert counts.cpu().tolist() == hc
    M, n_split, n_ss, n_ds, n_keep = hc
    assert dst_src[2 * N:].tolist() == [-5, -5] and dst_sample[2 * N:].tolist() == [-5, -5]
    samples = T(case.sample_pool[:2 * n_split])
    rows = M + 3
    mk = lambda like: [torch.full((rows,) + tuple(t.shape[1:]), SENTINEL, device=DEV) for t in like]
    dst, dm, dv = mk(src), mk(src), mk(src)
    args = [six(src), six(dst)] + ([six(sm), six(dm), six(sv), six(dv)] if moments else [None] * 4)
    rc = lib.gps_densify_apply(N, case.K, M, n_split, n_ss, n_ds, n_keep, dst_src.data_ptr(), dst_sample.data_ptr(),
                               samples.data_ptr() if n_split else None, *args, st)
    assert rc == 0
    torch.cuda.synchronize()
    n = lambda ts: [t.cpu().numpy() for t in ts]
    # out of place: the sources are what they were
    for a, b in zip(n(src) + n(sm) + n(sv), case.params + case.m + case.v):
        assert np.array_equal(bits(a), bits(b))
    return dict(counts=hc, dst_src=dst_src.cpu().numpy(), dst_sample=dst_sample.cpu().numpy(), params=n(dst), m=n(dm), v=n(dv))


def check_model(case, exp, params, m=None, v=None, what=""):
    """params / m / v: six arrays of exactly M rows each"""
    M = exp.M
    copied_rows = exp.kind != 1
    child = ~copied_rows
    scale_bound, mean_bound = dc.child_bounds(case, exp)
    for k in range(6):
        got = np.asarray(params[k])
        assert got.shape == (M,) + case.params[k].shape[1:], (what, k, got.shape)
        want = exp.params[k]
        rows = copied_rows if k < 2 else np.ones(M, bool)
        assert np.array_equal(bits(got[rows]), bits(want[rows].astype(np.float32))), (what, case, "parameter", k)   # bit copies of float32 rows
        if k == 0 and child.any():
            err = np.abs(got[child].astype(np.float64) - want[child])
            assert np.all(err <= mean_bound), (what, case, "child mean", float((err / mean_bound).max()))
        if k == 1 and child.any():
            err = np.abs(got[child].astype(np.float64) - want[child])
            assert np.all(err <= scale_bound), (what, case, "child log-scale", float((err / scale_bound).max()))
    if m is not None:
        em, ev = dc.expected_moments(case, exp)
        for k in range(6):
            assert np.array_equal(bits(m[k]), bits(em[k])), (what, case, "exp_avg", k)
            assert np.array_equal(bits(v[k]), bits(ev[k])), (what, case, "exp_avg_sq", k)
            assert not np.asarray(m[k])[exp.kind != 0].any() and not np.asarray(v[k])[exp.kind != 0].any()


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_plan_and_apply_against_the_oracle(name):
    case, exp = BY_NAME[name], expected(BY_NAME[name])
    out = run_abi(case)
    M = exp.M
    assert out["counts"] == exp.counts.tolist(), (out["counts"], exp.counts.tolist())
    assert np.array_equal(out["dst_src"][:M], exp.src)
    c = exp.kind == 1
    assert np.array_equal(out["dst_sample"][:M][c], exp.sample[c])
    check_model(case, exp, [p[:M] for p in out["params"]], [p[:M] for p in out["m"]], [p[:M] for p in out["v"]], "C ABI")
    for group in (out["params"], out["m"], out["v"]):       # nothing written behind row M
        for t in group:
            assert np.all(t[M:] == np.float32(SENTINEL))


def test_apply_without_moments_writes_the_parameters_only():
    case = BY_NAME["k16_n257"]
    exp = expected(case)
    out = run_abi(case, moments=False)
    check_model(case, exp, [p[:exp.M] for p in out["params"]], what="no optimiser")
    for t in out["m"] + out["v"]:
        assert np.all(t == np.float32(SENTINEL))


def test_accumulate_norm_count_and_untouched_rows():
    lib = _lib()
    st = torch.cuda.current_stream().cuda_stream
    W, H = 64, 48
    for N in (1, 255, 256, 257, 513):
        rng = np.random.default_rng(N)
        g = (rng.choice([-1.0, 1.0], (N, 2)) * 10.0 ** rng.uniform(-6, -2, (N, 2))).astype(np.float32)
        g[rng.random(N) < 0.1, 0] = 0.0
        radii = rng.integers(-2, 40, N).astype(np.int32)
        radii[rng.random(N) < 0.3] = 0
        radii[0] = 3
        vis = radii > 0
        norm = np.sqrt((g[:, 0].astype(np.float64) * W / 2) ** 2 + (g[:, 1].astype(np.float64) * H / 2) ** 2)
        # from zero: the norm itself, the count exactly 1
        gs, vc = torch.zeros(N + 1, device=DEV), torch.zeros(N + 1, device=DEV)
        gs[N], vc[N] = 5.0, 6.0
        assert lib.gps_densify_accumulate(N, T(g).data_ptr(), T(radii).data_ptr(), W, H, gs.data_ptr(), vc.data_ptr(), st) == 0
        torch.cuda.synchronize()
        a, c = gs.cpu().numpy().astype(np.float64), vc.cpu().numpy()
        assert a[N] == 5.0 and c[N] == 6.0                                  # the row behind the last one
        assert np.all(np.abs(a[:N][vis] - norm[vis]) <= 2.0 ** -22 * norm[vis]), float((np.abs(a[:N][vis] - norm[vis]) / norm[vis]).max())
        assert np.array_equal(c[:N], vis.astype(np.float32)) and not a[:N][~vis].any()
        # onto earlier statistics: one more rounding, that of the sum; rows with radii <= 0 bit-unchanged
        prev_g = (rng.uniform(0, 0.05, N)).astype(np.float32)
        prev_c = rng.integers(0, 500, N).astype(np.float32)
        gs, vc = T(prev_g), T(prev_c)
        dg, dr = T(g), T(radii)
        assert lib.gps_densify_accumulate(N, dg.data_ptr(), dr.data_ptr(), W, H, gs.data_ptr(), vc.data_ptr(), st) == 0
        torch.cuda.synchronize()
        a, c = gs.cpu().numpy(), vc.cpu().numpy()
        assert np.array_equal(bits(a[~vis]), bits(prev_g[~vis])) and np.array_equal(c[~vis], prev_c[~vis])
        want = prev_g[vis].astype(np.float64) + norm[vis]
        assert np.all(np.abs(a[vis].astype(np.float64) - want) <= 2.0 ** -22 * norm[vis] + 2.0 ** -24 * want)
        assert np.array_equal(c[vis], prev_c[vis] + 1)


# ------------------------------------------------------------------ RawGaussianModel
RESET_INTERVAL = 100


def make_model(case, capacity, optimiser=True):
    h = _host()
    m = h.SLAMGaussianModel()
    deg = {1: 0, 16: 3}[case.K]
    m.loadConfig(dict(capacity=capacity, sh_degree=deg, render_method="raw"))
    m.getGaussianParms().add([T(p) for p in case.params])
    m.densify_grad_thres, m.densify_large_thres, m.prune_opacity_thres = case.grad_thres, case.split_scale, case.prune_opac
    m.reset_opacity_interval, m.pause_refine_after_reset = RESET_INTERVAL, 0
    if optimiser:
        m.initOptimizers(-1, 1.0)
        st = m.adamState()
        for k in range(6):
            st[k].copy_(T(case.m[k])); st[6 + k].copy_(T(case.v[k]))
    gs, vc = m.densifyStats()
    gs.copy_(T(case.grad_sum)); vc.copy_(T(case.vis_count))
    return m


def model_arrays(m):
    torch.cuda.synchronize()
    p = m.getGaussianParms()
    params = [t.cpu().numpy() for t in (p.getMeans(), p.getScales(), p.getQuats(), p.getFeaturesDc(), p.getFeaturesRest(), p.getOpacities())]
    st = [t.cpu().numpy() for t in m.adamState()]
    return params, st[:6], st[6:]


def densify(m, case, exp):
    """curr_iter on the side of reset_opacity_interval that the case's scale criterion asks for"""
    curr_iter = RESET_INTERVAL + 50 if case.scale_prune else RESET_INTERVAL - 50
    n_split = int(exp.counts[1])
    return m.densifiyGs(1.0, curr_iter, T(case.sample_pool[:2 * n_split]) if n_split else None)


@pytest.mark.parametrize("name", ["k1_n513", "k16_n513", "k16_scale_prune_off", "k16_scale_prune_on", "k1_one_plain", "k16_all_split"])
def test_model_densify_against_the_oracle(name):
    case, exp = BY_NAME[name], expected(BY_NAME[name])
    m = make_model(case, 2048)
    step, events = m.adamStep(), m.densify_events
    got = densify(m, case, exp)
    assert got == exp.counts.tolist() and m.getGaussianNum() == exp.M and m.capacity() == 2048 and m.adamStep() == step
    changed = exp.M != case.N or int(exp.counts[4]) != case.N
    assert m.densify_events == events + (1 if changed else 0)
    check_model(case, exp, *model_arrays(m), what="model")
    gs, vc = m.densifyStats()
    if changed:
        assert gs.shape[0] == exp.M and not gs.any() and not vc.any()       # the statistics belonged to the old rows


def test_model_without_optimiser_and_generator_draws():
    """no initOptimizers: parameters only.  Without samples from the caller they come from the seeded host generator: the draws
    of torch.randn on a CPU generator of that seed, [2 n_split, 3]"""
    case = BY_NAME["k16_n257"]
    exp0 = expected(case)
    n_split = int(exp0.counts[1])
    m = make_model(case, 1024, optimiser=False)
    m.setDensifySeed(77)
    curr_iter = RESET_INTERVAL + 50
    assert m.densifiyGs(1.0, curr_iter) == exp0.counts.tolist()
    z = torch.randn((2 * n_split, 3), generator=torch.Generator().manual_seed(77))
    assert torch.equal(m.lastSplitSamples().cpu(), z)
    exp = dc.oracle_index(case, z.numpy())
    assert m.adamState() == []
    p = m.getGaussianParms()
    torch.cuda.synchronize()
    params = [t.cpu().numpy() for t in (p.getMeans(), p.getScales(), p.getQuats(), p.getFeaturesDc(), p.getFeaturesRest(), p.getOpacities())]
    M = exp.M
    c = exp.kind == 1
    ls = case.log_scales.astype(np.float64)[exp.src[c]]
    zz = z.numpy().astype(np.float64)[exp.sample[c]]
    bound = 64 * 2.0 ** -24 * (np.linalg.norm(np.exp(ls) * zz, axis=1) + np.abs(case.means.astype(np.float64)[exp.src[c]]).max(1))
    assert params[0].shape[0] == M
    assert np.all(np.abs(params[0][c].astype(np.float64) - exp.params[0][c]) <= bound[:, None])
    assert np.array_equal(bits(params[0][~c]), bits(exp.params[0][~c].astype(np.float32)))
    for k in (2, 3, 4, 5):
        assert np.array_equal(bits(params[k]), bits(exp.params[k].astype(np.float32)))
    # wrong number of samples from the caller: refused, the model as it was
    m2 = make_model(case, 1024)
    with pytest.raises(RuntimeError, match="split_samples"):
        m2.densifiyGs(1.0, curr_iter, torch.zeros((2 * n_split + 1, 3), device=DEV))
    assert m2.getGaussianNum() == case.N


def test_one_snapshot_one_seed_one_result():
    """plan and apply use no atomics and the samples come from a host generator: the same model, statistics and seed give the same
    bits, twice"""
    case = BY_NAME["k16_n513"]
    outs = []
    for _ in range(2):
        m = make_model(case, 2048)
        m.setDensifySeed(5)
        m.densifiyGs(1.0, RESET_INTERVAL + 50)
        params, mm, vv = model_arrays(m)
        outs.append(params + mm + vv)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(*outs)) and outs[0][0].shape[0] == expected(case).M


@pytest.mark.parametrize("K", [1, 16])
def test_every_row_pruned_leaves_an_empty_usable_model(K):
    case = BY_NAME["k%d_all_pruned" % K]
    exp = expected(case)
    assert exp.M == 0
    m = make_model(case, 256)
    assert densify(m, case, exp) == exp.counts.tolist() and m.getGaussianNum() == 0
    p = m.getGaussianParms()
    assert p.getMeans().shape == (0, 3) and p.getFeaturesRest().shape == (0, K - 1, 3)
    assert m.densifiyGs(1.0, RESET_INTERVAL + 50) == []                         # an empty model: nothing to plan
    # usable: new Gaussians go in and densify as any others
    again = BY_NAME["k%d_n255" % K]
    p.add([T(t) for t in again.params])
    assert m.getGaussianNum() == 255 and m.capacity() == 256
    m.initOptimizers(-1, 1.0)
    st = m.adamState()
    for k in range(6):
        st[k].copy_(T(again.m[k])); st[6 + k].copy_(T(again.v[k]))
    gs, vc = m.densifyStats()
    gs.copy_(T(again.grad_sum)); vc.copy_(T(again.vis_count))
    e2 = expected(again)
    assert densify(m, again, e2) == e2.counts.tolist() and m.capacity() == 256
    check_model(again, e2, *model_arrays(m), what="after the empty model")


GROW = dc.make_case("grow", 16, ["clone"] * 30 + ["split"] * 10 + ["plain"] * 5 + ["low"] * 3, seed=91)


@pytest.mark.parametrize("slack", [0, -1])
def test_growth_with_live_moments(slack):
    """capacity exactly M: nothing is reallocated.  Capacity M - 1: every capacity-sized buffer grows (the parameters' policy: at
    least double, at least 2^19 rows), contents, moments and the step count survive"""
    case = GROW
    exp = dc.oracle_index(case)
    assert exp.counts.tolist() == [85, 10, 10, 30, 35]
    cap = exp.M + slack
    m = make_model(case, cap)
    assert m.capacity() == cap >= case.N
    step = m.adamStep()
    assert densify(m, case, exp) == exp.counts.tolist()
    assert m.capacity() == (cap if slack == 0 else max(2 * cap, 1 << 19)) and m.adamStep() == step
    check_model(case, exp, *model_arrays(m), what="growth")
    gs, vc = m.densifyStats()
    assert gs.shape[0] == exp.M and not gs.any() and not vc.any()
    # the grown model densifies again (all buffers are of one capacity): nothing is high any more, the low rows are gone
    assert m.densifiyGs(1.0, RESET_INTERVAL + 50) == [exp.M, 0, 0, 0, exp.M]


def test_pause_after_reset_keeps_the_reference_condition():
    case = BY_NAME["k1_n255"]
    m = make_model(case, 1024)
    m.pause_refine_after_reset = 60
    assert m.densifiyGs(1.0, RESET_INTERVAL + 50) == [] and m.getGaussianNum() == case.N     # 150 % 100 = 50 < 60: nothing at all
    m.pause_refine_after_reset = 50
    assert densify(m, case, expected(case)) == expected(case).counts.tolist()


@pytest.mark.parametrize("K", [1, 16])
def test_opacity_reset(K):
    case = BY_NAME["k%d_n257" % K]
    m = make_model(case, 512)
    step = m.adamStep()
    m.resetOpacities()
    params, mm, vv = model_arrays(m)
    top = float(torch.logit(torch.tensor(np.float32(2) * np.float32(case.prune_opac))))   # the float logit of a host tensor, as the reference
    want = np.minimum(case.opac, np.float32(top))
    assert np.array_equal(bits(params[5]), bits(want)) and (case.opac > top).any() and (case.opac < top).any()
    assert abs(1 / (1 + np.exp(-top)) - 2 * case.prune_opac) < 1e-7
    for k in range(5):
        assert np.array_equal(bits(params[k]), bits(case.params[k]))
        assert np.array_equal(bits(mm[k]), bits(case.m[k])) and np.array_equal(bits(vv[k]), bits(case.v[k]))
    assert not mm[5].any() and not vv[5].any() and m.adamStep() == step and m.getGaussianNum() == case.N


def test_model_reads_the_keys_from_a_shipped_file():
    import os
    h = _host()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "tests", "golden", "configs", "release", "replica", "office0.yaml")).read()
    for old, new in (("densify_start_iter: 500", "densify_start_iter: 7"), ("densify_end_iter: 6000", "densify_end_iter: 91"),
                     ("densify_interval: 100", "densify_interval: 13"), ("densify_grad_thres: 0.0002", "densify_grad_thres: 0.25"),
                     ("densify_large_thres: 0.01", "densify_large_thres: 0.5"), ("reset_opacity_interval: 3000", "reset_opacity_interval: 17"),
                     ("prune_opacity_thres: 0.005", "prune_opacity_thres: 0.125"), ("  delta_depth: 0.1\n", "  delta_depth: 0.1\n  capacity: 1024\n")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    m = h.SLAMGaussianModel()
    m.loadConfig(h.parse_yaml(text, "edited.yaml")["MODEL"])
    assert (m.densify_start_iter, m.densify_end_iter, m.densify_interval, m.reset_opacity_interval) == (7, 91, 13, 17)
    assert (m.densify_grad_thres, m.densify_large_thres, m.prune_opacity_thres, m.pause_refine_after_reset) == (0.25, 0.5, 0.125, 0)
