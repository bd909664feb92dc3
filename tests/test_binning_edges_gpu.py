"""Both tile binnings at their table, band and capacity edges (cases: tests/binning_cases.py, vetted on the CPU by
tests/test_binning_cases_cpu.py).

Everything compared here is an integer and compared with np.array_equal against the C oracle (orc.isect_tiles /
orc.isect_tiles_depth; the model path's class lists against scenes.bwd_class_lists) of the state the kernels themselves
projected: no tolerance anywhere.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from tests import binning_cases as bc
from tests import scenes
from tests.test_splat_gpu import N_, T, _bin_inputs
from tests.test_model_gpu import DEV

pytestmark = pytest.mark.gpu
TS = bc.TS
ICAP = 1 << 22
C_BYTES = bc.SB_MAX_TILES * bc.SB_MAX * 4     # the count table C: first in the workspace


# ------------------------------------------------------------------------------------------------------ sorted-key path
def _oracle(case):
    from oracle import splat_ref as orc
    tw, th = bc.grid(case["W"], case["H"])
    return orc.isect_tiles(case["m2"], case["radii"], TS, tw, th)


def _call(case, **kw):
    from gps_slam_amd import gsplat_ops as ops
    tw, th = bc.grid(case["W"], case["H"])
    N = case["radii"].size
    return ops.isect_tiles_no_depth(T(case["m2"]).reshape(1, N, 2), T(case["radii"]).reshape(1, N), TS, tw, th, **kw)


@pytest.mark.parametrize("name", list(bc.sorted_key_cases()))
def test_sorted_key_binning_is_the_oracles_on_the_case(name):
    case = bc.sorted_key_cases()[name]
    tpg, ids, flat, ggs, gst, offs = _oracle(case)
    for want_ids in (True, False):
        r = _call(case, want_isect_ids=want_ids)
        counts = N_(r.counts)
        assert counts.tolist() == [flat.shape[0], ggs.shape[0], 0, int((case["radii"] > 0).sum())], (want_ids, counts)
        ni, ng = flat.shape[0], ggs.shape[0]
        assert np.array_equal(N_(r.tiles_per_gauss)[0], tpg), want_ids
        if want_ids:
            assert np.array_equal(N_(r.isect_ids)[:ni], ids)
        else:
            assert r.isect_ids is None
        assert np.array_equal(N_(r.flatten_ids)[:ni], flat), want_ids
        assert np.array_equal(N_(r.group_gs_ids)[:ng], ggs) and np.array_equal(N_(r.group_starts)[:ng], gst), want_ids
        assert np.array_equal(N_(r.isect_offsets)[0], offs), want_ids
        bc.check_expect(case, case["radii"], N_(r.tiles_per_gauss)[0], N_(r.flatten_ids)[:ni], N_(r.isect_offsets))


@pytest.mark.parametrize("name", list(bc.depth_key_cases()))
def test_depth_keyed_binning_is_the_oracles_on_the_case(name):
    from gps_slam_amd import gsplat_ops as ops
    from oracle import splat_ref as orc
    case = bc.depth_key_cases()[name]
    tw, th = bc.grid(case["W"], case["H"])
    N = case["radii"].size
    tpg, ids, flat, offs = orc.isect_tiles_depth(case["m2"], case["radii"], case["depths"], TS, tw, th)
    r = ops.isect_tiles(T(case["m2"]).reshape(1, N, 2), T(case["radii"]).reshape(1, N), T(case["depths"]).reshape(1, N), TS, tw, th)
    counts = N_(r.counts)
    ni = flat.shape[0]
    assert int(counts[0]) == ni and int(counts[2]) == 0 and int(counts[3]) == int((case["radii"] > 0).sum()), counts
    assert np.array_equal(N_(r.tiles_per_gauss)[0], tpg)
    assert np.array_equal(N_(r.isect_ids)[:ni], ids)
    assert np.array_equal(N_(r.flatten_ids)[:ni], flat)
    assert np.array_equal(N_(r.isect_offsets)[0], offs)


def test_a_grid_of_more_than_65536_tiles_is_refused():
    from gps_slam_amd import gsplat_ops as ops
    m2, radii = _bin_inputs(100, 257 * 16, 256 * 16, seed=3)
    with pytest.raises(RuntimeError, match="gps_isect_tiles_no_depth"):
        ops.isect_tiles_no_depth(T(m2).reshape(1, -1, 2), T(radii).reshape(1, -1), TS, 257, 256)
    torch.cuda.synchronize()


def _random_640():
    m2, radii = _bin_inputs(5000, 640, 480, seed=5)
    return dict(name="random_640x480", W=640, H=480, m2=m2, radii=radii, expect={})


def _overflow_case(which):
    return bc.sorted_key_cases()["pile_up"] if which == "pile_up" else _random_640()


def _tile_lists(flat, offs, n):
    o = np.concatenate([np.asarray(offs).reshape(-1).astype(np.int64), [n]])
    return [flat[o[t]:o[t + 1]] for t in range(o.shape[0] - 1)]


@pytest.mark.parametrize("which", ["pile_up", "random_640x480"])
def test_sorted_key_overflow_contract(which):
    """isect_capacity == n_isects: exact, no flag.  One less, and half: the flag, counts[0] == capacity, offsets non-decreasing in
    [0, capacity], every tile's list strictly ascending and a subset of the oracle's, no id outside [0, N).  Only the group table
    too small: the flag, the intersection lists exact, counts[1] == capacity.  The flag is sticky across launches into the same
    `out`: overflowing, then not -> still 1, and the second launch's lists exact."""
    case = _overflow_case(which)
    N = case["radii"].size
    tpg, ids, flat, ggs, gst, offs = _oracle(case)
    ni, ng = flat.shape[0], ggs.shape[0]
    want = _tile_lists(flat, offs, ni)

    def exact(r, groups=True):
        assert np.array_equal(N_(r.tiles_per_gauss)[0], tpg) and np.array_equal(N_(r.flatten_ids)[:ni], flat)
        assert np.array_equal(N_(r.isect_offsets)[0], offs)
        if groups:
            assert np.array_equal(N_(r.group_gs_ids)[:ng], ggs) and np.array_equal(N_(r.group_starts)[:ng], gst)

    r = _call(case, isect_capacity=ni, group_capacity=ng)
    assert N_(r.counts).tolist() == [ni, ng, 0, int((case["radii"] > 0).sum())]
    exact(r)
    for cap in (ni - 1, ni // 2):
        r = _call(case, isect_capacity=cap, group_capacity=ng)
        counts = N_(r.counts)
        assert counts.tolist() == [cap, ng, 1, int((case["radii"] > 0).sum())], counts
        o = N_(r.isect_offsets).reshape(-1).astype(np.int64)
        assert (np.diff(o) >= 0).all() and o.min() >= 0 and o.max() <= cap
        got = N_(r.flatten_ids)[:cap]
        assert got.min() >= 0 and got.max() < N
        for t, lst in enumerate(_tile_lists(got, o, cap)):
            assert (np.diff(lst) > 0).all() and np.isin(lst, want[t]).all(), (cap, t)
    r = _call(case, isect_capacity=ni, group_capacity=ng - 1)
    assert N_(r.counts).tolist() == [ni, ng - 1, 1, int((case["radii"] > 0).sum())]
    exact(r, groups=False)
    assert np.array_equal(N_(r.group_gs_ids)[:ng - 1], ggs[:ng - 1]) and np.array_equal(N_(r.group_starts)[:ng - 1], gst[:ng - 1])
    # sticky: into the same `out` (its buffers are sized by the first call, so both launches take 2 N Gaussians) first the scene
    # twice over, which overflows, then the scene followed by N invisible Gaussians, which fits exactly
    from gps_slam_amd import gsplat_ops as ops
    tw, th = bc.grid(case["W"], case["H"])
    m2b = np.concatenate([case["m2"], case["m2"]])
    out = _call(dict(case, m2=m2b, radii=np.concatenate([case["radii"], case["radii"]])), isect_capacity=ni, group_capacity=ng)
    assert N_(out.counts).tolist()[:3] == [ni, ng, 1]
    rb = np.concatenate([case["radii"], np.zeros_like(case["radii"])])
    ops.isect_tiles_no_depth(T(m2b).reshape(1, -1, 2), T(rb).reshape(1, -1), TS, tw, th, isect_capacity=ni, group_capacity=ng, out=out)
    counts = N_(out.counts)
    assert counts.tolist() == [ni, ng, 1, int((case["radii"] > 0).sum())], counts
    assert np.array_equal(N_(out.flatten_ids)[:ni], flat) and np.array_equal(N_(out.isect_offsets)[0], offs)
    assert np.array_equal(N_(out.tiles_per_gauss)[0], np.concatenate([tpg, np.zeros_like(tpg)]))
    assert np.array_equal(N_(out.group_gs_ids)[:ng], ggs) and np.array_equal(N_(out.group_starts)[:ng], gst)


# ----------------------------------------------------------------------------------------------------------- model path
def _rows(s, sl=slice(None)):
    return dict(means=T(s["means"][sl]), scales=T(s["log_scales"][sl]), quats=T(s["quats"][sl]), featuresDc=T(s["sh"][sl, 0].copy()),
                featuresRest=T(s["sh"][sl, 1:].copy()), opacities=T(s["opac_logit"][sl]))


def _maps(W, H, seed=3):
    gen = torch.Generator().manual_seed(seed)
    gt = torch.rand((H, W, 3), generator=gen).to(DEV)
    base = torch.rand((H, W, 3), generator=gen).to(DEV)
    ref = (torch.rand((H, W, 1), generator=gen) * 4).to(DEV)
    ref[ref < 0.4] = 0.0
    return ref, base, gt


def _camera(case, cam_id=0, shift=0.0):
    from gps_slam_amd.gs_model import Camera
    s, W, H = case["scene"], case["W"], case["H"]
    K = s["K"]
    c2w = s["c2w"].copy()
    c2w[0, 3] += shift
    return Camera(cam_id, W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), c2w, device=DEV)


def _model(case, capacity=None, isect_capacity=ICAP):
    from gps_slam_amd.gs_model import SLAMGaussianModel
    cap = capacity or max(1 << 12, 1 << int(case["N"]).bit_length())      # the next power of two above N
    model = SLAMGaussianModel(dict(capacity=cap, isect_capacity=isect_capacity, fuse_sh_rest_adam=2, strip_backward=True), device=DEV)
    model.add_params(_rows(case["scene"]))
    return model


def _state(model):
    torch.cuda.synchronize()
    B, N = model._B, model.getGaussianNum()
    return B, N, N_(B["means2d"][:N]), N_(B["radii"][:N])


def _c_is_zero(model):
    return int(model._B["workspace"][:C_BYTES].view(torch.int64).ne(0).sum()) == 0


def _check_exact(model, W, H, stage, train, superblock=True):
    """the lists in the model's buffers == the oracle's for the radii / means2d the kernels projected -> (radii, tpg, flat, offs)"""
    from oracle import splat_ref as orc
    tw, th = bc.grid(W, H)
    B, N, m2, r = _state(model)
    tpg, ids, flat, ggs, gst, offs = orc.isect_tiles(m2, r, TS, tw, th)
    ni = flat.shape[0]
    counts = N_(B["counts"])
    assert int(counts[0]) == ni and int(counts[2]) == 0 and int(counts[3]) == int((r > 0).sum()), (stage, counts, ni)
    assert np.array_equal(N_(B["flatten_ids"][:ni]), flat), stage
    assert np.array_equal(N_(B["tile_offsets"]), offs.reshape(-1)), stage
    assert np.array_equal(N_(B["tiles_per_gauss"][:N]), tpg), stage
    if superblock:
        assert int(counts[1]) == 0, (stage, counts)
        _check_prefix_table(model, N, tw * th, flat, offs, stage)
        if train:
            _check_class_lists(B, m2, r, tw, th, stage)
    elif train:   # the sorted-key route builds the group table for the group backward
        ng = ggs.shape[0]
        assert int(counts[1]) == ng and ng > 0, (stage, counts)
        assert np.array_equal(N_(B["group_gs_ids"][:ng]), ggs) and np.array_equal(N_(B["group_starts"][:ng]), gst), stage
    assert _c_is_zero(model), stage
    return r, tpg, flat, offs


def _check_prefix_table(model, N, n_tiles, flat, offs, stage):
    """the table P[tile][superblock] (behind C in the workspace) = per tile the exclusive prefix of its pairs over the superblocks
    of sb_shift_for(N) blocks, as binning_cases restates it: pins the superblock size the kernels used"""
    P = N_(model._B["workspace"][C_BYTES:2 * C_BYTES].view(torch.int32)).reshape(bc.SB_MAX_TILES, bc.SB_MAX)[:n_tiles]
    n = flat.shape[0]
    tile = np.repeat(np.arange(n_tiles), np.diff(np.concatenate([offs.reshape(-1).astype(np.int64), [n]])))
    sb = flat.astype(np.int64) >> (8 + bc.sb_shift_for(N))
    cnt = np.bincount(tile * bc.SB_MAX + sb, minlength=n_tiles * bc.SB_MAX).reshape(n_tiles, bc.SB_MAX)
    assert np.array_equal(P, np.cumsum(cnt, 1) - cnt), stage


def _check_class_lists(B, m2, r, tw, th, stage):
    cc = N_(B["cls_counts"])
    for k, want in enumerate(scenes.bwd_class_lists(m2, r, TS, tw, th)):
        assert int(cc[k]) == want.shape[0] and np.array_equal(N_(B["cls_ids"][k, :want.shape[0]]), want), (stage, k)


def _tile_order(model, n_tiles):
    from gps_slam_amd._lib import lib
    B, st = model._B, model._step
    p = lib.gps_isect_workspace_tile_order(C.c_void_p(B["workspace"].data_ptr()), st.N, st.isect_capacity)
    off = p - B["workspace"].data_ptr()
    assert 0 < off < B["workspace"].numel()
    return N_(B["workspace"][off:off + 4 * n_tiles].view(torch.int32))


def _check_tile_order(model, case, offs, n):
    tw, th = bc.grid(case["W"], case["H"])
    order = _tile_order(model, tw * th)
    assert np.array_equal(np.sort(order), np.arange(tw * th))
    length = np.diff(np.concatenate([offs.reshape(-1).astype(np.int64), [n]]))
    cls = np.minimum(63, length[order] >> 5)
    assert (np.diff(cls) <= 0).all(), case["name"]
    if case["name"] == "long_tile":
        assert order[0] == 0 and cls[0] == 63 and cls[1] < 63
    if case["name"] == "uniform_lengths":
        assert (cls == 0).all()


ORDER_CASES = ("uniform_lengths", "long_tile", "grid_4096")
MODEL_NAMES = list(bc.MODEL_BUILDERS)


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_model_path_binning_is_the_oracles_on_the_case(name):
    """render-only forward (no class lists), then one train step: lists, offsets, counts, tiles_per_gauss and (train step) the class
    lists or -- where the superblock path is refused -- the group table are the oracle's; the case's properties hold on the state
    the kernels projected; the count table is zero after every launch."""
    from gps_slam_amd._lib import lib
    case = bc.model_case(name)
    W, H = case["W"], case["H"]
    sb = case["expect"]["superblock_path"]
    model = _model(case)
    cam = _camera(case)
    ref, base, gt = _maps(W, H)
    model.forward(cam, ref, base)
    for stage in ("forward", "train_step"):
        if stage == "train_step":
            model.initOptimizers(-1, 1.0)
            model.train_step(cam, ref, base, gt)
        r, tpg, flat, offs = _check_exact(model, W, H, (name, stage), stage == "train_step", superblock=sb)
        assert np.array_equal(r, case["design_radii"]), (name, stage)
        bc.check_expect(case, r, tpg, flat, offs)
        if sb and name in ORDER_CASES:
            _check_tile_order(model, case, offs, flat.shape[0])
    assert lib.gps_splat_can_prefetch(C.byref(model._step)) == (1 if sb else 0)
    for t in model.opt_gs_params.tensors():
        assert bool(torch.isfinite(t).all()), name


def test_one_workspace_through_wide_boxes_a_prune_and_alternating_rows():
    """the tables live in the workspace across launches: ~21 chunks per superblock on ~196 bins, then 300 Gaussians, then 4,096 more whose
    superblocks' bands are the whole grid -- every stage exact, the count table zero in between"""
    a, b = bc.model_case("one_tile_wide"), bc.model_case("alternating_rows")
    W, H = a["W"], a["H"]
    assert (W, H) == (b["W"], b["H"])
    model = _model(a, capacity=1 << 13)
    cam = _camera(a)
    ref, base, gt = _maps(W, H)
    model.initOptimizers(-1, 1.0)

    def stage(name):
        model.forward(cam, ref, base)
        _check_exact(model, W, H, (name, "forward"), False)
        model.train_step(cam, ref, base, gt)
        _check_exact(model, W, H, (name, "train_step"), True)

    stage("one_tile_wide")
    mask = torch.zeros(a["N"], dtype=torch.bool, device=DEV)
    mask[300:] = True
    model.prunePoints(mask)
    assert model.getGaussianNum() == 300
    stage("pruned to 300")
    model.add_params(_rows(b["scene"]))
    assert model.getGaussianNum() == 300 + b["N"]
    stage("alternating_rows added")


@pytest.mark.parametrize("name", ["block_edges_131073", "chunk_in_one_tile"])
def test_a_prefetched_step_bins_exactly(name):
    """the next step's histogram pass runs in the tail of this step's backward kernel: the consuming step's lists are exact"""
    case = bc.model_case(name)
    W, H = case["W"], case["H"]
    model = _model(case)
    cam, cam2 = _camera(case), _camera(case, 1, shift=0.004)
    ref, base, gt = _maps(W, H)
    model.initOptimizers(-1, 1.0)
    model.train_step(cam, ref, base, gt, next_cam=cam2)
    assert model._prefetched is not None
    model.train_step(cam2, ref, base, gt)
    torch.cuda.synchronize()
    assert int(model._step.preprocessed) == 1
    r, tpg, flat, offs = _check_exact(model, W, H, (name, "consuming step"), True)
    assert (r > 0).sum() > 0 and flat.shape[0] > 0


def test_superblock_overflow_contract():
    """isect_capacity about half the pairs of one_tile_wide: forward and train step return; counts[2] == 1, counts[0] == capacity,
    tile_offsets == min(oracle, capacity), flatten_ids[:capacity] == the oracle's sorted prefix, the class lists complete, the
    count table zero; check_binning_capacity() warns and doubles; the next step in the re-created buffers is exact, no flag."""
    from oracle import splat_ref as orc
    case = bc.model_case("one_tile_wide")
    W, H = case["W"], case["H"]
    tw, th = bc.grid(W, H)
    s = case["scene"]
    r0, m0, _, _ = orc.proj_fwd(s["means"], s["quats"], s["scales"], scenes.pose_inv(s["c2w"]), s["K"], W, H)
    n_pairs = int(bc.tiles_of(m0, np.minimum(r0, bc.MAX_RADIUS), tw, th).sum())
    cap = (n_pairs + 1) // 2 + 1000
    assert cap < n_pairs <= 2 * cap
    model = _model(case, isect_capacity=cap)
    cam = _camera(case)
    ref, base, gt = _maps(W, H)
    model.initOptimizers(-1, 1.0)
    for stage in ("forward", "train_step"):
        if stage == "forward":
            model.forward(cam, ref, base)
        else:
            model.train_step(cam, ref, base, gt)
        B, N, m2, r = _state(model)
        tpg, ids, flat, ggs, gst, offs = orc.isect_tiles(m2, r, TS, tw, th)
        assert flat.shape[0] == n_pairs
        counts = N_(B["counts"])
        assert counts.tolist() == [cap, 0, 1, N], (stage, counts)
        assert np.array_equal(N_(B["tile_offsets"]), np.minimum(offs.reshape(-1), cap)), stage
        assert np.array_equal(N_(B["flatten_ids"][:cap]), flat[:cap]), stage
        assert np.array_equal(N_(B["tiles_per_gauss"][:N]), tpg), stage
        if stage == "train_step":
            _check_class_lists(B, m2, r, tw, th, stage)
        assert _c_is_zero(model), stage
    with pytest.warns(UserWarning, match="overflowed"):
        ni, ng = model.check_binning_capacity()
    assert ni == cap and model.isect_capacity == 2 * cap and model.binning_overflows == 1
    model.train_step(cam, ref, base, gt)
    assert int(model._step.isect_capacity) == 2 * cap
    _check_exact(model, W, H, "after growing", True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model.check_binning_capacity()
