"""The record forward's per-group survivor lists (raster_ges_fwd_pk_kernel: a DPP row of 16 lanes owns a 32-pixel group of the wave's
16 x 8 half and walks only the entries whose packed pixel bounds touch that group).

gps_set_raster_fwd_group_cull(0) makes every group walk the half's whole list -- the trip structure before the group lists, in the
same code.  Outside its bounds an entry adds exact zeros, so the switch may not move one bit of any output: renders of crafted
records and lists (boxes on group corners and edges, empty, foreign, list lengths around every batch and part boundary, ragged
images), of random scenes, and two whole train steps (plain and with an exposure row).  The crafted renders are also checked
against a float64 evaluation of the definition over the whole list with NO box, with every (pixel, entry) alpha kept 1 % clear of
the 1/255 cut so that there is no accept / reject flip to excuse.  The crafted boxes are group-shape agnostic: they sit on the
corners and edges of both the 8 x 4 and the 4 x 8 grouping (GPS_FWD_GROUP_W)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTA = 0.1
f32 = np.float32


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _lib():
    from gps_slam_amd._lib import lib
    return lib


class _cull:
    """with _cull(on): ... -- the process-wide switch, back to its default (on) afterwards"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        _lib().gps_set_raster_fwd_group_cull(self.on)

    def __exit__(self, *a):
        _lib().gps_set_raster_fwd_group_cull(1)


# ------------------------------------------------------------------------------------------------ crafted records
def _box(mx, my, ca, cb, cc, opac):
    """pack_record's pixel bounds (splat_math.hpp) in float32, unfused -> x_lo, x_hi, y_lo, y_hi (int arrays)"""
    mx, my, ca, cb, cc, opac = (np.asarray(v, f32) for v in (mx, my, ca, cb, cc, opac))
    with np.errstate(invalid="ignore", divide="ignore"):
        tau = np.log(f32(255.0) * opac).astype(f32)
        det = (ca * cc - cb * cb).astype(f32)
        ex = (np.sqrt(f32(2.0) * tau * cc / det) * f32(1.01) + f32(0.01)).astype(f32)
        ey = (np.sqrt(f32(2.0) * tau * ca / det) * f32(1.01) + f32(0.01)).astype(f32)
    ok = (tau > 0) & (det > 0)
    clamp = lambda v: np.clip(v, -32768.0, 32767.0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        x_lo = np.where(ok, clamp(np.nan_to_num(np.floor(mx - ex - f32(0.5)))), 1)
        x_hi = np.where(ok, clamp(np.nan_to_num(np.ceil(mx + ex - f32(0.5)))), 0)
        y_lo = np.where(ok, clamp(np.nan_to_num(np.floor(my - ey - f32(0.5)))), 1)
        y_hi = np.where(ok, clamp(np.nan_to_num(np.ceil(my + ey - f32(0.5)))), 0)
    return x_lo, x_hi, y_lo, y_hi


def _pack(E):
    """entries E[n, 10] = {mx, my, ca, cb, cc, opac, depth, r, g, b} -> records [n, 12] float32 as gps_gauss_preprocess_fwd packs them"""
    E = np.asarray(E, f32).reshape(-1, 10)
    x_lo, x_hi, y_lo, y_hi = _box(E[:, 0], E[:, 1], E[:, 2], E[:, 3], E[:, 4], E[:, 5])
    words = lambda lo, hi: (((lo & 0xffff) | ((hi & 0xffff) << 16)) & 0xffffffff).astype(np.uint32).view(f32)
    rec = np.empty((E.shape[0], 12), f32)
    rec[:, 0:4] = E[:, 0:4]
    rec[:, 4], rec[:, 5], rec[:, 6], rec[:, 7] = E[:, 4], E[:, 5], E[:, 6], E[:, 7]
    rec[:, 8], rec[:, 9] = E[:, 8], E[:, 9]
    rec[:, 10], rec[:, 11] = words(x_lo, x_hi), words(y_lo, y_hi)
    return rec, np.stack([x_lo, x_hi, y_lo, y_hi], 1)


def _axis(lo, hi, tau, short):
    """centre and conic coefficient of an axis-aligned Gaussian whose packed bounds on this axis are exactly [lo, hi] (hi > lo): the
    centre in the middle of the pixel span, the half-extent `short` (0.1 .. 0.6 pixels) less than half the span"""
    m = 0.5 * (lo + hi + 1)
    ext = 0.5 * (hi - lo) - short
    r = (ext - 0.01) / 1.01          # sqrt(2 tau / c)
    return m, 2.0 * tau / (r * r)


class _Pool:
    """draws entries; colours, depths and opacities from a seeded generator"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def _rest(self, opac=None):
        r = self.rng
        depth = r.uniform(1.0, 1.9) if r.uniform() < 0.7 else r.uniform(2.3, 3.0)   # (the cut is at 2.1 or 1000.1: see _ref_depth)
        return [r.uniform(0.05, 0.95) if opac is None else opac, depth, r.uniform(0, 1), r.uniform(0, 1), r.uniform(0, 1)]

    def boxed(self, x_lo, x_hi, y_lo, y_hi, opac=None):
        rest = self._rest(opac)
        tau = np.log(255.0 * rest[0])
        mx, ca = _axis(x_lo, x_hi, tau, self.rng.uniform(0.1, min(0.6, 0.5 * (x_hi - x_lo) - 0.1)))
        my, cc = _axis(y_lo, y_hi, tau, self.rng.uniform(0.1, min(0.6, 0.5 * (y_hi - y_lo) - 0.1)))
        return [mx, my, ca, 0.0, cc] + rest

    def pixel(self, x, y):
        """support = the one pixel (x, y); its bounds are the 3 x 3 around it"""
        return self.boxed(x - 1, x + 1, y - 1, y + 1)

    def random(self, X0, Y0, spill=3.0):
        r = self.rng
        mx, my = X0 + r.uniform(-spill, 16 + spill), Y0 + r.uniform(-spill, 16 + spill)
        sx, sy = np.exp(r.uniform(np.log(0.25), np.log(3.0), 2))
        rho = r.uniform(-0.8, 0.8) if r.uniform() < 0.5 else 0.0
        det = sx * sx * sy * sy * (1 - rho * rho)
        return [mx, my, sy * sy / det, -rho * sx * sy / det, sx * sx / det] + self._rest()

    def span(self, X0, Y0):
        r = self.rng
        return [X0 + r.uniform(4, 12), Y0 + r.uniform(4, 12), 1 / 400.0, 0.0, 1 / 400.0] + self._rest(r.uniform(0.3, 0.9))

    def empty(self, X0, Y0):
        r = self.rng
        return [X0 + r.uniform(0, 16), Y0 + r.uniform(0, 16), 0.5, 0.0, 0.5] + self._rest(0.003)   # (below 1/255: bounds hi < lo)


GROUP_EDGES = (0, 3, 4, 7, 8, 11, 12, 15)   # first / last column (row) of every 8 x 4 and 4 x 8 group of a tile


def _special(pool, kind, X0, Y0):
    """-> one draw function per entry (drawn again, with other colours and opacity, until the entry is clear of the alpha cut)"""
    return [(lambda a=a: getattr(pool, a[0])(*a[1:])) for a in _special_args(kind, X0, Y0)]


def _special_args(kind, X0, Y0):
    if kind == "corners":       # one-pixel supports on every group corner of either grouping
        return [("pixel", X0 + x, Y0 + y) for y in GROUP_EDGES for x in GROUP_EDGES]
    if kind == "edges":         # bounds that end on the last column / row before a group edge, and that start on the edge
        out = []
        for b in (4, 8, 12):
            for other in ((0, 15), (1, 3), (5, 10), (12, 14)):
                out.append(("boxed", X0 + b - 3, X0 + b - 1, Y0 + other[0], Y0 + other[1]))
                out.append(("boxed", X0 + b, X0 + b + 2, Y0 + other[0], Y0 + other[1]))
                out.append(("boxed", X0 + other[0], X0 + other[1], Y0 + b - 3, Y0 + b - 1))
                out.append(("boxed", X0 + other[0], X0 + other[1], Y0 + b, Y0 + b + 2))
        return out
    if kind == "single_group":  # every entry inside columns 0-3, rows 0-3: one group of half 0 under either grouping
        return [("boxed", X0 + a, X0 + a + 2 + (k & 1) * (1 - a), Y0 + c, Y0 + c + 2) for k, (a, c) in enumerate([(0, 0), (1, 1), (0, 1), (1, 0)] * 10)]
    if kind == "alternating":   # left-only, right-only, left-only, ...
        return [("boxed", X0 + 1 + 8 * (k & 1), X0 + 6 + 8 * (k & 1), Y0 + (k % 5), Y0 + 9 + (k % 6)) for k in range(60)]
    if kind == "mixed":         # whole-tile, empty, and (added by the caller) entries of other tiles
        return [("span", X0, Y0)] * 6 + [("empty", X0, Y0)] * 10
    raise KeyError(kind)


def _ref_depth(W, H, seed):
    rng = np.random.default_rng(seed)
    ref = np.full((H, W), 2.0, f32)
    ref[rng.uniform(size=(H, W)) < 0.3] = 1000.0
    return ref


def _alpha64(E, xs, ys):
    """float64: sigma and opac * exp(-sigma) of entries E on pixel centres (xs, ys) -> [n_pix, n_entries]"""
    E = E.astype(np.float64)
    dx, dy = E[None, :, 0] - xs[:, None], E[None, :, 1] - ys[:, None]
    sigma = 0.5 * (E[None, :, 2] * dx * dx + E[None, :, 4] * dy * dy) + E[None, :, 3] * dx * dy
    return sigma, E[None, :, 5] * np.exp(-sigma)


def _crafted(W, H, tiles, seed):
    """tiles: per tile (row-major) a (list length, special kind or None, foreign entries) triple -> records, bounds, lists; every
    entry that comes within 1 % of the alpha cut on a pixel of a tile that lists it is drawn again"""
    tw, th = (W + 15) // 16, (H + 15) // 16
    assert len(tiles) == tw * th
    pool = _Pool(seed)
    entries, lists = [], []
    for t, (length, kind, foreign) in enumerate(tiles):
        X0, Y0 = 16 * (t % tw), 16 * (t // tw)
        ys, xs = np.mgrid[Y0:min(Y0 + 16, H), X0:min(X0 + 16, W)]
        xs, ys = xs.ravel() + 0.5, ys.ravel() + 0.5

        def clear(e):
            _, a = _alpha64(np.asarray(e, f32)[None].astype(f32), xs, ys)
            return bool((np.abs(255.0 * a - 1.0) > 0.011).all())
        def until_clear(draw):
            for _ in range(100):
                e = draw()
                if clear(e):
                    return e
            raise AssertionError("no draw of this entry is clear of the alpha cut")
        mine = [until_clear(d) for d in (_special(pool, kind, X0, Y0) if kind else [])]
        for k in range(foreign):   # entries of the tile diagonally across the image: listed here, touching nothing here
            e = pool.random(16 * ((t + 1) % tw), 16 * ((t // tw + 1) % th), spill=-2.0)
            sx = 1.0 / np.sqrt(e[2])
            if clear(e) and sx < 1.5:
                mine.append(e)
        assert len(mine) <= length or kind is None
        while len(mine) < length:
            e = pool.random(X0, Y0)
            if clear(e):
                mine.append(e)
        mine = mine[:length]
        order = pool.rng.permutation(len(mine)) if kind != "alternating" else np.arange(len(mine))
        lists.append([len(entries) + int(k) for k in order])
        entries += mine
    E = np.asarray(entries, f32).reshape(-1, 10)
    rec, bounds = _pack(E)
    offsets = np.cumsum([0] + [len(l) for l in lists])[:-1].astype(np.int32)
    flat = np.asarray([k for l in lists for k in l], np.int32)
    return E, rec, bounds, lists, offsets, flat


def _render(rec, ref, W, H, offsets, flat, n_isects, tile_order=None):
    """gps_raster_ges_fwd_rec_ordered on NaN-filled outputs -> (render_colors [H,W,4], weight sums [H,W])"""
    from gps_slam_amd._lib import check
    lib = _lib()
    rc = torch.full((1, H, W, 4), float("nan"), device=DEV)
    ra = torch.full((1, H, W, 1), float("nan"), device=DEV)
    counts = torch.tensor([n_isects, 0, 0, 0], dtype=torch.int64, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(lib.gps_raster_ges_fwd_rec_ordered(rec.shape[0], ptr(rec), ptr(ref), W, H, ptr(offsets), ptr(flat), ptr(counts), DELTA, ptr(rc),
                                             ptr(ra), ptr(tile_order) if tile_order is not None else C.c_void_p(0), sp),
          "gps_raster_ges_fwd_rec_ordered")
    torch.cuda.synchronize()
    return rc[0], ra[0, ..., 0]


def _definition64(E, lists, ref, W, H):
    """the forward's definition in float64 over each tile's WHOLE list, no bounds: alpha = min(0.999, o exp(-sigma)), counted iff the
    entry is not behind the cut, sigma >= 0 and alpha >= 1/255 -> sums of {r, g, b, depth} * alpha and of alpha; and the smallest
    distance of any 255 * o exp(-sigma) from 1 (the margin to the cut)"""
    tw = (W + 15) // 16
    rc, ra = np.zeros((H, W, 4)), np.zeros((H, W))
    margin = np.inf
    for t, l in enumerate(lists):
        if not l:
            continue
        X0, Y0 = 16 * (t % tw), 16 * (t // tw)
        ys, xs = np.mgrid[Y0:min(Y0 + 16, H), X0:min(X0 + 16, W)]
        shape = xs.shape
        xs, ys = xs.ravel(), ys.ravel()
        e = E[l].astype(np.float64)
        sigma, a = _alpha64(E[l], xs + 0.5, ys + 0.5)
        margin = min(margin, float(np.abs(255.0 * a - 1.0).min()))
        cut = ref[ys, xs].astype(np.float64) + np.float64(f32(DELTA))
        hit = (e[None, :, 6] <= cut[:, None]) & (sigma >= 0) & (a >= 1.0 / 255.0)
        a = np.where(hit, np.minimum(a, 0.999), 0.0)
        cols = np.stack([e[:, 7], e[:, 8], e[:, 9], e[:, 6]], 1)
        rc[ys, xs] = a @ cols
        ra[ys, xs] = a.sum(1)
    return rc, ra, margin


def _check_crafted(W, H, tiles, seed):
    E, rec, bounds, lists, offsets, flat = _crafted(W, H, tiles, seed)
    ref = _ref_depth(W, H, seed)
    d_rec, d_ref, d_off, d_flat = T(rec), T(ref), T(offsets), T(flat)
    with _cull(1):
        rc_on, ra_on = _render(d_rec, d_ref, W, H, d_off, d_flat, flat.size)
    with _cull(0):
        rc_off, ra_off = _render(d_rec, d_ref, W, H, d_off, d_flat, flat.size)
    assert torch.isfinite(rc_on).all() and torch.isfinite(ra_on).all()
    assert torch.equal(rc_on, rc_off) and torch.equal(ra_on, ra_off), "the group lists changed the render"
    e_rc, e_ra, margin = _definition64(E, lists, ref, W, H)
    print("%dx%d: %d entries, alpha margin to 1/255: %.3g, max weight sum %.3g" % (W, H, flat.size, margin, e_ra.max()))
    assert margin > 0.01
    np.testing.assert_allclose(rc_on.cpu().numpy(), e_rc, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(ra_on.cpu().numpy(), e_ra, rtol=2e-4, atol=2e-4)
    return bounds, lists


def test_crafted_boxes_are_what_they_claim():
    """(CPU part of the crafted scenes: _axis really yields the packed bounds it is asked for, a one-pixel support has the 3 x 3
    bounds around it, an opacity under 1/255 packs an empty box)"""
    pool = _Pool(0)
    for (x_lo, x_hi, y_lo, y_hi) in [(5, 7, 0, 15), (8, 10, 1, 2), (0, 15, 9, 11), (13, 14, 12, 14), (33, 39, 20, 23)]:
        _, b = _pack([pool.boxed(x_lo, x_hi, y_lo, y_hi)])
        assert b[0].tolist() == [x_lo, x_hi, y_lo, y_hi]
    e = pool.pixel(7, 4)
    _, b = _pack([e])
    assert b[0].tolist() == [6, 8, 3, 5]
    ys, xs = np.mgrid[0:16, 0:16]
    _, a = _alpha64(np.asarray([e], f32), xs.ravel() + 0.5, ys.ravel() + 0.5)
    assert ((a[:, 0] >= 1 / 255.0) == ((xs.ravel() == 7) & (ys.ravel() == 4))).all()
    _, b = _pack([pool.empty(0, 0)])
    assert b[0, 1] < b[0, 0] and b[0, 3] < b[0, 2]


# list lengths around the 16-trip chunk, the 64-lane vector, the 128-survivor part and the 512-entry batch
@pytest.mark.parametrize("lengths", [(0, 1, 15, 16, 17, 1025), (127, 128, 129, 511, 512, 513)])
def test_list_lengths_48x32(lengths):
    _check_crafted(48, 32, [(n, None, 0) for n in lengths], seed=sum(lengths))


def test_group_corners_edges_single_group_alternating_48x32():
    tiles = [(400, "corners", 0), (300, "edges", 0), (40, "single_group", 0), (60, "alternating", 0), (200, "mixed", 60), (0, None, 0)]
    bounds, lists = _check_crafted(48, 32, tiles, seed=7)
    b = bounds[lists[2]]   # the single-group tile: every box inside columns 0-3, rows 0-3 of tile (2, 0)
    assert (b[:, 0] >= 32).all() and (b[:, 1] <= 35).all() and (b[:, 2] >= 0).all() and (b[:, 3] <= 3).all()
    b = bounds[lists[3]]   # alternating: even entries in the tile's left 8 columns, odd ones in its right 8 (tile (0, 1))
    assert (b[0::2, 1] <= 7).all() and (b[1::2, 0] >= 8).all()
    b = bounds[lists[4]]   # mixed: some empty boxes, some that miss the tile (tile (1, 1): columns 16-31, rows 16-31)
    assert (b[:, 1] < b[:, 0]).sum() >= 5
    miss = (b[:, 1] >= b[:, 0]) & ((b[:, 1] < 16) | (b[:, 0] > 31) | (b[:, 3] < 16) | (b[:, 2] > 31))
    assert miss.sum() >= 20


@pytest.mark.parametrize("W,H", [(50, 37), (33, 17)])
def test_ragged_images(W, H):
    """the last tile column / row is 2 / 5 (1 / 1) pixels: groups partly or wholly outside the image"""
    tw, th = (W + 15) // 16, (H + 15) // 16
    kinds = ["corners", "edges", "mixed", "alternating"]
    tiles = []
    for t in range(tw * th):
        edge = (t % tw == tw - 1) or (t // tw == th - 1)
        kind = kinds[t % 4] if edge else None
        tiles.append(({"corners": 200, "edges": 530, "mixed": 130, "alternating": 60, None: 90}[kind], kind, 20 if kind == "mixed" else 0))
    _check_crafted(W, H, tiles, seed=W)


# ------------------------------------------------------------------------------------------------ random scenes
@pytest.mark.parametrize("N,W,H", [(3000, 96, 64), (4000, 50, 37), (150000, 640, 480)])
def test_random_scene(N, W, H):
    from gps_slam_amd import gsplat_ops as ops
    tw, th = (W + 15) // 16, (H + 15) // 16
    g = scenes.random_gaussians(N, seed=N + 1, scale_range=(0.003, 0.05))
    c2w, K = scenes.default_camera(W, H, seed=N + 1)
    vm = scenes.pose_inv(c2w)
    rng = np.random.default_rng(N)
    ref_depth = rng.uniform(1.5, 4.5, (H, W)).astype(f32)
    ref_depth[rng.uniform(size=(H, W)) < 0.1] = 1000.0
    rec = torch.empty((N, 12), device=DEV)
    sh = T(g["sh"])
    radii, m2, depths, conics, colors, opac = ops.gauss_preprocess_fwd(
        T(g["means"]), T(g["log_scales"]), T(g["quats"]), T(g["opac_logit"]).view(-1), sh[:, 0].contiguous(),
        sh[:, 1:].contiguous(), 3, T(vm), T(K), T(c2w[:3, 3].copy()), W, H, records=rec)
    isect = ops.isect_tiles_no_depth(m2.view(1, N, 2), radii.view(1, N), 16, tw, th)
    tref = T(ref_depth)[None, ..., None].contiguous()
    n_isects = int(isect.counts[0])
    with _cull(1):
        rc_on, ra_on = _render(rec, tref, W, H, isect.isect_offsets, isect.flatten_ids, n_isects)
    with _cull(0):
        rc_off, ra_off = _render(rec, tref, W, H, isect.isect_offsets, isect.flatten_ids, n_isects)
    assert torch.isfinite(rc_on).all() and torch.isfinite(ra_on).all()
    assert torch.equal(rc_on, rc_off) and torch.equal(ra_on, ra_off), "the group lists changed the render"
    rc1, ra1, _ = ops.rasterize_to_pixels_fwd_ges(m2, conics, colors, opac, tref, W, H, 16, isect, DELTA)
    assert ra1.max().item() > 1.0
    # the bar of test_record_streaming_forward_equals_lds_forward (test_splat_gpu.py)
    for got, ref in ((rc_on, rc1[0]), (ra_on, ra1[0, ..., 0])):
        d = (got - ref).abs()
        bad = d > (2e-4 * ref.abs() + 2e-4)
        print("groups-vs-lds: max %.3g, frac over tol %.3g" % (d.max().item(), bad.float().mean().item()))
        assert bad.float().mean().item() <= 2e-5
        assert d.max().item() < 0.05


# ------------------------------------------------------------------------------------------------ train step
@pytest.mark.parametrize("exposure", [False, True], ids=["plain", "exposure_row"])
def test_two_train_steps_are_bit_identical_with_the_switch_on_and_off(exposure):
    """Everything a train step writes, bit for bit, except the loss scalar.  The loss is the one output whose bits no launch fixes:
    every tile adds its sum of |gt - rgb| to the scalar with a float atomicAdd, in the order the tiles happen to finish
    (test_model_gpu.py and test_train_step_full_gpu.py compare it with a tolerance for the same reason).  Its terms are pinned
    through `rgb`, which must be bit-equal; the scalar itself may differ by what re-ordering a float32 sum of n = tiles
    non-negative terms can change: each order is within (n - 1) * 2^-24 * sum of the exact sum."""
    from gps_slam_amd.gs_model import Camera, SLAMGaussianModel
    N, W, H = 3000, 96, 64
    g = scenes.random_gaussians(N, seed=11, scale_range=(0.003, 0.05))
    c2w, K = scenes.default_camera(W, H, seed=11)
    gen = torch.Generator().manual_seed(11)
    gt = torch.rand((H, W, 3), generator=gen).to(DEV)
    base = torch.rand((H, W, 3), generator=gen).to(DEV)
    ref = (torch.rand((H, W, 1), generator=gen) * 3.5 + 0.5).to(DEV)
    ref[torch.rand((H, W, 1), generator=gen).to(DEV) < 0.1] = 0.0
    table = (torch.eye(3, 4).repeat(2, 1, 1) + 0.1 * (torch.rand((2, 3, 4), generator=gen) - 0.5)).to(DEV)

    def run(on):
        m = SLAMGaussianModel(dict(capacity=1 << 13, fuse_sh_rest_adam=2, strip_backward=True, use_exposure=exposure, exposure_lr=0.01),
                              device=DEV)
        m.add_params(dict(means=T(g["means"]), scales=T(g["log_scales"]), quats=T(g["quats"]), featuresDc=T(g["sh"][:, 0].copy()),
                          featuresRest=T(g["sh"][:, 1:].copy()), opacities=T(g["opac_logit"])))
        if exposure:
            m.opt_gs_params.setExposure(table)
        m.initOptimizers(-1, 3.3)
        cam = Camera(1, W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), c2w, image=gt, device=DEV)
        out = {}
        with _cull(on):
            for it in range(2):
                m.train_step(cam, ref, base, gt)
                torch.cuda.synchronize()
                B = m._B
                for k in ("loss", "render_colors", "weight_sum", "rgb", "v_render_colors", "v_render_alphas", "pix2"):
                    out["%s[%d]" % (k, it)] = B[k].clone()
                if exposure:
                    out["slab[%d]" % it] = m._exp["slab"][:12 * ((W + 15) // 16) * ((H + 15) // 16)].clone()   # (the rows the forward writes: one per tile)
                    out["exposure[%d]" % it] = m.getExposure().clone()
                    for k in ("m", "v", "g"):
                        out["exposure_%s[%d]" % (k, it)] = m._exp[k].clone()
        p = m.opt_gs_params
        for n in p.NAMES:
            out["param " + n] = p._buf[n][:N].clone()
        for k in ("m", "v"):
            for j, n in enumerate(p.NAMES):
                out["%s %s" % (k, n)] = m._opt[k][j][:N].clone()
        return out
    a, b = run(1), run(0)
    assert float(a["weight_sum[1]"].max()) > 1.0 and float(a["loss[1]"]) > 0
    if exposure:
        assert float(a["slab[1]"].abs().max()) > 0 and float((a["exposure[1]"][1] - table[1]).abs().max()) > 0
    diff = [k for k in a if not k.startswith("loss[") and not torch.equal(a[k], b[k])]
    assert not diff, diff
    n_terms = ((W + 15) // 16) * ((H + 15) // 16)
    for it in range(2):
        la, lb = float(a["loss[%d]" % it]), float(b["loss[%d]" % it])
        print("loss[%d]: on %.9g off %.9g" % (it, la, lb))
        assert abs(la - lb) <= 2 * (n_terms * (it + 1) - 1) * 2.0 ** -24 * max(la, lb)   # (the scalar accumulates over the steps)
