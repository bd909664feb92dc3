"""The loss-terms stage (gps_loss_terms, gps_loss_terms_exposure + gps_exposure_reduce; csrc/splat_loss.hip) at the shapes the two
float64 modules (tests/test_loss_terms_gpu.py, tests/test_loss_terms_exposure_gpu.py: 2 x 2 tiles) do not reach: one tile with a
crop of one pixel, a crop of one line across a tile boundary, an interior tile, a last tile column / row narrower than the SSIM halo
or exactly as wide, more slab rows than the slab sum has threads (270 and 816 rows against 256), more exposure partials than
gps_exposure_reduce has threads (272), and pixels no Gaussian reaches (render_colors = 0, weight_sum = 0; depth = 0 / 0 where the
raycast missed as well).  Inputs, oracles and both float32 routes are the helpers of those two modules.

1. against the float64 oracle, with the rule of those modules: per output the stage may be 2 x as far off as the float32 operator
   chain on the same inputs, + 1e-6 of the output's largest magnitude; the four scalars and the elements of d loss / d E one by
   one, each against its own magnitude.  _excluded may drop at most 2 + 1e-4 W H pixels (expected share of a pixel whose L1 sign
   the oracle decides within 1e-6: about 6e-6).
2. a frame whose depth sums are integers: terms[3] and the depth gradient exactly, so that a slab row dropped or counted twice
   changes n_valid and shows as an inequality of floats.
3. uncovered pixels: NaN in depth only at 0 / 0 and in no other output.

Measured (MI355X), stage / chain per size and output, and the excluded-pixel counts: LABBOOK.md §19."""
import numpy as np
import pytest
import torch

from tests.test_loss_terms_exposure_gpu import F, ROW, _case_e, _chain32e, _oracle64e, _row_table, _stage32e
from tests.test_loss_terms_gpu import DELTA, DEV, WEIGHTS, _case, _chain32, _excluded, _images, _lib, _oracle64, _stage32, _stream

pytestmark = pytest.mark.gpu
SPREAD = 0.8
# (W, H): tiles; what the size reaches
SMALL = [(11, 11),    # 1 x 1; the crop is one pixel, its whole window zero padding
         (43, 11),    # 2 x 1; the crop is one line of 33 pixels across the tile boundary
         (11, 43),    # 1 x 2
         (96, 96),    # 3 x 3; both extents multiples of 32, one interior tile
         (67, 99),    # 3 x 4; last column and row 3 px wide (< HALO): wholly outside the crop
         (69, 37)]    # 3 x 2; last column and row exactly HALO wide: the crop ends on the tile boundary in x and y
LARGE = [(320, 288),  # 10 x 9; 270 slab rows (second trip of the slab sum, 14-row tail), 90 exposure partials
         (544, 512)]  # 17 x 16; 816 slab rows (four trips, ragged), 272 partials (second trip of gps_exposure_reduce, 16-row tail)
CASES = [(W, H, s, d) for W, H in SMALL for s, d in WEIGHTS] + [(W, H, 0.2, 0.1) for W, H in LARGE]
TERMS = ("total", "l1", "ssim", "depth")


def _keep(o, gt, d, W, H, tag):
    """~_excluded, which may drop at most 2 + 1e-4 W H pixels"""
    ex = _excluded(o, gt, d)
    n = int(ex.sum())
    print("%s excluded pixels: %d of %d" % (tag, n, W * H))
    assert n <= 2 + 1e-4 * W * H, (n, W * H)
    return ~ex


def _compare(tag, got, chain, o, keep, names, covered=None, defined=None):
    """the tolerance rule of test_loss_terms_against_float64_autograd for every output in names.  covered ([H,W,1] or None): the
    chain's error is taken over these pixels only;  defined ([H,W,1] or None): the pixels at which depth is a number"""
    for name in names:
        ref64 = o[name]
        e_chain = (chain[name].double().cpu() - ref64).abs()
        e_got = (got[name].double().cpu() - ref64).abs()
        if name == "terms":   # four scalars, each against its own magnitude
            assert bool(torch.isfinite(got[name]).all()), name
            for k, term in enumerate(TERMS):
                print("%s %-5s: stage %.3g chain %.3g (value %.6g)" % (tag, term, float(e_got[k]), float(e_chain[k]), float(ref64[k])))
                assert float(e_got[k]) <= 2.0 * float(e_chain[k]) + 1e-6 * abs(float(ref64[k])), (term, float(e_got[k]), float(e_chain[k]))
            continue
        if name == "dE":      # the camera's twelve elements one by one; the other rows are compared exactly by the caller
            assert bool(torch.isfinite(got[name]).all()), name
            worst = max(range(12), key=lambda k: float(e_got[ROW].reshape(12)[k]) - 2.0 * float(e_chain[ROW].reshape(12)[k])
                        - 1e-6 * abs(float(ref64[ROW].reshape(12)[k])))
            print("%s %-5s: stage %.3g chain %.3g (value %.6g; element %d; all: stage %.3g chain %.3g of max %.3g)"
                  % (tag, name, float(e_got[ROW].reshape(12)[worst]), float(e_chain[ROW].reshape(12)[worst]),
                     float(ref64[ROW].reshape(12)[worst]), worst, float(e_got.max()), float(e_chain.max()), float(ref64.abs().max())))
            for k in range(12):
                eg, ec, v = (float(t[ROW].reshape(12)[k]) for t in (e_got, e_chain, ref64))
                assert eg <= 2.0 * ec + 1e-6 * abs(v), (name, k, eg, ec, v)
            continue
        sel_got = torch.ones(ref64.shape[:2] + (1,), dtype=torch.bool)
        if name in ("v_rc", "v_ra"):
            sel_got = sel_got & keep
        if name == "depth" and defined is not None:
            sel_got = sel_got & defined
        sel_chain = sel_got if covered is None else sel_got & covered
        assert bool(torch.isfinite(got[name].cpu()[sel_got.expand_as(e_got)]).all()), name
        scale = float(ref64[torch.isfinite(ref64)].abs().max())
        e_got, e_chain = e_got[sel_got.expand_as(e_got)], e_chain[sel_chain.expand_as(e_chain)]
        print("%s %-5s: stage %.3g chain %.3g of max %.3g" % (tag, name, float(e_got.max()), float(e_chain.max()), scale))
        assert float(e_got.max()) <= 2.0 * float(e_chain.max()) + 1e-6 * scale, (name, float(e_got.max()), float(e_chain.max()), scale)


def _identities(got):
    """the scalar the step reports, and what the strip backward gathers"""
    assert torch.equal(got["loss"][0], got["terms"][0])
    assert torch.equal(got["pix2"][..., 0:1], got["v_ra"]) and torch.equal(got["pix2"][..., 1:2], got["refc"] + np.float32(DELTA))


def _exposure_side(got, ins, table, W, H):
    """rgb is what the render-only compose writes for this camera, bit for bit; the rows of the table without a camera stay zero"""
    rc, ws, base, ref = ins[:4]
    rgb_c, dep_c = torch.empty_like(base), torch.empty_like(ref)
    assert _lib().gps_compose_exposure(W, H, rc.data_ptr(), ws.data_ptr(), base.data_ptr(), ref.data_ptr(), table[ROW].data_ptr(),
                                       rgb_c.data_ptr(), dep_c.data_ptr(), _stream()) == 0
    assert torch.equal(got["rgb"], rgb_c)
    others = torch.arange(F) != ROW
    assert torch.equal(got["dE"][others], torch.zeros((F - 1, 3, 4), device=DEV))
    assert float(got["dE"][ROW].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 1. float64, both instances
@pytest.mark.parametrize("W,H,s,d", CASES)
def test_plain_stage_against_float64_autograd_at_tile_and_slab_edges(W, H, s, d):
    ins_cpu, o = _case(W, H, s, d)
    ins = [t.to(DEV).contiguous() for t in ins_cpu]
    tag = "plain %dx%d s=%.1f d=%.1f" % (W, H, s, d)
    keep = _keep(o, ins_cpu[4], d, W, H, tag)
    chain = _chain32(*ins, s, d)
    got = _stage32(*ins, s, d)   # (checks the guard words behind the workspace)
    _compare(tag, got, chain, o, keep, ("rgb", "depth", "terms", "v_rc", "v_ra"))
    _identities(got)
    if d == 0:
        assert torch.equal(got["v_rc"][..., 3], torch.zeros((H, W), device=DEV))
    else:
        assert float(got["v_rc"][..., 3].abs().max()) > 0
    again = _stage32(*ins, s, d)   # bit-identical run to run
    for name in ("rgb", "depth", "terms", "v_rc", "v_ra", "pix2"):
        assert torch.equal(got[name], again[name]), name


@pytest.mark.parametrize("W,H,s,d", CASES)
def test_exposure_stage_against_float64_autograd_at_tile_and_slab_edges(W, H, s, d):
    ins_cpu, table_cpu, o = _case_e(W, H, s, d, SPREAD)
    ins = [t.to(DEV).contiguous() for t in ins_cpu]
    table = table_cpu.to(DEV).contiguous()
    tag = "exposure %dx%d s=%.1f d=%.1f" % (W, H, s, d)
    keep = _keep(o, ins_cpu[4], d, W, H, tag)
    chain = _chain32e(*ins, s, d, table)
    got = _stage32e(*ins, s, d, table)   # (checks the guard words behind the workspace and the slab, and the slab's rows)
    _compare(tag, got, chain, o, keep, ("rgb", "depth", "terms", "v_rc", "v_ra", "dE"))
    _exposure_side(got, ins, table, W, H)
    _identities(got)
    again = _stage32e(*ins, s, d, table)   # bit-identical run to run
    for name in ("rgb", "depth", "terms", "v_rc", "v_ra", "pix2", "dE"):
        assert torch.equal(got[name], again[name]), name


# ------------------------------------------------------------------------------------------------ 2. integer-valued depth sums
def _counted_depth(W, H):
    """gt_depth = 3 on a different number of pixels in every 32 x 32 tile (a permutation of 1 .. tiles over the tiles, the pixels
    spread over the tile's four waves), 0 elsewhere -> (gt_depth, number of such pixels)"""
    assert W % 32 == 0 and H % 32 == 0
    tx, tiles = W // 32, (W // 32) * (H // 32)
    assert tiles % 37 != 0 and tiles <= 1024
    gtd = torch.zeros((H, W, 1))
    for t in range(tiles):
        k = (torch.arange((t * 37) % tiles + 1) * 7) % 1024   # 37 is prime to both tile counts, 7 to 1024
        gtd[(t // tx) * 32 + k // 32, (t % tx) * 32 + k % 32, 0] = 3.0
    n = tiles * (tiles + 1) // 2
    assert int((gtd > 0).sum()) == n
    return gtd, n


@pytest.mark.parametrize("W,H", LARGE)
@pytest.mark.parametrize("instance", ["plain", "exposure"])
def test_integer_depth_sums_are_exact_over_every_slab_row(W, H, instance):
    """ssim_weight 0, depth_weight 0.1, nothing rendered, the raycast at depth 1 everywhere and a sensor depth of 3 on n_valid
    pixels: every |gt_depth - depth| is exactly 2, every tile's and the slab's sums are integers below 2^24, the depth term is
    2.0 and the depth gradient -(0.1f / (float) n_valid) / 1, in the kernel's float32 operations."""
    rc, ws, base, ref, gt, gtd = _images(W, H)
    rc, ws, ref = torch.zeros_like(rc), torch.zeros_like(ws), torch.ones_like(ref)
    gtd, n_valid = _counted_depth(W, H)
    ins = [t.to(DEV).contiguous() for t in (rc, ws, base, ref, gt, gtd)]
    if instance == "plain":
        got = _stage32(*ins, 0.0, 0.1)
    else:
        got = _stage32e(*ins, 0.0, 0.1, _row_table(SPREAD).to(DEV).contiguous())
    assert torch.equal(got["depth"], torch.ones((H, W, 1), device=DEV))
    print("%s %dx%d: n_valid %d, depth term %r" % (instance, W, H, n_valid, float(got["terms"][3])))
    assert float(got["terms"][3]) == 2.0
    g = np.float32(0.1) / np.float32(n_valid)   # dw / (float) n_valid; then / (w + bw) = 1
    want = torch.where(ins[5][..., 0] > 0, torch.full((H, W), -float(g), device=DEV), torch.zeros((H, W), device=DEV))
    assert torch.equal(got["v_rc"][..., 3].contiguous().view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(got["v_ra"]).all()) and bool(torch.isfinite(got["terms"]).all())
    _identities(got)


# ------------------------------------------------------------------------------------------------ 3. pixels no Gaussian reaches
UNCOVERED = dict(hit=(slice(60, 68), slice(28, 36)),     # raycast hit, sensor depth: depth = the raycast depth, a valid pixel
                 miss=(slice(28, 36), slice(60, 67)),    # no raycast hit, sensor depth: depth = 0 / 0
                 blind=(slice(92, 99), slice(28, 36)))   # no raycast hit, no sensor depth: depth = 0 / 0


def _uncovered_images(W, H):
    """_images with three rectangles without a Gaussian, each across a tile boundary in x and y"""
    rc, ws, base, ref, gt, gtd = (t.clone() for t in _images(W, H))
    gen = torch.Generator().manual_seed(5)
    for name, (ys, xs) in UNCOVERED.items():
        rc[0, ys, xs], ws[0, ys, xs] = 0.0, 0.0
        shape = ref[ys, xs].shape
        ref[ys, xs] = 1.0 + 2.0 * torch.rand(shape, generator=gen) if name == "hit" else 0.0
        gtd[ys, xs] = 0.0 if name == "blind" else 0.2 + 3.0 * torch.rand(shape, generator=gen)
    return rc, ws, base, ref, gt, gtd


def _oracle64_uncovered(ins, s, d, table=None):
    """_oracle64 / _oracle64e for the colour terms (depth weight 0) plus the depth term with the 0 / 0 pixels taken out BEFORE the
    division (a safe denominator under torch.where), autograd down to render_colors / weight_sum;  + 'hole': the 0 / 0 pixels"""
    rc, ws, base, ref, gt, gtd = ins
    o = dict(_oracle64(*ins, s, 0.0) if table is None else _oracle64e(*ins, s, 0.0, table))
    rc64, ws64 = rc.double().requires_grad_(True), ws.double().requires_grad_(True)
    ref64, gtd64 = ref.double(), gtd.double()
    b = (ref64 > 0).double()
    den = ws64[0] + b
    hole = (den == 0).detach()
    assert bool((rc64[0, ..., 3:][hole] == 0).all())   # 0 / 0, not x / 0
    depth = (rc64[0, ..., 3:] + ref64 * b) / torch.where(hole, torch.ones_like(den), den)
    valid = (gtd64 > 0) & (depth > 0) & ~hole
    depth_loss = (gtd64[valid] - depth[valid]).abs().mean()
    (float(np.float32(d)) * depth_loss).backward()
    terms = o["terms"].clone()
    terms[0] += float(np.float32(d)) * depth_loss.detach()
    terms[3] = depth_loss.detach()
    assert torch.equal(torch.isnan(o["depth"]), hole) and torch.equal(o["depth"][~hole], depth.detach()[~hole])
    o.update(terms=terms, v_rc=o["v_rc"] + rc64.grad[0], v_ra=o["v_ra"] + ws64.grad[0], hole=hole, valid=valid)
    return o


@pytest.mark.parametrize("instance", ["plain", "exposure"])
def test_pixels_no_gaussian_reaches_leave_nan_in_depth_alone(instance):
    """render_colors = 0 and weight_sum = 0 on three rectangles of a 67 x 99 frame (3 x 4 tiles), weights (0.2, 0.1).  Where the
    raycast missed as well, depth = (0 + 0) / (0 + 0) is NaN, as in the reference's compose.  The stage takes such a pixel out of
    the depth term (depth > 0 is false) and gives it a zero depth gradient: that is the limit of the term's gradient as the
    weight sum goes to zero with the pixel invalid, and it is what this oracle states by removing the pixel before the division.
    The reference's own dense autograd does not give that limit: the mask passes a zero gradient back to depth, the division's
    backward multiplies it by 1 / 0 and by the NaN depth, and render_colors[..., 3] and weight_sum receive NaN at those pixels
    (the operator chain does the same here, so its error is taken over the covered pixels only)."""
    W, H, s, d = 67, 99, 0.2, 0.1
    ins_cpu = _uncovered_images(W, H)
    table_cpu = _row_table(SPREAD) if instance == "exposure" else None
    o = _oracle64_uncovered(ins_cpu, s, d, table_cpu)
    rc, ws, base, ref, gt, gtd = ins_cpu
    hole, covered = o["hole"], ws[0] > 0
    inside = torch.zeros((H, W, 1), dtype=torch.bool)
    for ys, xs in UNCOVERED.values():
        inside[ys, xs] = True
    assert torch.equal(covered, ~inside)
    assert torch.equal(hole, inside & (ref == 0)) and int(hole.sum()) == 8 * 7 + 7 * 8
    ys, xs = UNCOVERED["hit"]
    assert bool(o["valid"][ys, xs].all()) and torch.equal(o["depth"][ys, xs], ref.double()[ys, xs])
    ys, xs = UNCOVERED["miss"]
    assert bool((gtd[ys, xs] > 0).all()) and not bool(o["valid"][ys, xs].any())
    ins = [t.to(DEV).contiguous() for t in ins_cpu]
    tag = "uncovered %s %dx%d s=%.1f d=%.1f" % (instance, W, H, s, d)
    keep = _keep(o, gt, d, W, H, tag)
    if instance == "plain":
        chain, got, names = _chain32(*ins, s, d), _stage32(*ins, s, d), ("rgb", "depth", "terms", "v_rc", "v_ra")
    else:
        table = table_cpu.to(DEV).contiguous()
        chain, got = _chain32e(*ins, s, d, table), _stage32e(*ins, s, d, table)
        names = ("rgb", "depth", "terms", "v_rc", "v_ra", "dE")
        _exposure_side(got, ins, table, W, H)
    # NaN in depth at 0 / 0 and nowhere else, and in nothing that goes on to the backward rasterizer or the optimiser
    assert torch.equal(torch.isnan(got["depth"]).cpu(), hole)
    for name in ("terms", "loss", "v_rc", "v_ra") + (("dE",) if instance == "exposure" else ()):
        assert bool(torch.isfinite(got[name]).all()), name
    assert bool(torch.isfinite(got["pix2"][..., 0]).all())
    invalid = ~o["valid"]
    assert int(invalid.sum()) > int(hole.sum())
    assert torch.equal(got["v_rc"][..., 3:].cpu()[invalid], torch.zeros(int(invalid.sum())))
    print("%s chain at the 0/0 pixels: v_rc[3] NaN at %d, v_ra NaN at %d of %d" % (
        tag, int(torch.isnan(chain["v_rc"][..., 3:].cpu()[hole]).sum()), int(torch.isnan(chain["v_ra"].cpu()[hole]).sum()), int(hole.sum())))
    _compare(tag, got, chain, o, keep, names, covered=covered, defined=~hole)
    _identities(got)
    again = _stage32(*ins, s, d) if instance == "plain" else _stage32e(*ins, s, d, table)
    for name in ("rgb", "terms", "v_rc", "v_ra", "pix2") + (("dE",) if instance == "exposure" else ()):
        assert torch.equal(got[name], again[name]), name
    assert torch.equal(got["depth"].view(torch.int32), again["depth"].view(torch.int32))
