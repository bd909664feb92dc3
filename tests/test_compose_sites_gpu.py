"""The `ges` compose (rgb = (raw + base) / (Ws + 1), depth = (raw_d + ref [ref > 0]) / (Ws + [ref > 0])), its L1 sign gradient and
its backward are written once (csrc/splat_compose.hpp) and used by every kernel that composes: gps_compose_l1, the forward
rasterizer's compose epilogue (the L1-only train step), gps_compose_exposure (forward() for a camera with an exposure row) and
the loss-terms stage.  On the same render these sites must agree BIT FOR BIT, without and with an exposure row: equalities only, no
tolerance.  Sizes ragged against both the 16-pixel raster tile and the 32-pixel loss tile; 33 x 17 has a one-pixel-wide last tile
column."""
import pytest
import torch

from tests.test_exposure_gpu import _table
from tests.test_loss_terms_exposure_gpu import F, ROW, _stage32e
from tests.test_loss_terms_gpu import DEV, _lib, _py_cam, _py_model, _scene, _stage32, _stream

pytestmark = pytest.mark.gpu
SIZES = [(37, 50), (64, 48), (33, 17)]


def _compose_l1(rc, ws, base, ref, gt):
    """gps_compose_l1 with every output -> dict"""
    H, W = gt.shape[:2]
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    out = dict(rgb=nan(H, W, 3), depth=nan(H, W, 1), loss=torch.zeros(1, device=DEV), v_rc=nan(H, W, 4), v_ra=nan(H, W, 1))
    assert _lib().gps_compose_l1(W, H, rc.data_ptr(), ws.data_ptr(), base.data_ptr(), ref.data_ptr(), gt.data_ptr(),
                                 out["rgb"].data_ptr(), out["depth"].data_ptr(), out["loss"].data_ptr(), out["v_rc"].data_ptr(),
                                 out["v_ra"].data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return out


def _images(W, H):
    """seeded random render, base colour and ground truth; ref_depth and weight_sum each with a block of zeros that overlap in part
    (depth = 0 / 0 there) -> device tensors"""
    gen = torch.Generator().manual_seed(100 * W + H)
    rc = torch.rand((1, H, W, 4), generator=gen)
    rc[..., 3] *= 3.0
    ws = 0.05 + 1.5 * torch.rand((1, H, W, 1), generator=gen)
    base = torch.rand((H, W, 3), generator=gen)
    ref = 0.5 + 4.0 * torch.rand((H, W, 1), generator=gen)
    gt = torch.rand((H, W, 3), generator=gen)
    ref[H // 4:H // 2, W // 3:] = 0.0            # no raycast hit (reaches the last tile column)
    ys, xs = slice(H // 3, 2 * H // 3), slice(W // 2, W)
    rc[0, ys, xs], ws[0, ys, xs] = 0.0, 0.0      # no Gaussian
    hole = (ws[0] == 0) & (ref == 0)
    assert int(hole.sum()) > 0 and int(((ws[0] == 0) & (ref > 0)).sum()) > 0 and int(((ws[0] > 0) & (ref == 0)).sum()) > 0
    return [t.to(DEV).contiguous() for t in (rc, ws, base, ref, gt)], hole.to(DEV)


@pytest.mark.parametrize("W,H", SIZES)
def test_compose_l1_equals_the_loss_stage_without_weights(W, H):
    """gps_compose_l1 against gps_loss_terms(ssim_weight = 0, depth_weight = 0) on the same images"""
    (rc, ws, base, ref, gt), hole = _images(W, H)
    a = _compose_l1(rc, ws, base, ref, gt)
    b = _stage32(rc, ws, base, ref, gt, torch.zeros_like(ref), 0.0, 0.0, with_depth=False)
    assert torch.equal(torch.isnan(a["depth"]), hole)
    torch.testing.assert_close(b["depth"], a["depth"], rtol=0, atol=0, equal_nan=True)
    for name in ("rgb", "v_rc", "v_ra"):
        assert bool(torch.isfinite(a[name]).all()), name
        assert torch.equal(b[name], a[name]), name


def _step_buffers(m):
    B = m._B
    return {k: B[k].clone() for k in ("render_colors", "weight_sum", "rgb", "v_render_colors", "v_render_alphas", "pix2")}


@pytest.mark.parametrize("W,H", SIZES)
def test_l1_train_step_composes_as_compose_l1_does(W, H):
    """the forward rasterizer's compose epilogue (L1-only train step of the Python model) against gps_compose_l1 run on the step's
    own render"""
    tensors, c2w, K, gt, base, ref, _ = _scene(2000, W, H)
    m = _py_model(tensors)
    m.train_step(_py_cam(W, H, K, c2w, gt), ref, base, gt)
    torch.cuda.synchronize()
    s = _step_buffers(m)
    assert float(s["weight_sum"].max()) > 0
    a = _compose_l1(s["render_colors"], s["weight_sum"], base, ref, gt)
    assert torch.equal(s["rgb"], a["rgb"])
    assert torch.equal(s["v_render_colors"][0], a["v_rc"])
    assert torch.equal(s["v_render_alphas"][0], a["v_ra"])
    assert torch.equal(s["pix2"][:, 0], a["v_ra"].reshape(-1))


@pytest.mark.parametrize("W,H", SIZES)
def test_exposure_sites_agree_bit_for_bit(W, H):
    """a camera with a non-identity exposure row: rgb of the L1-only train step, of forward() and of the loss-terms stage
    (ssim_weight 0.2); v_render_colors / v_render_alphas of the L1-only train step and of the loss-terms stage without weights, on
    the same render"""
    tensors, c2w, K, gt, base, ref, gtd = _scene(2000, W, H)
    table = _table(F, 5, 0.6)
    m = _py_model(tensors, use_exposure=True)
    m.opt_gs_params.setExposure(table)
    cam = _py_cam(W, H, K, c2w, gt, cam_id=ROW)
    assert m.exposure_row(cam) == ROW
    rgb_forward = m.forward(cam, ref, base)["rgb"].clone()
    m.train_step(cam, ref, base, gt)   # (steps the table: `table` keeps the row the step composed with)
    torch.cuda.synchronize()
    s = _step_buffers(m)
    assert float(s["weight_sum"].max()) > 0 and not torch.equal(m.getExposure()[ROW], table[ROW])
    ssim = _stage32e(s["render_colors"], s["weight_sum"], base, ref, gt, gtd, 0.2, 0.0, table)
    l1 = _stage32e(s["render_colors"], s["weight_sum"], base, ref, gt, gtd, 0.0, 0.0, table)
    assert torch.equal(rgb_forward, ssim["rgb"]) and torch.equal(l1["rgb"], ssim["rgb"])
    assert torch.equal(s["rgb"], rgb_forward)
    assert torch.equal(s["v_render_colors"][0], l1["v_rc"])
    assert torch.equal(s["v_render_alphas"][0], l1["v_ra"])
