"""The loss-terms stage of the fused train step for a camera with an exposure row (ssim_weight / depth_weight together with
use_exposure; the reference's raw_gs_model.cpp:318-346 followed by computeLoss :369-417): gps_loss_terms_exposure against
gps_loss_terms (identity row), against a dense float64 formulation with autograd down to the table, the train step with
gps_splat_step::exposure_terms against the autograd route of the C++ host, both hosts against each other, and the argument checks.

Tolerance of the float64 comparison (the rule of tests/test_loss_terms_gpu.py): today's float32 operator chain (gps_compose_l1 ->
gps_exposure_fwd -> compute_loss -> gps_exposure_bwd + gps_exposure_reduce -> the compose backward) is measured against the same
oracle on the same inputs; the stage may be 2 x that far off per output (a different summation order) plus 1e-6 of the output's
largest magnitude."""
import numpy as np
import pytest
import torch

from tests import scenes
from tests.test_exposure_gpu import _params, _table
from tests.test_loss_terms_gpu import (DELTA, DEV, G11, NAMES, SIZES, WEIGHTS, T, _cpp_cam, _cpp_model, _excluded, _host, _images, _lib,
                                       _py_cam, _py_model, _raw_step, _scene, _stage32, _state, _stream)

pytestmark = pytest.mark.gpu
SPREADS = [0.02, 0.8]
F, ROW = 4, 2


def _row_table(spread):
    """test_exposure_gpu._table's construction on the CPU: eye(3,4) + spread (U - 0.5), F rows, seed 7; the camera's row is ROW"""
    gen = torch.Generator().manual_seed(7)
    return torch.eye(3, 4).repeat(F, 1, 1) + spread * (torch.rand((F, 3, 4), generator=gen) - 0.5)


# ------------------------------------------------------------------------------------------------ float64 oracle
def _oracle64e(rc, ws, base, ref, gt, gtd, s, d, table):
    """tests.test_loss_terms_gpu._oracle64 with rgb = lin @ E[:, :3]^T + E[:, 3] between the compose and the terms; autograd down
    to render_colors / weight_sum and to the table"""
    rc64, ws64 = rc.double().requires_grad_(True), ws.double().requires_grad_(True)
    E64 = table.double().requires_grad_(True)
    base, ref, gt, gtd = base.double(), ref.double(), gt.double(), gtd.double()
    lin = (rc64[0, ..., :3] + base) / (ws64[0] + 1.0)
    rgb = torch.matmul(lin, E64[ROW][:, :3].T) + E64[ROW][:, 3]
    b = (ref > 0).double()
    depth = (rc64[0, ..., 3:] + ref * b) / (ws64[0] + b)
    l1 = (gt - rgb).abs().mean()
    ssim_loss = torch.zeros((), dtype=torch.float64)
    if s > 0:
        g = torch.tensor(G11, dtype=torch.float32).double()
        k2 = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)
        conv = lambda x: torch.nn.functional.conv2d(x, k2, padding=5, groups=3)   # zero padding of the TRANSFORMED image
        x, y = rgb.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None]
        C1, C2 = float(np.float32(0.01 * 0.01)), float(np.float32(0.03 * 0.03))
        mu1, mu2 = conv(x), conv(y)
        s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
        m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
        ssim_loss = 1.0 - m[:, :, 5:-5, 5:-5].mean()
        rgb_loss = (1.0 - float(np.float32(s))) * l1 + float(np.float32(s)) * ssim_loss
    else:
        rgb_loss = l1
    valid = (gtd > 0) & (depth > 0)
    depth_loss = (gtd[valid] - depth[valid]).abs().mean() if (d > 0 and bool(valid.any())) else torch.zeros((), dtype=torch.float64)
    total = rgb_loss + float(np.float32(d)) * depth_loss
    total.backward()
    terms = torch.stack([total.detach(), l1.detach(), ssim_loss.detach(), depth_loss.detach()])
    return dict(rgb=rgb.detach(), depth=depth.detach(), terms=terms, v_rc=rc64.grad[0], v_ra=ws64.grad[0], dE=E64.grad)


_CACHE = {}


def _case_e(W, H, s, d, spread):
    """(inputs, table, oracle), CPU tensors, computed once"""
    key = (W, H, s, d, spread)
    if key not in _CACHE:
        ins, table = _images(W, H), _row_table(spread)
        _CACHE[key] = (ins, table, _oracle64e(*ins, s, d, table))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the two float32 routes
def _chain32e(rc, ws, base, ref, gt, gtd, s, d, table):
    """today's operator chain: gps_compose_l1 -> gps_exposure_fwd -> compute_loss (torch + gps_ssim_fwd / gps_ssim_bwd) ->
    gps_exposure_bwd + gps_exposure_reduce -> the compose backward as the render function forms it"""
    from gps_slam_amd import gsplat_wapper as gw
    lib = _lib()
    H, W = gt.shape[:2]
    P = W * H
    E = table[ROW]
    lin, depth = torch.empty_like(base), torch.empty_like(ref)
    assert lib.gps_compose_l1(W, H, rc.data_ptr(), ws.data_ptr(), base.data_ptr(), ref.data_ptr(), None, lin.data_ptr(),
                              depth.data_ptr(), None, None, None, _stream()) == 0
    rgb = torch.empty_like(lin)
    assert lib.gps_exposure_fwd(P, lin.data_ptr(), E.data_ptr(), rgb.data_ptr(), _stream()) == 0
    r = dict(rgb=rgb.clone().requires_grad_(True), depth=depth.clone().requires_grad_(True))
    loss = gw.compute_loss(r, gt, gt_depth=gtd, has_depth=True, ssim_weight=s, depth_weight=d)
    loss["total"].backward()
    l1 = (gt - rgb).abs().mean()
    ssim_loss = torch.zeros((), device=DEV)
    if s > 0:
        C1, C2 = float(np.float32(0.01 * 0.01)), float(np.float32(0.03 * 0.03))
        ssim_loss = 1.0 - gw.FusedSSIMMap.apply(C1, C2, rgb.permute(2, 0, 1).unsqueeze(0), gt.permute(2, 0, 1).unsqueeze(0), "valid",
                                                False).mean()
    terms = torch.stack([loss["total"].detach(), l1, ssim_loss, loss["depth"].detach() if d > 0 else torch.zeros((), device=DEV)])
    g_out = r["rgb"].grad.contiguous()
    g_lin = torch.empty_like(lin)
    slab = torch.empty(int(lib.gps_exposure_slab_floats(W, H)), device=DEV)
    dE = torch.full((F, 3, 4), float("nan"), device=DEV)
    assert lib.gps_exposure_bwd(P, lin.data_ptr(), E.data_ptr(), g_out.data_ptr(), g_lin.data_ptr(), slab.data_ptr(), _stream()) == 0
    assert lib.gps_exposure_reduce(slab.data_ptr(), 1024, F, ROW, dE.data_ptr(), _stream()) == 0
    Ws = ws[0]
    inv = 1.0 / (Ws + 1.0)
    v_rc = torch.zeros((H, W, 4), device=DEV)
    v_rc[..., :3] = g_lin * inv
    v_ra = -(g_lin * lin).sum(-1, keepdim=True) * inv
    if r["depth"].grad is not None:
        b = (ref > 0).float()
        inv_d = 1.0 / (Ws + b)
        v_rc[..., 3:] = r["depth"].grad * inv_d
        v_ra = v_ra - r["depth"].grad * depth * inv_d
    return dict(rgb=rgb, depth=depth, terms=terms, v_rc=v_rc, v_ra=v_ra, dE=dE)


def _stage32e(rc, ws, base, ref, gt, gtd, s, d, table):
    """gps_loss_terms_exposure + gps_exposure_reduce over its partials; workspace and slab with guard words, the slab NaN-filled"""
    lib = _lib()
    H, W = gt.shape[:2]
    refc = torch.where(ref < 0.01, torch.full_like(ref, 1000.0), ref)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    out = dict(rgb=nan(H, W, 3), depth=nan(H, W, 1), terms=nan(4), v_rc=nan(H, W, 4), v_ra=nan(H, W, 1), pix2=nan(H, W, 2),
               loss=nan(1), dE=nan(F, 3, 4))
    wsz, ssz = int(lib.gps_loss_terms_workspace_floats(W, H)), int(lib.gps_exposure_slab_floats(W, H))
    partials = int(lib.gps_loss_terms_exposure_partials(W, H))
    assert partials == ((W + 31) // 32) * ((H + 31) // 32) and 12 * partials <= ssz
    work, slab = nan(wsz + 64), nan(ssz + 64)
    work[wsz:] = 7.0   # guard words behind the workspace and the slab
    slab[ssz:] = 7.0
    E = table[ROW]
    rcode = lib.gps_loss_terms_exposure(W, H, rc.data_ptr(), ws.data_ptr(), base.data_ptr(), ref.data_ptr(), refc.data_ptr(), DELTA,
                                        gt.data_ptr(), gtd.data_ptr(), s, d, out["rgb"].data_ptr(), out["depth"].data_ptr(),
                                        out["terms"].data_ptr(), out["loss"].data_ptr(), out["v_rc"].data_ptr(),
                                        out["v_ra"].data_ptr(), out["pix2"].data_ptr(), work.data_ptr(), E.data_ptr(),
                                        slab.data_ptr(), _stream())
    assert rcode == 0
    assert lib.gps_exposure_reduce(slab.data_ptr(), partials, F, ROW, out["dE"].data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    guard = torch.full((64,), 7.0, device=DEV)
    assert torch.equal(work[wsz:], guard), "the stage wrote behind its workspace"
    assert torch.equal(slab[ssz:], guard), "the stage wrote behind the exposure slab"
    assert bool(torch.isfinite(slab[:12 * partials]).all()), "a launched workgroup left its slab row unwritten"
    assert bool(torch.isnan(slab[12 * partials:ssz]).all()), "slab rows behind the partials were written"
    out["refc"] = refc
    return out


# ------------------------------------------------------------------------------------------------ 1. identity row
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("s,d", WEIGHTS)
def test_identity_row_equals_the_plain_stage(W, H, s, d):
    """E = [I | 0]: 1 c0 + 0 c1 + 0 c2 + 0 is exact in every association, with or without fused multiply-adds"""
    ins = [t.to(DEV).contiguous() for t in _images(W, H)]
    ident = torch.eye(3, 4, device=DEV).repeat(F, 1, 1).contiguous()
    plain = _stage32(*ins, s, d)
    got = _stage32e(*ins, s, d, ident)
    for name in ("rgb", "depth", "terms", "loss", "v_rc", "v_ra", "pix2"):
        assert torch.equal(got[name], plain[name]), name


# ------------------------------------------------------------------------------------------------ 2. float64 autograd
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("s,d", WEIGHTS)
@pytest.mark.parametrize("spread", SPREADS)
def test_exposure_stage_against_float64_autograd(W, H, s, d, spread):
    ins_cpu, table_cpu, o = _case_e(W, H, s, d, spread)
    ins = [t.to(DEV).contiguous() for t in ins_cpu]
    table = table_cpu.to(DEV).contiguous()
    gt = ins_cpu[4]
    chain = _chain32e(*ins, s, d, table)
    got = _stage32e(*ins, s, d, table)
    keep = ~_excluded(o, gt, d)
    tag = "%dx%d s=%.1f d=%.1f spread=%.2f" % (W, H, s, d, spread)
    for name in ("rgb", "depth", "terms", "v_rc", "v_ra", "dE"):
        ref64 = o[name]
        e_chain = (chain[name].double().cpu() - ref64).abs()
        e_got = (got[name].double().cpu() - ref64).abs()
        assert bool(torch.isfinite(got[name]).all()), name
        if name in ("v_rc", "v_ra"):
            e_chain, e_got = e_chain[keep.expand_as(e_chain)], e_got[keep.expand_as(e_got)]
        scale = float(ref64.abs().max())
        if name == "terms":   # four scalars, each against its own magnitude
            for k, term in enumerate(("total", "l1", "ssim", "depth")):
                print("%s %-5s: stage %.3g chain %.3g (value %.6g)" % (tag, term, float(e_got[k]), float(e_chain[k]), float(ref64[k])))
                assert float(e_got[k]) <= 2.0 * float(e_chain[k]) + 1e-6 * abs(float(ref64[k])), (term, float(e_got[k]), float(e_chain[k]))
            continue
        print("%s %-5s: stage %.3g chain %.3g of max %.3g" % (tag, name, float(e_got.max()), float(e_chain.max()), scale))
        assert float(e_got.max()) <= 2.0 * float(e_chain.max()) + 1e-6 * scale, (name, float(e_got.max()), float(e_chain.max()), scale)
    # rgb is what the render-only compose writes for this camera, bit for bit
    lib = _lib()
    rc, ws, base, ref = ins[:4]
    rgb_c, dep_c = torch.empty_like(base), torch.empty_like(ref)
    assert lib.gps_compose_exposure(W, H, rc.data_ptr(), ws.data_ptr(), base.data_ptr(), ref.data_ptr(), table[ROW].data_ptr(),
                                    rgb_c.data_ptr(), dep_c.data_ptr(), _stream()) == 0
    assert torch.equal(got["rgb"], rgb_c)
    # the scalar the step reports, what the strip backward gathers, the rows of the table without a camera
    assert torch.equal(got["loss"][0], got["terms"][0])
    assert torch.equal(got["pix2"][..., 0:1], got["v_ra"]) and torch.equal(got["pix2"][..., 1:2], got["refc"] + np.float32(DELTA))
    others = torch.arange(F) != ROW
    assert torch.equal(got["dE"][others], torch.zeros((F - 1, 3, 4), device=DEV))
    assert float(got["dE"][ROW].abs().max()) > 0
    # bit-identical run to run
    again = _stage32e(*ins, s, d, table)
    for name in ("rgb", "depth", "terms", "v_rc", "v_ra", "pix2", "dE"):
        assert torch.equal(got[name], again[name]), name


# ------------------------------------------------------------------------------------------------ 3. the whole step
WEIGHT_CFG = dict(ssim_weight=0.2, depth_weight=0.1)


def _cam_with_id(h, W, H, K, c2w, image, depth, cam_id):
    cam = _cpp_cam(h, W, H, K, c2w, image, depth)
    cam.id = cam_id
    return cam


@pytest.mark.parametrize("W,H,N", [(64, 48, 800), (37, 50, 2000)])
def test_gradients_through_the_whole_step_equal_the_autograd_route_with_an_exposure_row(W, H, N):
    """use_exposure, a 2-row table of spread 0.1, cam.id = 0, weights (0.2, 0.1), fuse_sh_rest_adam = 0: g_* and the table's
    gradient of the fused step against forward -> computeLoss -> backward of the C++ host on the same state.  Budget per Gaussian
    (tests/scenes.py condition_budget): the autograd route's own sensitivity to a 1-ulp jitter of the parameters."""
    h = _host()
    tensors, c2w, K, gt, base, ref, gtd = _scene(N, W, H)
    table = _table(2, 9, 0.1)

    def autograd_route(*params):
        m = _cpp_model(h, [T(p) for p in params], use_exposure=1)
        m.getGaussianParms().setExposure(table)
        cam = _cam_with_id(h, W, H, K, c2w, gt, gtd, 0)
        m.initOptimizers(-1, 1.0)
        r = m.forward(cam, ref, base)
        loss = m.computeLoss(r, cam, WEIGHT_CFG)
        loss["total"].backward()
        grads = tuple(g.detach().cpu().numpy().copy() for g in m.leafGrads())
        total = float(loss["total"].detach())
        m.optimizersStep()   # (copies the table leaf's gradient to where exposureGrad() reports it)
        dE = m.exposureGrad().clone()
        m.optimizersZeroGrad()
        return grads, total, dE

    base_np = [t.cpu().numpy() for t in tensors]
    e_g, total_a, dE_a = autograd_route(*base_np)
    budget = scenes.condition_budget(lambda *p: autograd_route(*p)[0], base_np, e_g, trials=3)
    f = _cpp_model(h, tensors, fuse_sh_rest_adam=0, use_exposure=1)
    f.getGaussianParms().setExposure(table)
    cam = _cam_with_id(h, W, H, K, c2w, gt, gtd, 0)
    f.initOptimizers(-1, 1.0)
    f.trainStep(cam, ref, base, None, None, WEIGHT_CFG)
    torch.cuda.synchronize()
    assert all(not g.defined() if hasattr(g, "defined") else g is None for g in f.leafGrads())   # no autograd graph
    terms = f.lossTerms()
    assert abs(float(terms[0]) - total_a) <= 1e-5 * abs(total_a)
    assert float(terms[3]) > 0 and float(terms[2]) > 0
    dE = f.exposureGrad()
    rel = float((dE.double() - dE_a.double()).abs().max() / dE_a.double().abs().max())
    print("%dx%d d E: relative error %.3g" % (W, H, rel))
    assert rel < 1e-5, rel
    assert torch.equal(dE[1], torch.zeros(3, 4, device=DEV)) and f.exposureStep() == 1
    assert not torch.equal(f.getExposure()[0], table[0]) and torch.equal(f.getExposure()[1], table[1])
    seen = 0
    for name, got, want, bud in zip(NAMES, f.grads(), e_g, budget):
        got = got.cpu().numpy().reshape(N, -1).astype(np.float64)
        err = np.abs(got - want.reshape(N, -1)).max(1)
        ratio = err / (bud + 1e-300)
        print("%dx%d %s: max error / budget %.3f" % (W, H, name, ratio.max()))
        assert (err <= bud).all(), (name, int((err > bud).sum()), float(ratio.max()))
        seen += int((np.abs(want.reshape(N, -1)).max(1) > 0).sum())
    assert seen > N   # the scene is on screen


# ------------------------------------------------------------------------------------------------ 4. five iterations
def test_five_iterations_over_three_cameras_equal_the_autograd_route():
    """the set-up of tests/test_exposure_gpu.py::test_fused_train_step_equals_operator_route with the weights, 64x48, 2 000
    Gaussians, and its tolerances"""
    h = _host()
    W, H = 64, 48
    tensors, c2w, K, gt, base, ref, gtd = _scene(2000, W, H)
    cams = []
    for k in range(3):
        c2w_k = np.asarray(c2w, np.float32).copy()
        c2w_k[0, 3] += 0.01 * k
        gt_k = (gt * (0.8 + 0.2 * k)).clamp(0, 1).contiguous()
        cams.append(_cam_with_id(h, W, H, K, c2w_k, gt_k, gtd, k))
    table = _table(3, 9, 0.1)
    a_model = _cpp_model(h, tensors, use_exposure=1, exposure_lr=0.01)
    f_model = _cpp_model(h, tensors, use_exposure=1, exposure_lr=0.01)
    for m in (a_model, f_model):
        m.getGaussianParms().setExposure(table)
        m.initOptimizers(-1, 1.0)
    for it in range(5):
        cam = cams[it % 3]
        r = a_model.forward(cam, ref, base)
        a_model.computeLoss(r, cam, WEIGHT_CFG)["total"].backward()
        a_model.optimizersStep()
        a_model.optimizersZeroGrad()
        f_model.trainStep(cam, ref, base, None, None, WEIGHT_CFG)
    torch.cuda.synchronize()
    for a, b in zip(_params(a_model), _params(f_model)):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(a_model.getExposure(), f_model.getExposure(), rtol=1e-5, atol=1e-6)
    assert a_model.exposureStep() == f_model.exposureStep() == 5
    assert float((f_model.getExposure() - table).abs().max()) > 1e-3
    for a, b in zip(a_model.exposureAdamState(), f_model.exposureAdamState()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    assert all(not g.defined() if hasattr(g, "defined") else g is None for g in f_model.leafGrads())


# ------------------------------------------------------------------------------------------------ 5. Python mirror == C++ host
def test_python_mirror_train_step_equals_the_cpp_host_with_weights_and_an_exposure_row():
    """one shared state, three iterations with (0.2, 0.1) and a table on each host: the same C-ABI calls on the same values.  The
    pose is a pure translation by binary fractions, so that both hosts' world-to-camera matrices are the same floats."""
    h = _host()
    from gps_slam_amd.gs_model import Camera, SLAMGaussianModel
    W, H, N = 64, 48, 2000
    g = scenes.random_gaussians(N, seed=4, scale_range=(0.01, 0.05))
    tensors = [T(g["means"]), T(g["log_scales"]), T(g["quats"]), T(g["sh"][:, 0].copy()), T(g["sh"][:, 1:].copy()), T(g["opac_logit"])]
    K = scenes.intrinsics(W, H)
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = (0.125, -0.0625, 0.0)
    gen = torch.Generator().manual_seed(9)
    gt = torch.rand((H, W, 3), generator=gen).to(DEV)
    base = torch.rand((H, W, 3), generator=gen).to(DEV)
    ref = (torch.rand((H, W, 1), generator=gen) * 4).to(DEV)
    ref[ref < 0.4] = 0.0
    gtd = (0.5 + 3.0 * torch.rand((H, W, 1), generator=gen)).to(DEV)
    gtd[:, : W // 4] = 0.0
    table = _table(3, 5, 0.3)
    cm = h.SLAMGaussianModel()
    cm.loadConfig(dict(capacity=1 << 12, use_exposure=1, exposure_lr=0.01))
    cm.getGaussianParms().add([t.clone() for t in tensors])
    cm.getGaussianParms().setExposure(table)
    cm.initOptimizers(-1, 1.0)
    ccam = h.Camera(W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), True, torch.as_tensor(c2w))
    ccam.id = 1
    ccam.image, ccam.depth = gt, gtd
    ccam.toGPU()
    pm = SLAMGaussianModel(dict(capacity=1 << 12, fuse_sh_rest_adam=2, use_exposure=True, exposure_lr=0.01), device=DEV)
    pm.add_params(dict(zip(NAMES, [t.clone() for t in tensors])))
    pm.opt_gs_params.setExposure(table)
    pm.initOptimizers(-1, 1.0)
    pcam = Camera(1, W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), c2w, image=gt, device=DEV)
    for _ in range(3):
        cm.trainStep(ccam, ref, base, None, None, WEIGHT_CFG)
        pm.train_step(pcam, ref, base, gt, gt_depth=gtd, **WEIGHT_CFG)
    torch.cuda.synchronize()
    assert torch.equal(cm.lossTerms(), pm.loss_terms()) and float(cm.lossTerms()[3]) > 0 and float(cm.lossTerms()[2]) > 0
    for a, b in zip(_params(cm), pm.opt_gs_params.tensors()):
        assert torch.equal(a, b[:N])
    assert torch.equal(cm.getExposure(), pm.getExposure()) and not torch.equal(cm.getExposure(), table)
    assert torch.equal(cm.exposureGrad(), pm.exposureGrad())
    assert cm.exposureStep() == 3 == pm._exp["step"]
    assert not torch.equal(_params(cm)[0], tensors[0])


# ------------------------------------------------------------------------------------------------ 6. the C ABI
def test_exposure_terms_field_of_the_raw_step():
    W, H = 64, 48
    tensors, c2w, K, gt, base, ref, gtd = _scene(300, W, H)
    cam = _py_cam(W, H, K, c2w, gt)
    lib = _lib()
    work = torch.empty(int(lib.gps_loss_terms_workspace_floats(W, H)), device=DEV)
    table0 = _table(2, 9, 0.1).contiguous()

    def fields(table, bufs, terms, slab, exposure_terms):
        return dict(ssim_weight=0.2, depth_weight=0.1, ref_depth_raw=ref, gt_depth=gtd, loss_terms=terms, loss_ws=work, exposure=table,
                    exposure_grad=bufs[0], exposure_m=bufs[1], exposure_v=bufs[2], exposure_slab=slab, exposure_rows=2, exposure_row=0,
                    exposure_step=1, exposure_lr=0.01, exposure_terms=exposure_terms)

    def disarm(m):
        st = m._step_struct(W, H)
        st.exposure, st.exposure_slab, st.exposure_terms = None, None, 0

    slab = torch.empty(int(lib.gps_exposure_slab_floats(W, H)), device=DEV)
    # exposure_terms = 0: refused as before, nothing ran;  exposure_terms = 1 without a slab: refused as well
    m = _py_model(tensors)
    m._step_struct(W, H)   # (the step's buffers, loss_sum() among them)
    table, bufs, terms = table0.clone(), [torch.zeros_like(table0) for _ in range(3)], torch.full((4,), 5.0, device=DEV)
    before = _state(m)
    assert _raw_step(m, cam, ref, base, gt, **fields(table, bufs, terms, slab, 0)) == -1
    assert _raw_step(m, cam, ref, base, gt, **fields(table, bufs, terms, None, 1)) == -1
    disarm(m)
    for a, b in zip(before, _state(m)):
        assert torch.equal(a, b)
    assert torch.equal(table, table0) and torch.equal(terms, torch.full((4,), 5.0, device=DEV))
    assert all(torch.equal(b, torch.zeros_like(b)) for b in bufs)
    # everything set: the step runs; two such steps from one state give the same bytes
    runs = []
    for _ in range(2):
        m = _py_model(tensors)
        table, bufs, terms = table0.clone(), [torch.zeros_like(table0) for _ in range(3)], torch.zeros(4, device=DEV)
        assert _raw_step(m, cam, ref, base, gt, **fields(table, bufs, terms, slab, 1)) == 0
        disarm(m)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(terms).all()) and float(terms[2]) > 0 and float(terms[3]) > 0
        assert not torch.equal(table[0], table0[0]) and torch.equal(table[1], table0[1])
        assert float(bufs[0][0].abs().max()) > 0 and torch.equal(bufs[0][1], torch.zeros(3, 4, device=DEV))
        runs.append((_state(m), [table] + bufs + [terms]))
    for a, b in zip(runs[0][0][:-1] + runs[0][1], runs[1][0][:-1] + runs[1][1]):
        assert torch.equal(a, b)
    # (the loss scalar: the rule of tests/test_loss_terms_gpu.py::test_all_zero_weights_run_the_step_exactly_as_without_the_fields)
    torch.testing.assert_close(runs[0][0][-1], runs[1][0][-1], rtol=1e-6, atol=0)
    assert not torch.equal(runs[0][0][0], tensors[0])   # the parameters moved
