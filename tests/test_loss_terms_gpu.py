"""The loss-terms stage of the fused train step (ssim_weight / depth_weight; the reference's computeLoss, raw_gs_model.cpp:369-417):
gps_loss_terms against a dense float64 formulation with autograd, the train step with the weights against the struct without them
(weights zero), against the autograd route of the C++ host (weights set), its determinism and its argument checks.

Tolerance of the float64 comparison: today's float32 operator chain (gps_compose_l1 -> torch + gps_ssim_fwd / gps_ssim_bwd, as
compute_loss and the render function's backward run it) is measured against the same oracle on the same inputs; the stage may be
2 x that far off per output (a different summation order) plus 1e-6 of the output's largest magnitude.
Measured (MI355X), stage / chain, worst over the six cases, as a fraction of the output's max: see LABBOOK.md (loss-terms entry)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTA = 0.1
G11 = [0.001028380123898387, 0.0075987582094967365, 0.036000773310661316, 0.10936068743467331, 0.21300552785396576,
       0.26601171493530273, 0.21300552785396576, 0.10936068743467331, 0.036000773310661316, 0.0075987582094967365,
       0.001028380123898387]
SIZES = [(37, 50), (64, 48)]
WEIGHTS = [(0.2, 0.0), (0.0, 0.1), (0.2, 0.1)]


def _lib():
    from gps_slam_amd._lib import lib
    return lib


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ inputs + float64 oracle
def _images(W, H, seed=11):
    """render and ground truth independent uniform; weight sums strictly positive; ref_depth with holes; gt_depth with a block of
    zeros (CPU tensors)"""
    gen = torch.Generator().manual_seed(seed + W)
    rc = torch.rand((1, H, W, 4), generator=gen)
    rc[..., 3] *= 3.0
    ws = 0.05 + 1.5 * torch.rand((1, H, W, 1), generator=gen)
    base = torch.rand((H, W, 3), generator=gen)
    ref = 4.0 * torch.rand((H, W, 1), generator=gen)
    ref[ref < 0.8] = 0.0                       # holes: no raycast hit
    gt = torch.rand((H, W, 3), generator=gen)
    gtd = 0.2 + 3.0 * torch.rand((H, W, 1), generator=gen)
    gtd[H // 4:H // 2, W // 3:2 * W // 3] = 0.0   # a block without sensor depth
    return rc, ws, base, ref, gt, gtd


def _oracle64(rc, ws, base, ref, gt, gtd, s, d):
    """dense float64: compose + the three terms, autograd down to render_colors / weight_sum"""
    rc64, ws64 = rc.double().requires_grad_(True), ws.double().requires_grad_(True)
    base, ref, gt, gtd = base.double(), ref.double(), gt.double(), gtd.double()
    rgb = (rc64[0, ..., :3] + base) / (ws64[0] + 1.0)
    b = (ref > 0).double()
    depth = (rc64[0, ..., 3:] + ref * b) / (ws64[0] + b)
    l1 = (gt - rgb).abs().mean()
    ssim_loss = torch.zeros((), dtype=torch.float64)
    if s > 0:
        g = torch.tensor(G11, dtype=torch.float32).double()
        k2 = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)
        conv = lambda x: torch.nn.functional.conv2d(x, k2, padding=5, groups=3)   # zero padding
        x, y = rgb.permute(2, 0, 1)[None], gt.permute(2, 0, 1)[None]
        C1, C2 = float(np.float32(0.01 * 0.01)), float(np.float32(0.03 * 0.03))
        mu1, mu2 = conv(x), conv(y)
        s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
        m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
        ssim_loss = 1.0 - m[:, :, 5:-5, 5:-5].mean()                               # padding == "valid"
        rgb_loss = (1.0 - float(np.float32(s))) * l1 + float(np.float32(s)) * ssim_loss
    else:
        rgb_loss = l1
    valid = (gtd > 0) & (depth > 0)
    depth_loss = (gtd[valid] - depth[valid]).abs().mean() if (d > 0 and bool(valid.any())) else torch.zeros((), dtype=torch.float64)
    total = rgb_loss + float(np.float32(d)) * depth_loss
    total.backward()
    terms = torch.stack([total.detach(), l1.detach(), ssim_loss.detach(), depth_loss.detach()])
    return dict(rgb=rgb.detach(), depth=depth.detach(), terms=terms, v_rc=rc64.grad[0], v_ra=ws64.grad[0])


def _excluded(o, gt, d):
    """pixels whose L1 sign (or depth validity) the oracle itself decides within 1e-6"""
    ex = ((gt.double() - o["rgb"]).abs() < 1e-6).any(-1, keepdim=True)
    if d > 0:
        ex = ex | (o["depth"].abs() < 1e-6)
    return ex


_CACHE = {}


def _case(W, H, s, d):
    key = (W, H, s, d)
    if key not in _CACHE:
        ins = _images(W, H)
        _CACHE[key] = (ins, _oracle64(*ins, s, d))
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ the two float32 routes
def _chain32(rc, ws, base, ref, gt, gtd, s, d):
    """today's operator chain: gps_compose_l1 -> compute_loss (torch + gps_ssim_fwd / gps_ssim_bwd) -> the compose backward as
    the render function forms it"""
    from gps_slam_amd import gsplat_wapper as gw
    lib = _lib()
    H, W = gt.shape[:2]
    rgb, depth = torch.empty_like(base), torch.empty_like(ref)
    assert lib.gps_compose_l1(W, H, rc.data_ptr(), ws.data_ptr(), base.data_ptr(), ref.data_ptr(), None, rgb.data_ptr(),
                              depth.data_ptr(), None, None, None, _stream()) == 0
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
    g_rgb = r["rgb"].grad
    Ws = ws[0]
    inv = 1.0 / (Ws + 1.0)
    v_rc = torch.zeros((H, W, 4), device=DEV)
    v_rc[..., :3] = g_rgb * inv
    v_ra = -(g_rgb * rgb).sum(-1, keepdim=True) * inv
    if r["depth"].grad is not None:
        b = (ref > 0).float()
        inv_d = 1.0 / (Ws + b)
        v_rc[..., 3:] = r["depth"].grad * inv_d
        v_ra = v_ra - r["depth"].grad * depth * inv_d
    return dict(rgb=rgb, depth=depth, terms=terms, v_rc=v_rc, v_ra=v_ra)


def _stage32(rc, ws, base, ref, gt, gtd, s, d, with_depth=True):
    lib = _lib()
    H, W = gt.shape[:2]
    refc = torch.where(ref < 0.01, torch.full_like(ref, 1000.0), ref)
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    out = dict(rgb=nan(H, W, 3), depth=nan(H, W, 1), terms=nan(4), v_rc=nan(H, W, 4), v_ra=nan(H, W, 1), pix2=nan(H, W, 2),
               loss=nan(1))
    wsz = int(lib.gps_loss_terms_workspace_floats(W, H))
    work = torch.full((wsz + 64,), float("nan"), device=DEV)
    work[wsz:] = 7.0   # guard words behind the workspace
    rcode = lib.gps_loss_terms(W, H, rc.data_ptr(), ws.data_ptr(), base.data_ptr(), ref.data_ptr(), refc.data_ptr(), DELTA,
                               gt.data_ptr(), gtd.data_ptr() if with_depth else None, s, d, out["rgb"].data_ptr(),
                               out["depth"].data_ptr(), out["terms"].data_ptr(), out["loss"].data_ptr(), out["v_rc"].data_ptr(),
                               out["v_ra"].data_ptr(), out["pix2"].data_ptr(), work.data_ptr(), _stream())
    assert rcode == 0
    torch.cuda.synchronize()
    assert torch.equal(work[wsz:], torch.full((64,), 7.0, device=DEV)), "the stage wrote behind its workspace"
    out["refc"] = refc
    return out


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("s,d", WEIGHTS)
def test_loss_terms_against_float64_autograd(W, H, s, d):
    ins_cpu, o = _case(W, H, s, d)
    ins = [t.to(DEV).contiguous() for t in ins_cpu]
    gt = ins_cpu[4]
    chain = _chain32(*ins, s, d)
    got = _stage32(*ins, s, d)
    keep = ~_excluded(o, gt, d)
    for name in ("rgb", "depth", "terms", "v_rc", "v_ra"):
        ref64 = o[name]
        e_chain = (chain[name].double().cpu() - ref64).abs()
        e_got = (got[name].double().cpu() - ref64).abs()
        assert bool(torch.isfinite(got[name]).all()), name
        if name in ("v_rc", "v_ra"):
            e_chain, e_got = e_chain[keep.expand_as(e_chain)], e_got[keep.expand_as(e_got)]
        scale = float(ref64.abs().max())
        if name == "terms":   # four scalars, each against its own magnitude
            for k, term in enumerate(("total", "l1", "ssim", "depth")):
                print("%dx%d s=%.1f d=%.1f %-5s: stage %.3g chain %.3g (value %.6g)"
                      % (W, H, s, d, term, float(e_got[k]), float(e_chain[k]), float(ref64[k])))
                assert float(e_got[k]) <= 2.0 * float(e_chain[k]) + 1e-6 * abs(float(ref64[k])), (term, float(e_got[k]), float(e_chain[k]))
            continue
        print("%dx%d s=%.1f d=%.1f %-5s: stage %.3g chain %.3g of max %.3g" % (W, H, s, d, name, float(e_got.max()), float(e_chain.max()), scale))
        assert float(e_got.max()) <= 2.0 * float(e_chain.max()) + 1e-6 * scale, (name, float(e_got.max()), float(e_chain.max()), scale)
    # the scalar the step reports, and what the strip backward gathers
    assert torch.equal(got["loss"][0], got["terms"][0])
    assert torch.equal(got["pix2"][..., 0:1], got["v_ra"]) and torch.equal(got["pix2"][..., 1:2], got["refc"] + np.float32(DELTA))
    if d == 0:
        assert torch.equal(got["v_rc"][..., 3], torch.zeros((H, W), device=DEV))
    else:
        assert float(got["v_rc"][..., 3].abs().max()) > 0
    # bit-identical run to run
    again = _stage32(*ins, s, d)
    for name in ("rgb", "depth", "terms", "v_rc", "v_ra", "pix2"):
        assert torch.equal(got[name], again[name]), name


def test_zero_valid_depth_pixels_give_a_zero_depth_term_and_finite_gradients():
    W, H = 37, 50
    ins_cpu, _ = _case(W, H, 0.2, 0.1)
    ins = [t.to(DEV).contiguous() for t in ins_cpu]
    ins[5] = torch.zeros_like(ins[5])   # no sensor depth anywhere
    got = _stage32(*ins, 0.2, 0.1)
    ref = _stage32(*ins, 0.2, 0.1, with_depth=False)
    assert float(got["terms"][3]) == 0.0
    for name in ("terms", "v_rc", "v_ra"):
        assert bool(torch.isfinite(got[name]).all()) and torch.equal(got[name], ref[name]), name


# ------------------------------------------------------------------------------------------------ through the train step
NAMES = ("means", "scales", "quats", "featuresDc", "featuresRest", "opacities")


def _scene(N, W, H, seed=3):
    g = scenes.random_gaussians(N, seed=seed, scale_range=(0.01, 0.06))
    c2w, K = scenes.default_camera(W, H, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    gt = torch.rand((H, W, 3), generator=gen).to(DEV)
    base = torch.rand((H, W, 3), generator=gen).to(DEV)
    ref = (torch.rand((H, W, 1), generator=gen) * 4).to(DEV)
    ref[ref < 0.4] = 0.0
    gtd = (0.5 + 3.0 * torch.rand((H, W, 1), generator=gen)).to(DEV)
    gtd[: H // 5] = 0.0
    tensors = [T(g["means"]), T(g["log_scales"]), T(g["quats"]), T(g["sh"][:, 0].copy()), T(g["sh"][:, 1:].copy()), T(g["opac_logit"])]
    return tensors, c2w, K, gt, base, ref, gtd


def _py_model(tensors, **cfg):
    from gps_slam_amd.gs_model import SLAMGaussianModel
    m = SLAMGaussianModel(dict(capacity=1 << 12, **cfg), device=DEV)
    m.add_params(dict(zip(NAMES, [t.clone() for t in tensors])))
    m.initOptimizers(-1, 1.0)
    return m


def _py_cam(W, H, K, c2w, gt, cam_id=0):
    from gps_slam_amd.gs_model import Camera
    return Camera(cam_id, W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), c2w, image=gt, device=DEV)


def _raw_step(m, cam, ref, base, gt, **fields):
    """gps_splat_train_step on the mirror's struct with the loss fields set by hand -> status"""
    lib = _lib()
    st = m._step_struct(cam.width, cam.height)
    m._bind_camera(st, cam, m.clamp_ref_depth(ref), base, gt)
    st.exposure = None
    st.exposure_row = -1
    for k in ("ssim_weight", "depth_weight"):
        setattr(st, k, 0.0)
    for k in ("ref_depth_raw", "gt_depth", "loss_terms", "loss_ws"):
        setattr(st, k, None)
    keep = []
    for k, v in fields.items():
        if isinstance(v, torch.Tensor):
            keep.append(v)
            v = v.data_ptr()
        setattr(st, k, v)
    m._opt["step"] += 1
    rc = lib.gps_splat_train_step(C.byref(st), m._opt["step"], _stream())
    torch.cuda.synchronize()
    for k in ("ssim_weight", "depth_weight"):
        setattr(st, k, 0.0)
    return rc


def _state(m):
    N = m.getGaussianNum()
    return [t[:N].clone() for t in m.opt_gs_params.tensors()] + [t[:N].clone() for k in ("m", "v") for t in m._opt[k]] + [m.loss_sum().clone()]


def test_all_zero_weights_run_the_step_exactly_as_without_the_fields():
    W, H = 64, 48
    tensors, c2w, K, gt, base, ref, gtd = _scene(600, W, H)
    cam = _py_cam(W, H, K, c2w, gt)
    plain, zero_w = _py_model(tensors, fuse_sh_rest_adam=2), _py_model(tensors, fuse_sh_rest_adam=2)
    work = torch.empty(int(_lib().gps_loss_terms_workspace_floats(W, H)), device=DEV)
    terms = torch.full((4,), 5.0, device=DEV)
    for _ in range(2):
        plain.train_step(cam, ref, base, gt)
        assert _raw_step(zero_w, cam, ref, base, gt, ssim_weight=0.0, depth_weight=0.0, ref_depth_raw=ref, gt_depth=gtd,
                         loss_terms=terms, loss_ws=work) == 0
    torch.cuda.synchronize()
    sp, sz = _state(plain), _state(zero_w)
    for a, b in zip(sp[:-1], sz[:-1]):   # parameters and moments
        assert torch.equal(a, b)
    # the L1 step adds its loss up with one float atomic per tile: two runs of the SAME struct agree only up to the order of those
    # additions (tests/test_exposure_gpu.py compares this scalar the same way); everything in the gradient path is bit-identical
    torch.testing.assert_close(sp[-1], sz[-1], rtol=1e-6, atol=0)
    assert torch.equal(terms, torch.full((4,), 5.0, device=DEV))   # untouched


def test_train_step_with_loss_terms_is_bit_reproducible():
    W, H = 64, 48
    tensors, c2w, K, gt, base, ref, gtd = _scene(600, W, H)
    cam = _py_cam(W, H, K, c2w, gt)
    runs = []
    for _ in range(2):
        m = _py_model(tensors, fuse_sh_rest_adam=0)
        for _ in range(2):
            m.train_step(cam, ref, base, gt, ssim_weight=0.2, depth_weight=0.1, gt_depth=gtd)
        torch.cuda.synchronize()
        runs.append(_state(m) + [g.clone() for g in m.grads()] + [m.loss_terms().clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    terms = runs[0][-1]
    assert bool(torch.isfinite(terms).all()) and float(terms[2]) > 0 and float(terms[3]) > 0
    assert torch.equal(runs[0][-8], terms[0:1])   # loss_sum() holds the total


def test_argument_errors():
    W, H = 64, 48
    tensors, c2w, K, gt, base, ref, gtd = _scene(300, W, H)
    cam = _py_cam(W, H, K, c2w, gt)
    m = _py_model(tensors)
    work = torch.empty(int(_lib().gps_loss_terms_workspace_floats(W, H)), device=DEV)
    terms = torch.zeros(4, device=DEV)
    common = dict(ref_depth_raw=ref, gt_depth=gtd, loss_terms=terms, loss_ws=work)
    st = m._step_struct(W, H)
    before = _state(m)
    # a weight without the record forward
    records = st.records
    assert _raw_step(m, cam, ref, base, gt, ssim_weight=0.2, depth_weight=0.0, records=None, **common) == -1
    st.records = records
    assert _raw_step(m, cam, ref, base, gt, ssim_weight=0.0, depth_weight=0.1, records=None, **common) == -1
    st.records = records
    # a weight together with an exposure row
    table = torch.eye(3, 4, device=DEV).repeat(2, 1, 1).contiguous()
    buf = [torch.zeros_like(table) for _ in range(3)]
    slab = torch.empty(int(_lib().gps_exposure_slab_floats(W, H)), device=DEV)
    assert _raw_step(m, cam, ref, base, gt, ssim_weight=0.2, depth_weight=0.1, exposure=table, exposure_grad=buf[0], exposure_m=buf[1],
                     exposure_v=buf[2], exposure_slab=slab, exposure_rows=2, exposure_row=0, exposure_step=1, exposure_lr=0.01,
                     **common) == -1
    m._step_struct(W, H).exposure = None
    for a, b in zip(before, _state(m)):
        assert torch.equal(a, b)   # nothing ran
    # the SSIM window does not fit: width or height below 11
    for w, h in ((10, 48), (48, 10)):
        t2, c2w2, K2, gt2, base2, ref2, gtd2 = _scene(100, w, h)
        m2 = _py_model(t2)
        cam2 = _py_cam(w, h, K2, c2w2, gt2)
        work2 = torch.empty(int(_lib().gps_loss_terms_workspace_floats(w, h)), device=DEV)
        c2 = dict(ref_depth_raw=ref2, gt_depth=gtd2, loss_terms=terms, loss_ws=work2)
        assert _raw_step(m2, cam2, ref2, base2, gt2, ssim_weight=0.2, depth_weight=0.0, **c2) == -1
        assert _raw_step(m2, cam2, ref2, base2, gt2, ssim_weight=0.0, depth_weight=0.1, **c2) == 0   # (the depth term alone needs no window)
    # a frame without a single valid depth pixel: depth term 0, finite gradients
    m3 = _py_model(tensors, fuse_sh_rest_adam=0)
    m3.train_step(cam, ref, base, gt, ssim_weight=0.2, depth_weight=0.1, gt_depth=torch.zeros_like(gtd))
    torch.cuda.synchronize()
    assert float(m3.loss_terms()[3]) == 0.0 and bool(torch.isfinite(m3.loss_terms()).all())
    for g in m3.grads():
        assert bool(torch.isfinite(g).all())


def _cpp_model(h, tensors, **cfg):
    m = h.SLAMGaussianModel()
    c = dict(capacity=1 << 12)
    c.update(cfg)
    m.loadConfig(c)
    m.getGaussianParms().add([t.clone() for t in tensors])
    return m


def _cpp_cam(h, W, H, K, c2w, image, depth):
    cam = h.Camera(W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), True, torch.as_tensor(np.asarray(c2w, np.float32)))
    cam.id = 0
    cam.image, cam.depth = image, depth
    cam.toGPU()
    return cam


@pytest.mark.parametrize("W,H,N", [(64, 48, 800), (37, 50, 2000)])
def test_gradients_through_the_whole_step_equal_the_autograd_route(W, H, N):
    """fuse_sh_rest_adam = 0, weights (0.2, 0.1): g_* of the fused step against forward -> computeLoss -> backward of the C++
    host on the same state.  Budget per Gaussian (tests/scenes.py condition_budget): the autograd route's own sensitivity to a
    1-ulp jitter of the parameters (the two routes use different backward rasterizers: strips against pixel groups)."""
    h = _host()
    tensors, c2w, K, gt, base, ref, gtd = _scene(N, W, H)
    weights = dict(ssim_weight=0.2, depth_weight=0.1)

    def autograd_route(*params):
        m = _cpp_model(h, [T(p) for p in params])
        cam = _cpp_cam(h, W, H, K, c2w, gt, gtd)
        m.initOptimizers(-1, 1.0)
        r = m.forward(cam, ref, base)
        loss = m.computeLoss(r, cam, weights)
        loss["total"].backward()
        grads = tuple(g.detach().cpu().numpy().copy() for g in m.leafGrads())
        total = float(loss["total"].detach())
        m.optimizersZeroGrad()
        return grads, total

    base_np = [t.cpu().numpy() for t in tensors]
    e_g, total_a = autograd_route(*base_np)
    budget = scenes.condition_budget(lambda *p: autograd_route(*p)[0], base_np, e_g, trials=3)
    f = _cpp_model(h, tensors, fuse_sh_rest_adam=0)
    cam = _cpp_cam(h, W, H, K, c2w, gt, gtd)
    f.initOptimizers(-1, 1.0)
    f.trainStep(cam, ref, base, None, None, weights)
    torch.cuda.synchronize()
    assert all(not g.defined() if hasattr(g, "defined") else g is None for g in f.leafGrads())   # no autograd graph
    terms = f.lossTerms()
    assert abs(float(terms[0]) - total_a) <= 1e-5 * abs(total_a)
    assert float(terms[3]) > 0 and float(terms[2]) > 0
    seen = 0
    for name, got, want, bud in zip(NAMES, f.grads(), e_g, budget):
        got = got.cpu().numpy().reshape(N, -1).astype(np.float64)
        err = np.abs(got - want.reshape(N, -1)).max(1)
        ratio = err / (bud + 1e-300)
        print("%dx%d %s: max error / budget %.3f" % (W, H, name, ratio.max()))
        assert (err <= bud).all(), (name, int((err > bud).sum()), float(ratio.max()))
        seen += int((np.abs(want.reshape(N, -1)).max(1) > 0).sum())
    assert seen > N   # the scene is on screen
