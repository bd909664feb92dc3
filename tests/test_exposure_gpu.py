"""Per-frame exposure compensation (use_exposure; the reference's raw_gs_model.cpp:331-346, exposureOpt :672, the table's growth
in slam_gs_model.cpp:39-47): the kernels against float64 autograd, the forward of both hosts, the fused train step against the
operator route, the table's Adam against libtorch's torch::optim::Adam, and the table's growth / persistence."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("means", "scales", "quats", "featuresDc", "featuresRest", "opacities")


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


def _lib():
    from gps_slam_amd._lib import lib
    return lib


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _scene(N=20000, W=320, H=240, seed=3):
    g = scenes.random_gaussians(N, seed=seed, scale_range=(0.004, 0.03))
    c2w, K = scenes.default_camera(W, H, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    gt = torch.rand((H, W, 3), generator=gen).to(DEV)
    base = torch.rand((H, W, 3), generator=gen).to(DEV)
    ref = (torch.rand((H, W, 1), generator=gen) * 4).to(DEV)
    ref[ref < 0.4] = 0.0
    tensors = [T(g["means"]), T(g["log_scales"]), T(g["quats"]), T(g["sh"][:, 0].copy()), T(g["sh"][:, 1:].copy()),
               T(g["opac_logit"])]
    return tensors, c2w, K, gt, base, ref


def _cpp_model(h, tensors, **cfg):
    m = h.SLAMGaussianModel()
    c = dict(capacity=1 << 16)
    c.update(cfg)
    m.loadConfig(c)
    m.getGaussianParms().add([t.clone() for t in tensors])
    return m


def _cpp_cam(h, W, H, K, c2w, image, cam_id=0):
    cam = h.Camera(W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), True,
                   torch.as_tensor(np.asarray(c2w, np.float32)))
    cam.id = cam_id
    cam.image = image
    cam.toGPU()
    return cam


def _table(F, seed, spread):
    gen = torch.Generator().manual_seed(seed)
    E = torch.eye(3, 4).repeat(F, 1, 1) + spread * (torch.rand((F, 3, 4), generator=gen) - 0.5)
    return E.to(DEV)


def _params(m):
    p = m.getGaussianParms()
    return [p.getMeans(), p.getScales(), p.getQuats(), p.getFeaturesDc(), p.getFeaturesRest(), p.getOpacities()]


def _apply64(rgb, E):
    return torch.matmul(rgb.double(), E.double()[:, :3].T) + E.double()[:, 3]


# ------------------------------------------------------------------------------------------------ 1. kernels vs float64
@pytest.mark.parametrize("W,H", [(640, 480), (1200, 680)])
@pytest.mark.parametrize("spread", [0.02, 0.8])
def test_kernels_against_float64_autograd(W, H, spread):
    lib = _lib()
    gen = torch.Generator().manual_seed(W + int(100 * spread))
    P = W * H
    rgb = torch.rand((H, W, 3), generator=gen).to(DEV)
    gt = torch.rand((H, W, 3), generator=gen).to(DEV)
    F, row = 4, 2
    table = _table(F, 7, spread)
    E = table[row]
    out = torch.empty_like(rgb)
    assert lib.gps_exposure_fwd(P, rgb.data_ptr(), E.data_ptr(), out.data_ptr(), _stream()) == 0
    # float64 autograd of the reference's expression, followed by the L1
    r64 = rgb.double().requires_grad_(True)
    E64 = table.double().requires_grad_(True)
    o64 = torch.matmul(r64, E64[row][:, :3].T) + E64[row][:, 3]
    torch.testing.assert_close(out.double(), o64.detach(), rtol=0, atol=4 * 2.0 ** -23 * float(o64.detach().abs().max()))
    # the L1 gradient on the float output (what the compose epilogue forms)
    ic = np.float32(1.0 / (3 * P))
    d = gt - out
    v_out = torch.where(d > 0, -torch.full_like(d, float(ic)), torch.where(d < 0, torch.full_like(d, float(ic)), torch.zeros_like(d)))
    o64.backward(v_out.double())
    v_rgb = torch.empty_like(rgb)
    slab = torch.empty(int(lib.gps_exposure_slab_floats(W, H)), device=DEV)
    grads = []
    for _ in range(2):
        grad = torch.full((F, 3, 4), float("nan"), device=DEV)
        assert lib.gps_exposure_bwd(P, rgb.data_ptr(), E.data_ptr(), v_out.data_ptr(), v_rgb.data_ptr(), slab.data_ptr(), _stream()) == 0
        assert lib.gps_exposure_reduce(slab.data_ptr(), 1024, F, row, grad.data_ptr(), _stream()) == 0
        grads.append(grad)
    torch.testing.assert_close(v_rgb.double(), r64.grad, rtol=0, atol=4 * 2.0 ** -23 * float(r64.grad.abs().max()))
    g64 = E64.grad
    assert torch.equal(grads[0], grads[1]), "d E must be bit-reproducible"
    assert torch.equal(grads[0][torch.arange(F) != row], torch.zeros_like(grads[0][torch.arange(F) != row]))
    rel = float((grads[0].double() - g64).abs().max() / g64.abs().max())
    assert rel < 1e-5, rel
    # the render-only compose variant == compose followed by E
    rc = torch.rand((1, H, W, 4), generator=gen).to(DEV)
    ws = torch.rand((1, H, W, 1), generator=gen).to(DEV)
    base = torch.rand((H, W, 3), generator=gen).to(DEV)
    refd = torch.rand((H, W, 1), generator=gen).to(DEV)
    rgb_c, dep_c = torch.empty_like(base), torch.empty_like(refd)
    rgb_e, dep_e = torch.empty_like(base), torch.empty_like(refd)
    assert lib.gps_compose_l1(W, H, rc.data_ptr(), ws.data_ptr(), base.data_ptr(), refd.data_ptr(), None, rgb_c.data_ptr(),
                              dep_c.data_ptr(), None, None, None, _stream()) == 0
    assert lib.gps_compose_exposure(W, H, rc.data_ptr(), ws.data_ptr(), base.data_ptr(), refd.data_ptr(), E.data_ptr(),
                                    rgb_e.data_ptr(), dep_e.data_ptr(), _stream()) == 0
    assert lib.gps_exposure_fwd(P, rgb_c.data_ptr(), E.data_ptr(), out.data_ptr(), _stream()) == 0
    assert torch.equal(rgb_e, out) and torch.equal(dep_e, dep_c)


# ------------------------------------------------------------------------------------------------ 2. the forward, both hosts
def test_forward_applies_the_cameras_row_on_both_hosts():
    h = _host()
    from gps_slam_amd.gs_model import Camera, SLAMGaussianModel
    W, H = 320, 240
    tensors, c2w, K, gt, base, ref = _scene()
    table = _table(3, 5, 0.6)
    on, off = _cpp_model(h, tensors, use_exposure=1), _cpp_model(h, tensors, use_exposure=0)
    on.getGaussianParms().setExposure(table)
    off.getGaussianParms().setExposure(table)
    pm_on = SLAMGaussianModel(dict(use_exposure=True), device=DEV)
    pm_on.add_params(dict(zip(NAMES, [t.clone() for t in tensors])))
    pm_on.opt_gs_params.setExposure(table)
    for cam_id in (1, 3, 7):
        cam = _cpp_cam(h, W, H, K, c2w, gt, cam_id)
        pcam = Camera(cam_id, W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), c2w, image=gt, device=DEV)
        with torch.no_grad():
            r_off = {k: v.clone() for k, v in off.forward(cam, ref, base).items()}
            r_on = {k: v.clone() for k, v in on.forward(cam, ref, base).items()}
            r_py = {k: v.clone() for k, v in pm_on.forward(pcam, ref, base).items()}
        # (depth is 0 / 0 where nothing was hit and there is no reference depth: NaN on both sides)
        torch.testing.assert_close(r_on["depth"], r_off["depth"], rtol=0, atol=0, equal_nan=True)
        assert torch.equal(r_on["alpha"], r_off["alpha"])
        if cam_id < 3:
            want = _apply64(r_off["rgb"], table[cam_id]).float()
            torch.testing.assert_close(r_on["rgb"], want, rtol=0, atol=2e-6)
            assert not torch.equal(r_on["rgb"], r_off["rgb"])
        else:   # no row: exactly the render without exposure
            assert torch.equal(r_on["rgb"], r_off["rgb"])
        torch.testing.assert_close(r_py["rgb"], r_on["rgb"], rtol=1e-5, atol=1e-6)
        # the grad-mode forward (operator route) applies the same transform
        on.initOptimizers(-1, 1.0)
        r_g = on.forward(cam, ref, base)
        torch.testing.assert_close(r_g["rgb"].detach(), r_on["rgb"], rtol=0, atol=2e-6)
        on.optimizersZeroGrad()


# ------------------------------------------------------------------------------------------------ 3. identity table
def test_identity_table_changes_nothing_for_the_gaussians():
    h = _host()
    W, H = 320, 240
    tensors, c2w, K, gt, base, ref = _scene()
    cfg = dict(fuse_sh_rest_adam=0)
    on, off = _cpp_model(h, tensors, use_exposure=1, **cfg), _cpp_model(h, tensors, use_exposure=0, **cfg)
    ident = torch.eye(3, 4, device=DEV).repeat(2, 1, 1)
    on.getGaussianParms().setExposure(ident)
    cam = _cpp_cam(h, W, H, K, c2w, gt, 1)
    for m in (on, off):
        m.initOptimizers(-1, 1.0)
        m.trainStep(cam, ref, base)
    torch.cuda.synchronize()
    # (the loss is summed with float atomics: equal up to their order)
    torch.testing.assert_close(on.lossSum(), off.lossSum(), rtol=1e-6, atol=0)
    for a, b in zip(on.grads(), off.grads()):
        assert torch.equal(a, b)
    for a, b in zip(_params(on), _params(off)):
        assert torch.equal(a, b)
    E = on.getExposure()
    assert float((E[1] - ident[1]).abs().max()) > 0 and torch.equal(E[0], ident[0])   # (row 0: a zero gradient moves nothing at step 1)
    assert float(on.exposureGrad()[1].abs().max()) > 0 and torch.equal(on.exposureGrad()[0], torch.zeros(3, 4, device=DEV))
    # one operator-route iteration
    on2, off2 = _cpp_model(h, tensors, use_exposure=1), _cpp_model(h, tensors, use_exposure=0)
    on2.getGaussianParms().setExposure(ident)
    res = {}
    for name, m in (("on", on2), ("off", off2)):
        m.initOptimizers(-1, 1.0)
        r = m.forward(cam, ref, base)
        loss = m.computeLoss(r, cam, dict(l1_weight=1.0))
        loss["loss"].backward()
        m.optimizersStep()
        m.optimizersZeroGrad()
        res[name] = (r["rgb"].detach().clone(), loss["loss"].detach().clone())
    assert torch.equal(res["on"][0], res["off"][0]) and torch.equal(res["on"][1], res["off"][1])
    for a, b in zip(_params(on2), _params(off2)):
        assert torch.equal(a, b)
    assert float((on2.getExposure()[1] - ident[1]).abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 4. fused == operator route
def test_fused_train_step_equals_operator_route():
    h = _host()
    W, H = 320, 240
    tensors, c2w, K, gt, base, ref = _scene()
    cams = []
    for k in range(3):
        c2w_k = np.asarray(c2w, np.float32).copy()
        c2w_k[0, 3] += 0.01 * k
        gt_k = (gt * (0.8 + 0.2 * k)).clamp(0, 1).contiguous()
        cams.append(_cpp_cam(h, W, H, K, c2w_k, gt_k, k))
    table = _table(3, 9, 0.1)
    a_model, f_model = _cpp_model(h, tensors, use_exposure=1, exposure_lr=0.01), _cpp_model(h, tensors, use_exposure=1, exposure_lr=0.01)
    for m in (a_model, f_model):
        m.getGaussianParms().setExposure(table)
        m.initOptimizers(-1, 1.0)
    for it in range(5):
        cam = cams[it % 3]
        r = a_model.forward(cam, ref, base)
        a_model.computeLoss(r, cam, dict(l1_weight=1.0))["loss"].backward()
        a_model.optimizersStep()
        a_model.optimizersZeroGrad()
        f_model.trainStep(cam, ref, base)
    torch.cuda.synchronize()
    for a, b in zip(_params(a_model), _params(f_model)):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(a_model.getExposure(), f_model.getExposure(), rtol=1e-5, atol=1e-6)
    assert a_model.exposureStep() == f_model.exposureStep() == 5
    assert float((f_model.getExposure() - table).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 5. Adam vs libtorch
def test_table_adam_equals_torch_optim_adam():
    from oracle import libtorch_adam_build
    mod = libtorch_adam_build.load()
    h = _host()
    W, H = 320, 240
    tensors, c2w, K, gt, base, ref = _scene()
    lr = 0.003
    m = _cpp_model(h, tensors, use_exposure=1, exposure_lr=lr)
    table = _table(3, 4, 0.2)
    m.getGaussianParms().setExposure(table)
    cams = [_cpp_cam(h, W, H, K, c2w, gt, k) for k in (0, 2, 5)]   # id 5: no row
    ref_opt = mod.RefAdam([table.clone()], [float(np.float32(lr))])
    for generation in range(2):
        m.initOptimizers(-1, 1.0)
        if generation:
            ref_opt.init()
        for it in range(6):
            cam = cams[it % 3]
            before = (m.getExposure().clone(), [t.clone() for t in m.exposureAdamState()], m.exposureStep())
            m.trainStep(cam, ref, base)
            torch.cuda.synchronize()
            if cam.id >= 3:   # no row: nothing stepped, nothing counted
                assert torch.equal(m.getExposure(), before[0]) and m.exposureStep() == before[2]
                for a, b in zip(m.exposureAdamState(), before[1]):
                    assert torch.equal(a, b)
                continue
            ref_opt.step([m.exposureGrad().clone()])
            mm, vv = m.exposureAdamState()
            assert torch.equal(mm, ref_opt.exp_avg()[0]) and torch.equal(vv, ref_opt.exp_avg_sq()[0])
            p_ref = ref_opt.parameters()[0]
            torch.testing.assert_close(m.getExposure(), p_ref, rtol=0, atol=1e-6 * lr)
            p_ref.copy_(m.getExposure())   # compare steps, not drift
    assert m.exposureStep() == 4


# ------------------------------------------------------------------------------------------------ 6. growth + persistence
def _maps(W, H, seed):
    gen = torch.Generator().manual_seed(seed)
    vertex = (torch.rand((H, W, 3), generator=gen) + torch.tensor([0.0, 0.0, 1.0])).to(DEV)
    normal = torch.nn.functional.normalize(torch.rand((H, W, 3), generator=gen) - 0.5, dim=-1).to(DEV)
    image = torch.rand((H, W, 3), generator=gen).to(DEV)
    return dict(vertex_map=vertex.contiguous(), normal_map=normal.contiguous()), image


def test_table_growth_and_persistence_both_hosts(tmp_path):
    h = _host()
    from gps_slam_amd.gs_model import Camera, SLAMGaussianModel
    W, H = 64, 48
    c2w, K = scenes.default_camera(W, H, seed=1)
    cm = h.SLAMGaussianModel()
    cm.loadConfig(dict(capacity=1 << 14, use_exposure=1))
    pm = SLAMGaussianModel(dict(capacity=1 << 14, use_exposure=True), device=DEV)
    off = h.SLAMGaussianModel()
    off.loadConfig(dict(capacity=1 << 14))
    want = 0
    for k, (frame_num, frac) in enumerate([(5, 0.5), (6, 0.3), (4, 0.0), (7, 0.2)]):
        maps, image = _maps(W, H, k)
        mask = (torch.rand((H, W, 1), generator=torch.Generator().manual_seed(50 + k)) < frac).to(DEV)
        cam = _cpp_cam(h, W, H, K, c2w, image, k)
        pcam = Camera(k, W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), c2w, image=image, device=DEV)
        n_c = cm.addGaussians(cam, maps, mask, 0.1, frame_num)
        n_p = pm.addGaussians(pcam, maps, mask, 0.1, frame_num)
        off.addGaussians(cam, maps, mask, 0.1, frame_num)
        assert n_c == n_p
        if n_c > 0:
            want += frame_num
        assert cm.getExposure().shape[0] == want == pm.getExposure().shape[0]
    assert want == 5 + 6 + 7
    ident = torch.eye(3, 4, device=DEV).repeat(want, 1, 1)
    assert torch.equal(cm.getExposure(), ident) and torch.equal(pm.getExposure(), ident)
    e_off = off.getExposure()   # exposure off: addGaussians leaves the table alone
    assert e_off is None or e_off.numel() == 0
    # save / load round trip
    table = _table(want, 3, 0.3)
    cm.getGaussianParms().setExposure(table)
    f = str(tmp_path / "gs.pt")
    cm.getGaussianParms().saveTensor(f)
    cm2 = h.SLAMGaussianModel()
    cm2.loadConfig(dict(capacity=1 << 14, use_exposure=1))
    cm2.getGaussianParms().loadTensor(f)
    assert torch.equal(cm2.getExposure(), table)
    # prune never touches the table
    keep = torch.ones(cm2.getGaussianNum(), dtype=torch.bool, device=DEV)
    keep[::3] = False
    cm2.prunePoints(~keep)
    assert torch.equal(cm2.getExposure(), table)
