"""SLAMPipeline.fused_loss_terms: with ssim_weight / depth_weight set, the optimise iterations go through trainStep (one C-ABI call,
no autograd graph) instead of forward -> computeLoss -> backward -> optimizersStep; 160x120, 11 frames, 20 iterations, as the SSIM
pipeline case of tests/test_host_cpp_gpu.py.  With the flag off the route and its bytes are the ones of a pipeline that has never
heard of the flag; the Python mirror's train_step with the same weights gives the C++ host's parameters."""
import numpy as np
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, N_FRAMES = 160, 120, 11
WEIGHTS = dict(ssim_weight=0.2, depth_weight=0.1)


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


_SEQ = {}


def _sequence():
    if not _SEQ:
        seq = synth.make_sequence(W, H, N_FRAMES, step_deg=0.5)
        rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
        _SEQ.update(seq=seq, rgb=torch.as_tensor(rgba).to(DEV), dep=torch.as_tensor(seq["depth"].astype(np.int16)).to(DEV))
    return _SEQ["seq"], _SEQ["rgb"], _SEQ["dep"]


def _params(model):
    p = model.getGaussianParms()
    return [t.clone() for t in (p.getMeans(), p.getScales(), p.getQuats(), p.getFeaturesDc(), p.getFeaturesRest(), p.getOpacities())]


def _run(h, config):
    seq, rgb, dep = _sequence()
    eng = h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
    model = h.SLAMGaussianModel()
    model.loadConfig(dict(capacity=1 << 16))
    pipe = h.SLAMPipeline(eng, model, 5)
    pipe.loadConfig(config)
    for i in range(N_FRAMES):
        c = h.Camera(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], True, torch.as_tensor(seq["c2w"][i].astype(np.float32)))
        c.id = i
        c.image = rgb[i][..., :3].float() / 255.0
        c.depth = (dep[i].float() / 1000.0).unsqueeze(-1)
        pipe.processFrame(i, c, rgb[i], dep[i])
    torch.cuda.synchronize()
    cams, rcs = pipe.optCams(), pipe.optRaycasts()
    with torch.no_grad():
        out = model.forward(cams[0], rcs[0]["depth_map"], rcs[0]["color_map"])
    l1 = float((out["rgb"] - cams[0].image).abs().mean())
    tsdf_l1 = float((rcs[0]["color_map"] - cams[0].image).abs().mean())
    return pipe, model, l1, tsdf_l1


_RUNS = {}


def _runs():
    if not _RUNS:
        h = _host()
        _RUNS["on"] = _run(h, dict(fused_loss_terms=1, **WEIGHTS))
        _RUNS["off"] = _run(h, dict(fused_loss_terms=0, **WEIGHTS))
        _RUNS["parent"] = _run(h, dict(WEIGHTS))   # a configuration without the key: the route before the flag existed
    return _RUNS


def test_fused_loss_terms_runs_the_iterations_through_train_step():
    pipe, model, l1, tsdf_l1 = _runs()["on"]
    assert pipe.fused_loss_terms and pipe.stats()["opt_iters"] == 20 and model.getGaussianNum() > 50
    assert pipe.autograd_iters == 0                                   # not one iteration through forward / computeLoss / backward
    assert all(g is None for g in model.leafGrads())                  # ... and no autograd graph ever reached the leaves
    terms = model.lossTerms()
    assert bool(torch.isfinite(terms).all()) and float(terms[2]) > 0 and float(terms[3]) > 0
    assert torch.equal(model.lossSum(), terms[0:1])
    assert l1 <= tsdf_l1 * 1.02                                       # the render is no worse than the TSDF colour
    _, _, l1_off, _ = _runs()["off"]
    print("final L1 of the first optimised view: fused %.5f, autograd route %.5f (TSDF colour %.5f)" % (l1, l1_off, tsdf_l1))
    assert abs(l1 - l1_off) <= 0.02 * l1_off


def test_flag_off_keeps_the_autograd_route_and_its_bytes():
    pipe, model, _, _ = _runs()["off"]
    pipe_p, model_p, _, _ = _runs()["parent"]
    assert not pipe.fused_loss_terms and not pipe_p.fused_loss_terms
    assert pipe.autograd_iters == 20 == pipe_p.autograd_iters and pipe.stats() == pipe_p.stats()
    for a, b in zip(_params(model), _params(model_p)):
        assert torch.equal(a, b)


def test_python_mirror_train_step_equals_the_cpp_host_with_the_same_weights():
    """one shared state, three iterations with (0.2, 0.1) on each host: the same C-ABI calls on the same values.  The pose is a pure
    translation by binary fractions, so that both hosts' world-to-camera matrices are the same floats."""
    h = _host()
    from gps_slam_amd.gs_model import Camera, SLAMGaussianModel
    from tests import scenes
    N = 2000
    g = scenes.random_gaussians(N, seed=4, scale_range=(0.01, 0.05))
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
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
    cm = h.SLAMGaussianModel()
    cm.loadConfig(dict(capacity=1 << 12))
    cm.getGaussianParms().add([t.clone() for t in tensors])
    cm.initOptimizers(-1, 1.0)
    ccam = h.Camera(W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), True, torch.as_tensor(c2w))
    ccam.id = 0
    ccam.image, ccam.depth = gt, gtd
    ccam.toGPU()
    pm = SLAMGaussianModel(dict(capacity=1 << 12, fuse_sh_rest_adam=2), device=DEV)
    pm.add_params(dict(zip(("means", "scales", "quats", "featuresDc", "featuresRest", "opacities"), [t.clone() for t in tensors])))
    pm.initOptimizers(-1, 1.0)
    pcam = Camera(0, W, H, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), c2w, image=gt, device=DEV)
    for _ in range(3):
        cm.trainStep(ccam, ref, base, None, None, WEIGHTS)
        pm.train_step(pcam, ref, base, gt, gt_depth=gtd, **WEIGHTS)
    torch.cuda.synchronize()
    assert torch.equal(cm.lossTerms(), pm.loss_terms()) and float(cm.lossTerms()[3]) > 0
    for a, b in zip(_params(cm), pm.opt_gs_params.tensors()):
        assert torch.equal(a, b[:N])
    assert not torch.equal(_params(cm)[0], tensors[0])
