"""SLAMPipeline.fused_loss_terms in a use_exposure run: with ssim_weight / depth_weight set and almost every camera holding a row
of the exposure table, the optimise iterations go through trainStep (gps_splat_step::exposure_terms) instead of forward ->
computeLoss -> backward -> optimizersStep; the sequence and configuration of tests/test_loss_terms_pipeline_gpu.py with the
frames' colours scaled by a gain of 0.75 .. 1.25 as in tests/test_exposure_pipeline_gpu.py."""
import numpy as np
import pytest
import torch

from tests import synth
from tests.test_exposure_pipeline_gpu import _gained
from tests.test_loss_terms_pipeline_gpu import H, N_FRAMES, W, WEIGHTS, _host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(h, config):
    seq = synth.make_sequence(W, H, N_FRAMES, step_deg=0.5)
    rgb, dep = _gained(seq, 1.0 + 0.25 * np.sin(2 * np.pi * np.arange(N_FRAMES) / 8.0))
    eng = h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
    model = h.SLAMGaussianModel()
    model.loadConfig(dict(capacity=1 << 16, use_exposure=1))
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
    return pipe, model, l1


_RUNS = {}


def _runs():
    if not _RUNS:
        h = _host()
        _RUNS["on"] = _run(h, dict(fused_loss_terms=1, **WEIGHTS))
        _RUNS["off"] = _run(h, dict(fused_loss_terms=0, **WEIGHTS))
    return _RUNS


def _rows(model):
    E = model.getExposure()
    return 0 if E is None else int(E.shape[0])


def test_fused_loss_terms_serves_the_cameras_with_an_exposure_row():
    pipe, model, l1 = _runs()["on"]
    pipe_off, model_off, l1_off = _runs()["off"]
    assert pipe.fused_loss_terms and model.use_exposure and model.getGaussianNum() > 50
    assert pipe.stats()["opt_iters"] == pipe_off.stats()["opt_iters"] > 0
    assert pipe.autograd_iters == 0                                   # not one iteration through forward / computeLoss / backward
    assert all(g is None for g in model.leafGrads())                  # ... and no autograd graph ever reached the leaves
    terms = model.lossTerms()
    assert bool(torch.isfinite(terms).all()) and float(terms[2]) > 0 and float(terms[3]) > 0
    assert _rows(model) == _rows(model_off) > 0
    assert all(0 <= c.id < _rows(model) for c in pipe.optCams())      # the optimised cameras have their rows
    E = model.getExposure()
    assert float((E - torch.eye(3, 4, device=E.device)).abs().max()) > 1e-3 and model.exposureStep() > 0
    print("final L1 of the first optimised view: fused %.5f, autograd route %.5f" % (l1, l1_off))
    assert abs(l1 - l1_off) <= 0.02 * l1_off


def test_flag_off_keeps_the_autograd_route():
    pipe, model, _ = _runs()["off"]
    assert not pipe.fused_loss_terms
    assert pipe.autograd_iters == pipe.stats()["opt_iters"] > 0
