"""Per-frame exposure through the SLAM loop (SLAMTrainCams: TSDF every frame, a Gaussian update every local_opt_interval frames):
the table grows by frame_num rows per update that added Gaussians on both hosts and in the overlapped / threaded schedule, the
pipeline's cameras reach their rows, and on a sequence whose frames carry an auto-exposure-like gain the option lowers the L1."""
import numpy as np
import pytest
import torch

from tests import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INTERVAL = 10   # local_opt_interval (the reference's default, both hosts)


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


def _gained(seq, gains):
    """uint8 RGBA frames of the sequence with frame k's colours scaled by gains[k] (as an auto-exposure camera would deliver them)"""
    rgb = np.clip(np.rint(seq["rgb"].astype(np.float32) * np.asarray(gains, np.float32)[:, None, None, None]), 0, 255).astype(np.uint8)
    rgba = np.concatenate([rgb, np.full(rgb.shape[:-1] + (1,), 255, np.uint8)], -1)
    return torch.as_tensor(rgba).to(DEV), torch.as_tensor(seq["depth"].astype(np.int16)).to(DEV)


def _cpp_run(h, seq, rgb, dep, n, use_exposure, overlap=False, bookkeep=True):
    """the C++ host's loop; bookkeep: the host waits for every frame's update and sums frame_num over the updates that added
    Gaussians (frame_num = local_opt_interval, + 1 into an empty model: slam_pipeline.cpp:450-526)"""
    W, H = seq["W"], seq["H"]
    eng = h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
    model = h.SLAMGaussianModel()
    model.loadConfig(dict(capacity=1 << 17, use_exposure=1 if use_exposure else 0))
    pipe = h.SLAMPipeline(eng, model, 7)
    pipe.overlap_mapping = pipe.mapping_thread = bool(overlap)
    want, updates = 0, 0
    for i in range(n):
        if bookkeep:
            added0, n0 = pipe.stats()["added"], model.getGaussianNum()   # (stats() waits for the update in flight)
        img = rgb[i][..., :3].float() / 255.0
        cam = h.Camera(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], True, torch.as_tensor(seq["c2w"][i].astype(np.float32)))
        cam.id = i
        cam.image, cam.depth = img, (dep[i].float() / 1000.0).unsqueeze(-1)
        pipe.processFrame(i, cam, rgb[i], dep[i])
        if bookkeep and pipe.stats()["added"] > added0:
            want += INTERVAL + (1 if n0 == 0 else 0)
            updates += 1
    pipe.flush()
    torch.cuda.synchronize()
    return pipe, model, want, updates


def _table_rows(model):
    E = model.getExposure()
    return 0 if E is None else int(E.shape[0])


def _moved_rows(E):
    eye = torch.eye(3, 4, device=E.device)
    return [r for r in range(E.shape[0]) if float((E[r] - eye).abs().max()) > 1e-6]


# ------------------------------------------------------------------------------------------------ 6. growth through the loop
def test_table_grows_through_slam_train_cams_on_both_hosts_and_schedules():
    h = _host()
    from gps_slam_amd.gs_model import Camera, SLAMGaussianModel
    from gps_slam_amd.slam_pipeline import SLAMPipeline
    from gps_slam_amd.tsdf_engine import TsdfEngine
    W, H, n = 160, 120, 41
    seq = synth.make_sequence(W, H, n, step_deg=0.5)
    rgb, dep = _gained(seq, 1.0 + 0.2 * np.sin(np.arange(n) * 0.3))
    # C++ host, sequential schedule, frame by frame
    pipe_c, model_c, want_c, upd_c = _cpp_run(h, seq, rgb, dep, n, True)
    assert upd_c >= 3 and _table_rows(model_c) == want_c, (upd_c, want_c, _table_rows(model_c))
    # every optimised camera has its row, and the loop's trainStep / forward have moved the rows of the cameras it trained on
    E_c = model_c.getExposure()
    assert all(c.id < want_c for c in pipe_c.optCams())
    moved = _moved_rows(E_c)
    # (the optimise lists hold the window's cameras -- every 5th frame -- and history keyframes: 9 rows of 41 on the first run)
    assert len(moved) >= 5 and model_c.exposureStep() > 0, moved
    # overlapped schedule on a worker thread (the worker grows the table): same table, same rows
    pipe_o, model_o, want_o, _ = _cpp_run(h, seq, rgb, dep, n, True, overlap=True, bookkeep=False)
    assert _table_rows(model_o) == want_c
    torch.testing.assert_close(model_o.getExposure(), E_c, rtol=1e-4, atol=1e-5)
    # option off: the loop never touches the table
    _, model_off, _, _ = _cpp_run(h, seq, rgb, dep, n, False, bookkeep=False)
    assert _table_rows(model_off) == 0
    # Python mirror, same sequence and bookkeeping
    eng_p = TsdfEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], voxel_size=0.01, mu=0.04, device=DEV)
    model_p = SLAMGaussianModel(dict(use_exposure=True), device=DEV)
    pipe_p = SLAMPipeline(eng_p, model_p, seed=7)
    want_p = 0
    for i in range(n):
        added0, n0 = pipe_p.stats["added"], model_p.getGaussianNum()
        img = rgb[i][..., :3].float() / 255.0
        cam = Camera(i, W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], seq["c2w"][i], image=img,
                     depth=(dep[i].float() / 1000.0).unsqueeze(-1), device=DEV)
        pipe_p.process_frame(i, cam, rgb[i], dep[i])
        if pipe_p.stats["added"] > added0:
            want_p += INTERVAL + (1 if n0 == 0 else 0)
    torch.cuda.synchronize()
    assert model_p.opt_gs_params.exposureRows() == want_p
    assert want_p == want_c   # (the first update's masks are the same on both hosts; later ones add Gaussians on both)
    assert len(_moved_rows(model_p.getExposure())) >= 5


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_exposure_lowers_l1_on_a_flickering_sequence():
    """150 frames at 160x120 with given poses; frame k's colours carry the gain 1 + 0.25 sin(2 pi k / 37) (0.75 .. 1.25).  After
    the run, the L1 of the final model's render of the last optimise list (window + keyframes) against those frames, with the
    option on and off, and the learned table's mean diagonal against the applied gain over the rows the loop trained.
    Measured on the first run (MI355X): L1 on 0.0385 vs off 0.0576 (ratio 0.668); 30 trained rows (the window's cameras are every
    5th frame), Pearson correlation of their mean diagonal with the gain 0.854.  Thresholds: ratio < 0.8, >= 20 rows, corr > 0.7."""
    h = _host()
    W, H, n = 160, 120, 150
    seq = synth.make_sequence(W, H, n, step_deg=0.4)
    gains = 1.0 + 0.25 * np.sin(2 * np.pi * np.arange(n) / 37.0)
    rgb, dep = _gained(seq, gains)
    l1 = {}
    for on in (False, True):
        pipe, model, _, _ = _cpp_run(h, seq, rgb, dep, n, on, bookkeep=False)
        errs = []
        with torch.no_grad():
            for cam, rc in zip(pipe.optCams(), pipe.optRaycasts()):
                res = model.forward(cam, rc["depth_map"], rc["color_map"])
                errs.append(float((res["rgb"] - cam.image).abs().mean()))
        l1[on] = float(np.mean(errs))
        if on:
            E = model.getExposure()
            rows = _moved_rows(E)
            diag = np.array([float(E[r, [0, 1, 2], [0, 1, 2]].mean()) for r in rows])
            corr = float(np.corrcoef(diag, gains[rows])[0, 1])
    print("exposure e2e: L1 on %.4f off %.4f (ratio %.3f); %d trained rows, corr(diagonal, gain) %.3f"
          % (l1[True], l1[False], l1[True] / l1[False], len(rows), corr))
    assert l1[True] < 0.8 * l1[False], l1
    assert len(rows) >= 20 and corr > 0.7, (len(rows), corr)
