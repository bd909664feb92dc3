"""A session run from one of the reference's configuration files (gps_slam_amd/host/session.hpp, config_node.hpp): the node-typed
entry points against the flat gpsh::Config route, train -> save -> evaluate from disk with fresh objects, and work_mode recon.

Shape: 64 x 48 images (4 x 3 tiles, ragged last tile row), 12 frames, local_opt_interval 10 / local_opt_iters 4 /
keyframe_select_max 2 and a capacity of 4096 Gaussians -- exactly one map update, at frame 10, and two frames behind it.  The
YAML is the text of release/replica/office0.yaml with those values substituted (2 cm voxels and small hash tables: the engine's
files are then 33 MB, not 1 GB)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import digests, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFICE0 = os.path.join(ROOT, "tests", "golden", "configs", "release", "replica", "office0.yaml")
W, H, N = 64, 48, 12
SEED = 11


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


@pytest.fixture(scope="module")
def seq():
    return synth.make_sequence(W, H, N, step_deg=0.5)


def _yaml(seq, workspace, work_mode="train"):
    text = open(OFFICE0).read()

    def sub(old, new):
        nonlocal text
        assert text.count(old) == 1, old
        text = text.replace(old, new)

    sub("workspace_dir: output/release/replica/office0", "workspace_dir: %s" % workspace)
    sub("work_mode: train", "work_mode: %s" % work_mode)
    sub("intrinsics: [600, 600, 599.5, 339.5]", "intrinsics: [%r, %r, %r, %r]" % (seq["fx"], seq["fy"], seq["cx"], seq["cy"]))
    sub("image_shape: [1200, 680] ", "image_shape: [%d, %d] " % (W, H))
    sub("  end_frame: 1999", "  end_frame: %d" % (N - 1))
    sub("  local_opt_iters: 20", "  local_opt_iters: 4")
    sub("  keyframe_select_max: 7", "  keyframe_select_max: 2")
    sub("    voxel_size: 0.005\n    trunc_dist: 0.02\n",
        "    voxel_size: 0.02\n    trunc_dist: 0.08\n    sdf_local_block_num: 8192\n    sdf_bucket_num: 32768\n    sdf_excess_list_size: 4096\n")
    sub("  delta_depth: 0.1\n", "  delta_depth: 0.1\n  capacity: 4096\n")
    return text


# the same values, flattened by hand, for the gpsh::Config route
FLAT_MODEL = dict(render_method="ges", max_gs_radii=100, delta_depth=0.1, capacity=4096, sh_degree=3, sh_degree_interval=0,
                  max_init_scale=0.01, min_init_scale=-1, default_opacities=0.5, means_lr=0.00016, scales_lr=0.005, quats_lr=0.001,
                  featuresDc_lr=0.0025, featuresRest_lr=0.0005, opacities_lr=5e-2, exposure_lr=0.003, use_exposure=0)
FLAT_TSDF = dict(voxel_size=0.02, trunc_dist=0.08, viewFrustum_min=0.2, viewFrustum_max=10, use_gt_pose=1, sdf_local_block_num=8192,
                 sdf_bucket_num=32768, sdf_excess_list_size=4096)
FLAT_PIPE = dict(max_iterations=10000, enable_densify=0, eval_after_train=1, save_after_train=1, selected_cam_idx=-1, model_path="/gs_model",
                 log_path="/log", eval_path="/val", log_iter=1000, ssim_weight=0.0, depth_weight=0.0, color_error_max=0.1, depth_error_max=0.1,
                 depth_vis_max=5, depth_vis_min=0, alpha_vis_max=5, log_slam_state=0, new_gs_sample_ratio=0.25, color_error_thres=0.05,
                 localframe_cam_window_length=2, localframe_cam_window_interval=5, local_opt_iters=4, local_opt_interval=10,
                 keyframe_theta_thres=30, keyframe_trans_thres=0.3, keyframe_select_max=2, loss_thres=0.02, sample_method="random",
                 large_scale_thres=0.1, small_scale_thres=0.003, low_opac_thres=0.005, saved_mesh="tsdf_mesh.ply",
                 saved_engine="tsdf_engine/", saved_images="raycasted")


def _cameras(h, seq, reader=None):
    cams = []
    for i in range(N):
        c = h.Camera(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], True, torch.as_tensor(seq["c2w"][i].astype(np.float32)))
        c.id = i
        c.img_name = "frame%06d.jpg" % i
        c.image = torch.as_tensor(seq["rgb"][i].astype(np.float32) / 255.0)          # host tensors, as a dataset reader holds them
        c.depth = torch.as_tensor(seq["depth"][i].astype(np.float32) / 1000.0)[..., None]
        if reader is not None:
            reader.addTrainCamera(c)
        cams.append(c)
    return cams


def _file_crc(path):
    return digests.crc(np.fromfile(path, np.uint8))


def _scene_digest(h, cli, tmp):
    """the whole volume as the engine's own files hold it (voxel array, allocation list, hash table, excess list, the two counters),
    the live raycast and the counters"""
    eng = cli.getMainEngine()
    torch.cuda.synchronize()
    os.makedirs(tmp, exist_ok=True)
    eng.SaveToFile(str(tmp))
    d = {name: _file_crc(os.path.join(str(tmp), "Scene", name)) for name in ("voxel.dat", "alloc.dat", "hash.dat", "excess.dat", "vba.txt", "last.txt")}
    d["live"] = digests.crc(eng.GetLiveVertex().cpu().numpy())
    d["counters"] = eng.counters().cpu()[:3].tolist()
    return d


def _model_tensors(model):
    p = model.getGaussianParms()
    tensors = (p.getMeans(), p.getScales(), p.getQuats(), p.getFeaturesDc(), p.getFeaturesRest(), p.getOpacities(), p.getExposure())
    return [None if t is None else t.clone() for t in tensors]     # (no exposure table without use_exposure)


def test_node_route_equals_flat_route(seq, tmp_path):
    h = _host()
    ws = str(tmp_path / "ws")
    cfg = tmp_path / "office0.yaml"
    cfg.write_text(_yaml(seq, ws))
    root = h.load_yaml(str(cfg))

    def run(route):
        reader = h.DatasetReader()
        model = h.SLAMGaussianModel()
        pipe = h.SLAMPipeline(SEED)
        if route == "node":
            reader.loadConfig(root["READER"])
            _cameras(h, seq, reader)
            cli = h.createTsdfEngine(reader, root["PIPE"]["TSDF"])
            model.loadConfig(root["MODEL"])
            pipe.setTsdfEngine(cli)
            pipe.scene_scale = reader.scene_scale
            pipe.loadConfig(root["PIPE"], ws, False)
        else:
            reader = h.DatasetReader(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"])
            _cameras(h, seq, reader)
            cli = h.createTsdfEngine(reader, FLAT_TSDF)
            model.loadConfig(FLAT_MODEL)
            pipe.setTsdfEngine(cli)
            pipe.workspace_dir = ws
            pipe.loadConfig(dict(FLAT_PIPE, scene_scale=float(np.float32(1.1) * np.float32(1.0))))
        cams = pipe.SLAMTrainCamsModel(model, reader.trainCameras())
        torch.cuda.synchronize()
        out = dict(tensors=_model_tensors(model), digest=_scene_digest(h, cli, tmp_path / ("engine_" + route)), keyframes=pipe.keyframeCount(),
                   stats=pipe.stats(), pipe=pipe.settings(), model=model.settings(), poses=[c.c2w_slam.clone() for c in cams],
                   size=(reader.width, reader.height, reader.fx, reader.fy, reader.cx, reader.cy))
        cli.Shutdown()
        return out

    a, b = run("node"), run("flat")
    assert a["size"] == b["size"] == (W, H, float(np.float32(seq["fx"])), float(np.float32(seq["fy"])), float(np.float32(seq["cx"])), float(np.float32(seq["cy"])))
    assert a["stats"] == b["stats"] and a["stats"]["frames"] == N and a["stats"]["opt_iters"] == 4 and a["stats"]["added"] > 100, a["stats"]
    assert a["tensors"][0].shape[0] > 100 and a["tensors"][0].shape[0] <= 4096
    assert [t is None for t in a["tensors"]] == [t is None for t in b["tensors"]] == [False] * 6 + [True]
    for x, y in zip(a["tensors"][:6], b["tensors"][:6]):
        assert x.shape == y.shape and torch.equal(x, y)                   # bit-equal (no NaN can hide: torch.equal is false on NaN)
    assert a["digest"] == b["digest"], (a["digest"], b["digest"])
    assert a["keyframes"] == b["keyframes"] >= 1
    assert a["pipe"] == b["pipe"] and len(a["pipe"]) > 40, {k: (a["pipe"][k], b["pipe"].get(k)) for k in a["pipe"] if a["pipe"][k] != b["pipe"].get(k)}
    assert a["model"] == b["model"] and a["model"]["capacity"] == 4096 and a["model"]["opacities_lr"] == 0.05, (a["model"], b["model"])
    assert all(torch.equal(x, y) for x, y in zip(a["poses"], b["poses"]))
    assert not os.path.exists(ws)                                          # is_train = False: nothing created


def _ply_header(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    return raw[:end].decode().split("\n"), len(raw) - end


def _session_reader(h, seq, root):
    reader = h.DatasetReader()
    reader.loadConfig(root["READER"])
    _cameras(h, seq, reader)
    return reader


def test_train_save_then_evaluate_from_disk(seq, tmp_path):
    """Poses: with the cameras' c2w_slam handed over in memory the evaluation session reproduces the training session's
    eval_after_train renders byte for byte.  With the poses read back from val/pose/*.txt it cannot in general: six decimals are the
    reference's own format (saveTensorTXT), a pose read back from them differs from the estimate by up to 5e-7 per entry.  Measured
    on the MI355X for this sequence (LABBOOK.md section 25; the test prints them): 130 rgb_u8, 129 raycast_color_u8 and 15
    raycast_depth_u16 values of 110,592 per image kind differ, per-view PSNR by -2.8e-5 .. +8.9e-5 dB, the mean by +1.1e-5 dB.  The
    text-pose run is only asserted to complete and to render every view."""
    h = _host()
    ws = tmp_path / "ws"
    cfg = tmp_path / "office0.yaml"
    cfg.write_text(_yaml(seq, str(ws)))
    root = h.load_yaml(str(cfg))
    reader = _session_reader(h, seq, root)
    train = h.run_session(root, reader, str(cfg), False, SEED)
    assert train.work_mode == "train" and train.workspace_dir == str(ws) and train.gaussian_num > 100 and train.keyframe_count >= 1
    assert train.times.frames == N and train.times.slam_total > 0
    assert len(train.renders) == N and train.has_image_eval and len(train.image_eval.psnr) == N

    # what the session wrote
    gs = ws / "gs_model"
    pose_files = ["frame%06d.txt" % i for i in range(N)]
    assert sorted(os.listdir(ws / "val" / "pose")) == pose_files
    for f in ("cfg_args", "point_cloud/point_cloud.ply", "model.pt", "cameras.json"):
        assert (gs / f).is_file() and str(gs / f) in train.files, f
    for f in ("tsdf_engine/Scene/voxel.dat", "tsdf_engine/Scene/hash.dat", "tsdf_mesh.ply", "office0.yaml"):
        assert (ws / f).is_file() and os.path.getsize(ws / f) > 0, f
    for d in ("log", "val", "raycasted", "before_opt"):
        assert (ws / d).is_dir(), d
    assert open(ws / "office0.yaml").read() == cfg.read_text()
    assert open(gs / "cfg_args").read() == h.cfg_args_line(3)
    header, body = _ply_header(gs / "point_cloud" / "point_cloud.ply")
    golden, _ = _ply_header(os.path.join(ROOT, "tests", "golden", "gaussian_ply_n2_k16.ply"))
    assert golden[2] == "element vertex 2" and header[2] == "element vertex %d" % train.gaussian_num
    assert header[:2] + header[3:] == golden[:2] + golden[3:]
    assert body == train.gaussian_num * 4 * (len(header) - 5)             # one float per property and Gaussian, nothing else
    cams_json = json.load(open(gs / "cameras.json"))
    trained = reader.trainCameras()
    assert [c["id"] for c in cams_json] == list(range(N)) and [c["img_name"] for c in cams_json] == ["frame%06d.jpg" % i for i in range(N)]
    for c, cam in zip(cams_json, trained):
        got = np.array([r + [p] for r, p in zip(c["rotation"], c["position"])], np.float64).astype(np.float32)
        assert np.array_equal(got, cam.c2w_slam.numpy()[:3, :4]) and c["width"] == W and c["height"] == H
        assert open(ws / "val" / "pose" / ("frame%06d.txt" % cam.id)).read() == h.pose_txt(cam.c2w_slam)

    # a second session with fresh objects: work_mode eval, from disk
    cfg_eval = tmp_path / "office0_eval.yaml"
    cfg_eval.write_text(_yaml(seq, str(ws), "eval"))
    root_eval = h.load_yaml(str(cfg_eval))

    def evaluate(text_poses):
        r = _session_reader(h, seq, root_eval)
        if not text_poses:
            fresh = h.DatasetReader()
            fresh.loadConfig(root_eval["READER"])
            for cam, done in zip(r.trainCameras(), trained):
                cam.c2w_slam = done.c2w_slam.clone()              # the exact poses, handed over in memory
                fresh.addTrainCamera(cam)
            r = fresh
        before = sorted(os.listdir(ws))
        res = h.run_session(root_eval, r, "", text_poses, SEED)
        assert sorted(os.listdir(ws)) == before and res.files == []      # an evaluation writes nothing
        assert res.work_mode == "eval" and res.gaussian_num == train.gaussian_num and len(res.renders) == N
        return res, r

    mem, _ = evaluate(False)
    for i in range(N):
        for key in ("rgb_u8", "raycast_color_u8", "raycast_depth_u16", "gt_u8"):
            assert torch.equal(mem.renders[i][key], train.renders[i][key]), (i, key)
        assert torch.equal(mem.renders[i]["rgb"], train.renders[i]["rgb"])
    assert mem.has_image_eval and mem.image_eval.cam_ids == train.image_eval.cam_ids == list(range(N))
    assert mem.image_eval.psnr == train.image_eval.psnr and mem.image_eval.ssim == train.image_eval.ssim      # bit-equal doubles
    assert mem.image_eval.psnr_mean == train.image_eval.psnr_mean and mem.image_eval.ssim_mean == train.image_eval.ssim_mean
    assert all(np.isfinite(train.image_eval.psnr)) and min(train.image_eval.psnr) > 10.0

    txt, txt_reader = evaluate(True)
    for cam, done in zip(txt_reader.trainCameras(), trained):       # the reader's cameras carry the poses read back from val/pose/
        assert np.abs(cam.c2w_slam.numpy() - done.c2w_slam.numpy()).max() <= 5.0e-7 + 2.0 ** -23 * 4
        assert torch.equal(cam.c2w_slam, h.read_pose_txt(str(ws / "val" / "pose" / ("frame%06d.txt" % cam.id))))
    assert txt.has_image_eval and len(txt.image_eval.psnr) == N and all(np.isfinite(txt.image_eval.psnr))
    differing = {key: sum(int((txt.renders[i][key] != train.renders[i][key]).sum()) for i in range(N))
                 for key in ("rgb_u8", "raycast_color_u8", "raycast_depth_u16")}
    dpsnr = [a - b for a, b in zip(txt.image_eval.psnr, train.image_eval.psnr)]
    print("text poses against in-memory poses: differing values %s of %d per image kind; PSNR difference per view min %.3e max %.3e dB, mean %.3e dB"
          % (differing, N * W * H * 3, min(dpsnr), max(dpsnr), txt.image_eval.psnr_mean - train.image_eval.psnr_mean))
    for i in range(N):
        assert txt.renders[i]["rgb_u8"].shape == (H, W, 3) and txt.renders[i]["raycast_depth_u16"].shape[:2] == (H, W)


def test_recon_session_has_no_gaussians_and_saves_the_engine_only(seq, tmp_path):
    h = _host()
    ws = tmp_path / "ws"
    cfg = tmp_path / "office0.yaml"
    cfg.write_text(_yaml(seq, str(ws), "recon"))
    root = h.load_yaml(str(cfg))
    reader = _session_reader(h, seq, root)
    res = h.run_session(root, reader, str(cfg), False, SEED)
    assert res.work_mode == "recon" and res.gaussian_num == 0 and res.times.frames == N
    assert not res.has_image_eval and res.image_eval.psnr == []
    gs = ws / "gs_model"
    assert gs.is_dir() and os.listdir(gs) == []                            # save() returned at "empty model"
    assert (ws / "tsdf_engine" / "Scene" / "voxel.dat").is_file() and os.path.getsize(ws / "tsdf_mesh.ply") > 1000
    assert sorted(os.listdir(ws / "val" / "pose")) == ["frame%06d.txt" % i for i in range(N)]
    assert not any("gs_model" in f for f in res.files) and any(f.endswith("tsdf_mesh.ply") for f in res.files)
    # eval_after_train renders the TSDF's views alone
    assert len(res.renders) == N
    for r in res.renders:
        assert "rgb" not in r and "rgb_u8" not in r and r["raycast_color_u8"].shape == (H, W, 3) and r["raycast_depth_u16"].shape[:2] == (H, W)
    assert sum(int((r["raycast_depth_u16"] > 0).sum()) for r in res.renders) > N * W * H // 2
    # the same volume as a train session builds: the Gaussian block never writes the TSDF
    ws2 = tmp_path / "ws_train"
    cfg2 = tmp_path / "train.yaml"
    cfg2.write_text(_yaml(seq, str(ws2), "train"))
    root2 = h.load_yaml(str(cfg2))
    res2 = h.run_session(root2, _session_reader(h, seq, root2), str(cfg2), False, SEED)
    assert res2.gaussian_num > 100
    for name in ("voxel.dat", "hash.dat", "alloc.dat", "excess.dat"):
        assert _file_crc(ws / "tsdf_engine" / "Scene" / name) == _file_crc(ws2 / "tsdf_engine" / "Scene" / name), name
    for a, b in zip(res.renders, res2.renders):
        assert torch.equal(a["raycast_color_u8"], b["raycast_color_u8"]) and torch.equal(a["raycast_depth_u16"], b["raycast_depth_u16"])
