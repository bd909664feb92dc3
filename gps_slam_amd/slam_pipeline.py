"""Host-side mirror of SLAMPipeline (slam/slam_pipeline.{h,cpp}): the per-frame loop that drives the hot path.

    SLAMTrainCams      :52-173   per frame: TSDF ProcessFrame; every local_opt_interval frames:
    localFrameRaycast  :417-448  runRaycastByCam for the <= 2 window frames
    keyFrameRaycast    :528-561  + <= 7 random keyframes
    initNewGaussians   :450-526  error-mask sampling -> addGaussians
    localOptimize      :195-289  20 x (forward, L1, backward, 7 x Adam)
    removeRedundantGs  :564-586  prune by scale / opacity

All compute goes through the C-ABI (gs_model.py, tsdf_engine.py); this file is bookkeeping.  Random choices the
reference seeds from std::random_device (dataset_reader.h:39) are seeded here so runs are reproducible.
"""
import ctypes as C
import math
import random

import numpy as np
import torch

from ._lib import check, lib
from .gs_model import Camera, SLAMGaussianModel, pose_inv  # noqa: F401
from . import random_selector

DEFAULT_PIPE = dict(new_gs_sample_ratio=0.25, color_error_thres=0.05, localframe_cam_window_length=2,
                    localframe_cam_window_interval=5, local_opt_iters=20, local_opt_interval=10,
                    keyframe_theta_thres=30.0, keyframe_trans_thres=0.3, keyframe_select_max=7,
                    depth_vis_max=5.0, depth_vis_min=0.0, alpha_vis_max=5.0, large_scale_thres=0.1,
                    small_scale_thres=0.003, low_opac_thres=0.005, scene_scale=1.1 * 3.0)


class RandomSelector:
    """dataset_reader.h:26-100 (uniform branch): draw without replacement, refill when exhausted."""

    def __init__(self, items, rng):
        self.original = list(enumerate(items))
        self.current = list(self.original)
        self.rng = rng

    def getNext(self):
        if not self.current:
            self.current = list(self.original)
        i = self.rng.randrange(len(self.current))
        v = self.current[i]
        self.current[i] = self.current[-1]
        self.current.pop()
        return v  # (originalIndex, value)


def compute_normal_map(vertex_map):
    """computeNormalMap (tensor_math.cpp:278-300) -> gps_normal_map"""
    H, W, _ = vertex_map.shape
    vertex_map = vertex_map.contiguous()
    out = torch.empty_like(vertex_map)
    check(lib.gps_normal_map(W, H, vertex_map.data_ptr(), out.data_ptr(),
                             C.c_void_p(torch.cuda.current_stream(vertex_map.device).cuda_stream)), "gps_normal_map")
    return out


class SLAMPipeline:
    def __init__(self, tsdf_engine, model, pipe_cfg=None, seed=1234, work_mode="train", use_gt_pose=True):
        self.tsdf = tsdf_engine
        self.model = model
        self.cfg = dict(DEFAULT_PIPE)
        self.cfg.update(pipe_cfg or {})
        self.work_mode = work_mode
        # TSDF.use_gt_pose of the configs (true in every shipped one; createTsdfEngine then calls turnOffTracking,
        # InfiniTAM_tools.cpp:59-62); False keeps the depth-only ExtendedTracker active
        self.use_gt_pose = use_gt_pose
        if not use_gt_pose and not hasattr(tsdf_engine, "track_cfg"):
            tsdf_engine.turnOnTracking()
        self.rng = random.Random(seed)
        self.gen = torch.Generator().manual_seed(seed)  # host generator (see SLAMGaussianModel.addGaussians)
        self.device = model.device
        self.localframe_cam_window = []
        self.localframe_raycast_window = []
        self.keyframe_cam_list = []
        self.opt_cam_list, self.opt_raycast_list = [], []
        self.curr_frame_id = 0
        self.curr_cam = None
        self.stats = dict(frames=0, opt_iters=0, raycasts=0, added=0, pruned=0)
        self.workspace_dir, self.saved_mesh, self.saved_engine = ".", "", ""
        self.gtC2wPoses = []  # dataset pose of every processed frame (ITMBasicEngine::gtC2wPoses), for evalTrajectory
        # Pipeline::loadConfig's session settings gesTrainCams reads (src/pipeline.cpp:9-22) and this project's refine_* keys
        self.max_iterations, self.selected_cam_idx, self.log_iter = 10000, -1, 1000
        self.refine_iterations, self.refine_cams, self.refine_seed, self.refine_cache_mb = 0, "keyframes", seed, 16384
        self.refine_lr_decay = True   # False: gesTrainCams builds its optimisers without the scheduler (constant rates)
        self.curr_iter = 0
        self.refine_log = []   # (iter, loss) every log_iter iterations of gesTrainCams and at the last one

    @classmethod
    def from_config(cls, nested, tsdf_engine, model, seed=1234):
        """The pipeline as slam_trainer.cpp:26-41 sets it up from a config file: `nested` is what config.load_yaml returns.
        PIPE (with its nested sections folded, config.flatten) -> pipe_cfg; the root's work_mode and workspace_dir;
        scene_scale = 1.1 x READER.scene_scale (dataset_reader.cpp:231); TSDF.use_gt_pose, saved_mesh, saved_engine."""
        from . import config
        flat = config.flatten(nested["PIPE"], config.PIPE_KEYS)
        if flat["enable_densify"]:
            raise config.ConfigError("PIPE.enable_densify: densification is not supported (set it to false)")
        if flat["sample_method"] not in ("random", "ours"):
            raise config.ConfigError("PIPE.keyframe_sample_configs.sample_method: 'random' or 'ours', got '%s'" % flat["sample_method"])
        pipe_cfg = {k: flat[k] for k in DEFAULT_PIPE if k in flat}
        pipe_cfg["scene_scale"] = float(np.float32(1.1) * np.float32(nested["READER"]["scene_scale"].as_float()))
        pipe = cls(tsdf_engine, model, pipe_cfg, seed=seed, work_mode=nested["work_mode"].as_str(), use_gt_pose=flat["use_gt_pose"])
        pipe.workspace_dir = nested["workspace_dir"].as_str()
        pipe.saved_mesh, pipe.saved_engine = flat["saved_mesh"], flat["saved_engine"]
        pipe.max_iterations, pipe.selected_cam_idx, pipe.log_iter = flat["max_iterations"], flat["selected_cam_idx"], flat["log_iter"]
        if pipe.log_iter == -1:
            pipe.log_iter = pipe.max_iterations - 1   # src/pipeline.cpp:17-18
        refine = config.refine_settings(nested["PIPE"])
        pipe.refine_iterations, pipe.refine_cams, pipe.refine_cache_mb = refine["refine_iterations"], refine["refine_cams"], refine["refine_cache_mb"]
        if refine["refine_seed"] is not None:
            pipe.refine_seed = refine["refine_seed"]
        return pipe

    # ------------------------------------------------------------------ slam_pipeline.h:32-49
    def saveMesh(self):
        if self.saved_mesh:
            self.tsdf.SaveSceneToMesh(self.workspace_dir + "/" + self.saved_mesh)

    def saveEngine(self):
        if self.saved_engine:
            self.tsdf.SaveToFile(self.workspace_dir + "/" + self.saved_engine)

    def loadEngine(self):
        self.tsdf.LoadFromFile(self.workspace_dir + "/" + self.saved_engine)

    # ------------------------------------------------------------------ evaluation (scripts/geo_general.py, ate_general.py)
    def evalGeometry(self, gt_points_or_triangles, **kw):
        """TsdfEngine.EvalMesh of the attached engine (this pipeline runs its updates inline: nothing to flush)"""
        if self.tsdf is None:
            raise RuntimeError("evalGeometry: no TSDF engine attached")
        return self.tsdf.EvalMesh(gt_points_or_triangles, **kw)

    def evalTrajectory(self):
        """geom_eval.ate of the engine's stored per-frame poses (camPoses: GetInvM) against the dataset poses of the same frames"""
        from . import geom_eval
        if self.tsdf is None:
            raise RuntimeError("evalTrajectory: no TSDF engine attached")
        est = [np.asarray(invM, np.float64).reshape(4, 4).T for _, invM in self.tsdf.camPoses]   # ORUtils layout -> row-major
        if len(est) != len(self.gtC2wPoses):
            raise ValueError("evalTrajectory: %d stored poses against %d ground-truth poses" % (len(est), len(self.gtC2wPoses)))
        if len(est) < 3:
            raise ValueError("evalTrajectory: at least three frames are needed")
        return geom_eval.ate(np.stack(est), np.stack(self.gtC2wPoses))

    # ------------------------------------------------------------------ raycast -> tensors (runRaycastByCam :362-415)
    def runRaycastByCam(self, cam):
        eng = self.tsdf
        if 0 <= cam.id < len(eng.camPoses):
            pose = eng.camPoses[cam.id]
            eng.runRaycast(pose=pose)
        else:
            eng.runRaycast(c2w=cam.c2w.numpy())
        H, W = cam.height, cam.width
        d = self.device
        color = torch.empty((H, W, 3), device=d)
        vertex = torch.empty((H, W, 3), device=d)
        conf = torch.empty((H, W, 1), device=d)
        depth = torch.empty((H, W, 1), device=d)
        depth_c = torch.empty((H, W, 1), device=d)
        w2c = np.ascontiguousarray(pose_inv(cam.c2w).numpy().astype(np.float32))  # poseInv(cam.c2w): dataset pose (:398)
        check(lib.gps_raycast_to_maps(W, H, eng.fv_raycast.data_ptr(), eng.fv_colour.data_ptr(), eng.getVoxelSize(),
                                      w2c.ctypes.data, color.data_ptr(), vertex.data_ptr(), conf.data_ptr(),
                                      depth.data_ptr(), depth_c.data_ptr(),
                                      C.c_void_p(torch.cuda.current_stream(d).cuda_stream)),
              "gps_raycast_to_maps")
        self.stats["raycasts"] += 1
        return dict(color_map=color, vertex_map=vertex, confidence_map=conf, depth_map=depth,
                    depth_map_clamped=depth_c)

    # ------------------------------------------------------------------ frame bookkeeping (updateFrameList :319-360)
    def updateFrameList(self):
        c = self.cfg
        if self.curr_frame_id == 0:
            return
        if self.curr_frame_id % c["localframe_cam_window_interval"] == 0:
            self.localframe_cam_window.append(self.curr_cam)
            if len(self.localframe_cam_window) == c["localframe_cam_window_length"] + 1:
                self.localframe_cam_window.pop(0)
        is_key = False
        if not self.keyframe_cam_list:
            is_key = True
        else:
            last = self.keyframe_cam_list[-1]
            Rp, Rc = last.c2w_slam[:3, :3], self.curr_cam.c2w_slam[:3, :3]
            cos_t = float((torch.trace(Rp.t() @ Rc) - 1) / 2)
            theta = math.degrees(math.acos(max(-1.0, min(1.0, cos_t))))
            trans = float(torch.norm(last.c2w_slam[:3, 3] - self.curr_cam.c2w_slam[:3, 3]))
            is_key = theta > c["keyframe_theta_thres"] or trans > c["keyframe_trans_thres"]
        if is_key:
            self.keyframe_cam_list.append(self.curr_cam)

    def localFrameRaycast(self):
        self.localframe_raycast_window = [self.runRaycastByCam(cam) for cam in self.localframe_cam_window]

    def keyFrameRaycast(self):
        self.opt_cam_list = list(self.localframe_cam_window)
        self.opt_raycast_list = list(self.localframe_raycast_window)
        n = min(self.cfg["keyframe_select_max"], len(self.keyframe_cam_list))
        sel = RandomSelector(self.keyframe_cam_list, self.rng)
        for _ in range(n):
            _, cam = sel.getNext()
            self.opt_cam_list.append(cam)
            self.opt_raycast_list.append(self.runRaycastByCam(cam))

    # ------------------------------------------------------------------ initNewGaussians :450-526
    def initNewGaussians(self, raycast_maps):
        c, model, cam = self.cfg, self.model, self.curr_cam
        depth, color, vertex = raycast_maps["depth_map"], raycast_maps["color_map"], raycast_maps["vertex_map"]
        frame_num = c["local_opt_interval"]
        valid = (depth > c["depth_vis_min"]) & (depth < c["depth_vis_max"])
        valid = valid & ~((vertex.sum(2) == 0).unsqueeze(-1))
        if model.getGaussianNum() == 0:
            err = torch.mean(torch.abs(color - cam.image), -1, True)
            mask = (err > c["color_error_thres"]) & valid
            frame_num += 1
        else:
            res = model.forward(cam, depth, color)
            err = torch.mean(torch.abs(res["rgb"] - cam.image), -1, True)
            mask = (err > c["color_error_thres"]) & valid & (res["alpha"] < c["alpha_vis_max"])
        raycast_maps["normal_map"] = compute_normal_map(vertex)
        n = model.addGaussians(cam, raycast_maps, mask, c["new_gs_sample_ratio"], frame_num, generator=self.gen)
        self.stats["added"] += n

    # ------------------------------------------------------------------ localOptimize :195-289
    def localOptimize(self):
        model = self.model
        if model.getGaussianNum() == 0:
            return
        model.initOptimizers(-1, self.cfg["scene_scale"])
        loader = RandomSelector(self.opt_cam_list, self.rng)
        for _ in range(self.cfg["local_opt_iters"]):
            idx, cam = loader.getNext()
            self._optimize_one(cam, self.opt_raycast_list[idx])

    def _optimize_one(self, cam, rc, next_cam=None):
        """one optimise iteration on `cam` over its base layers: THE iteration body of localOptimize and of gesTrainCams"""
        self.model.train_step(cam, rc["depth_map"], rc["color_map"], cam.image, ref_depth_clamped=rc["depth_map_clamped"],
                              next_cam=next_cam)
        self.stats["opt_iters"] += 1

    # ------------------------------------------------------------------ gesTrainCams (src/pipeline.cpp:229-319)
    def refineKeyframeCams(self):
        """the "keyframes" set of refine_cams: keyframe_cam_list plus the live window (a camera in both counts once)"""
        out = list(self.keyframe_cam_list)
        out += [w for w in self.localframe_cam_window if all(k.id != w.id for k in out)]
        return out

    @staticmethod
    def refineCacheBytes(cams):
        """per pixel: colour 3 + depth 1 + clamped depth 1 floats of the base layers, 3 (+ 1 with a depth) of the camera's images"""
        return sum(c.width * c.height * (3 + 1 + 1 + 3 + (1 if c.depth is not None else 0)) * 4 for c in cams)

    def gesTrainCams(self, cams, max_iterations=-1, seed=-1, base_layers=None):
        """Mirror of SLAMPipeline::gesTrainCams (host/slam_pipeline.hpp): the pass over all of `cams` once the sequence is over,
        with ONE optimiser state, the means' rate decaying to 0.01 x its start and the SH degree growing by sh_degree_interval.
        Base layers: each camera's free view of the engine's final volume, or `base_layers` (one dict with depth_map and
        color_map per camera).  -> the number of iterations run."""
        model = self.model
        if not cams:
            raise ValueError("gesTrainCams: no cameras")
        need = self.refineCacheBytes(cams)
        if need > self.refine_cache_mb << 20:
            raise RuntimeError("gesTrainCams: the base layers and images of %d cameras need %d MiB on the device, refine_cache_mb allows %d"
                               % (len(cams), (need + (1 << 20) - 1) >> 20, self.refine_cache_mb))
        for cam in cams:
            cam.toGPU()
        if base_layers is None:
            layers = []
            for cam in cams:
                m = self.runRaycastByCam(cam)
                layers.append({k: m[k] for k in ("color_map", "depth_map", "depth_map_clamped")})
        else:
            if len(base_layers) != len(cams):
                raise ValueError("gesTrainCams: %d base layers for %d cameras" % (len(base_layers), len(cams)))
            layers = [dict(color_map=b["color_map"].to(self.device, torch.float32).contiguous(),
                           depth_map=b["depth_map"].to(self.device, torch.float32).contiguous()) for b in base_layers]
            for b in layers:
                b["depth_map_clamped"] = model.clamp_ref_depth(b["depth_map"])
        if max_iterations < 0:
            max_iterations = self.max_iterations
        if seed < 0:
            seed = self.refine_seed
        if not -1 <= self.selected_cam_idx < len(cams):
            raise ValueError("gesTrainCams: selected_cam_idx %d with %d cameras" % (self.selected_cam_idx, len(cams)))
        if self.curr_iter >= max_iterations or model.getGaussianNum() == 0:
            return 0
        model.initOptimizers(max_iterations if self.refine_lr_decay else -1, self.cfg["scene_scale"])
        loader = random_selector.RandomSelector(cams, seed)
        draw = (lambda: loader.getNext()[1]) if self.selected_cam_idx == -1 else (lambda: self.selected_cam_idx)
        if model._B is not None:
            model.loss_sum().zero_()
        first, since_log, nxt = self.curr_iter, 0, None
        while self.curr_iter < max_iterations:
            idx = draw() if nxt is None else nxt
            nxt = draw() if self.curr_iter + 1 < max_iterations else None   # one iteration early: the same draws in the same order
            model.updateSH(self.curr_iter)
            self._optimize_one(cams[idx], layers[idx], None if nxt is None else cams[nxt])
            model.schedulersStep()
            since_log += 1
            last = self.curr_iter + 1 == max_iterations
            if last or (self.log_iter > 0 and (self.curr_iter + 1) % self.log_iter == 0):
                self.refine_log.append((self.curr_iter, float(model.loss_sum()) / since_log))
                model.loss_sum().zero_()
                since_log = 0
                model.check_binning_capacity()
            self.curr_iter += 1
        return self.curr_iter - first

    # ------------------------------------------------------------------ removeRedundantGs :564-586
    def removeRedundantGs(self):
        model, c = self.model, self.cfg
        if model.getGaussianNum() == 0:
            return
        smax = model.getRealScales().max(-1).values
        mask = (smax < c["small_scale_thres"]) | (smax > c["large_scale_thres"]) | \
               (model.getRealOpacities().squeeze(-1) < c["low_opac_thres"])
        n = int(mask.sum())  # the reference syncs 5 times here for its printf; once is enough
        model.check_binning_capacity()  # the host is synchronised here anyway: read the kernels' sticky overflow flag
        if n > 0:
            model.prunePoints(mask)
            self.stats["pruned"] += n

    # ------------------------------------------------------------------ one SLAM frame (body of SLAMTrainCams :69-132)
    def process_frame(self, i, cam, rgb_u8_dev, depth_mm_dev):
        self.curr_frame_id = i
        if self.use_gt_pose:
            M, invM = self.tsdf.ProcessFrame(rgb_u8_dev, depth_mm_dev, cam.c2w.numpy())
        else:
            M, invM = self.tsdf.ProcessFrameTracked(rgb_u8_dev, depth_mm_dev)
        self.gtC2wPoses.append(np.asarray(cam.c2w.numpy(), np.float64).copy())
        # est_pose = pose_d->GetInvM() (:81-82): ORUtils layout -> row-major tensor
        cam.c2w_slam = torch.from_numpy(invM.reshape(4, 4).T.copy())
        cam.invalidate()
        self.curr_cam = cam
        cam.toGPU()
        self.updateFrameList()
        self.stats["frames"] += 1
        if self.work_mode == "recon":
            return
        if i % self.cfg["local_opt_interval"] == 0 and i > 0:
            self.localFrameRaycast()
            self.keyFrameRaycast()
            self.initNewGaussians(self.localframe_raycast_window[-1])
            self.localOptimize()
            self.removeRedundantGs()
