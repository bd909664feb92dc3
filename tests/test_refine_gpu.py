"""SLAMPipeline::gesTrainCams, the refinement pass over all keyframes once the sequence is over (host/slam_pipeline.hpp), on the
device: against a loop written here, against the Python mirror, the SH schedule, the optimiser state and the cache budget (the
session keys: tests/test_refine_session_gpu.py).

Shape: 64 x 48 images (4 x 3 tiles), 12 frames of the tests/synth orbit with given poses, 5 mm voxels and small hash tables, one
map update at frame 10 that keeps every masked pixel (new_gs_sample_ratio 1: about 500 Gaussians), sh_degree 3, and a keyframe
every second frame (the orbit turns 0.093 degrees per frame: keyframe_theta_thres 0.15)."""
import numpy as np
import pytest
import torch

from tests import digests, synth
from tests import test_session_gpu as S
from tests.test_refine_cpu import reference_rates

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, N, SEED = 64, 48, 12, 11
assert (S.W, S.H, S.N) == (W, H, N)
TSDF = dict(voxel_size=0.005, trunc_dist=0.02, viewFrustum_min=0.2, viewFrustum_max=10, use_gt_pose=1, sdf_local_block_num=0x4000,
            sdf_bucket_num=0x8000, sdf_excess_list_size=0x1000)
MODEL = dict(S.FLAT_MODEL, sh_degree_interval=2)
PIPE = dict(S.FLAT_PIPE, keyframe_theta_thres=0.15, new_gs_sample_ratio=1.0, scene_scale=float(np.float32(1.1) * np.float32(1.0)))
NAMES = ("getMeans", "getScales", "getQuats", "getFeaturesDc", "getFeaturesRest", "getOpacities")


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


class Scene:
    """one SLAM run; every test takes a fresh model with the run's parameters (the pipeline and the engine are shared)"""

    def __init__(self):
        h = self.h = _host()
        seq = synth.make_sequence(W, H, N, step_deg=0.5)
        reader = h.DatasetReader(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"])
        S._cameras(h, seq, reader)
        self.cli = h.createTsdfEngine(reader, TSDF)
        model = h.SLAMGaussianModel()
        model.loadConfig(MODEL)
        self.pipe = pipe = h.SLAMPipeline(SEED)
        pipe.setTsdfEngine(self.cli)
        pipe.loadConfig(PIPE)
        self.all_cams = pipe.SLAMTrainCamsModel(model, reader.trainCameras())     # host cameras with c2w_slam
        torch.cuda.synchronize()
        p = model.getGaussianParms()
        self.tensors = [getattr(p, n)().clone() for n in NAMES]
        self.cams = pipe.refineKeyframeCams()                                     # device cameras
        self.layers = [pipe.runRaycastByCam(c, False) for c in self.cams]
        self.keyframes = pipe.keyframeCount()
        c = self.cli.getMainEngine().counters().cpu()
        assert int(c[0]) > 0 and int(c[1]) > 0, "block array / excess list exhausted"

    def model(self, **extra):
        m = self.h.SLAMGaussianModel()
        m.loadConfig(dict(MODEL, **extra))
        m.getGaussianParms().add([t.clone() for t in self.tensors])
        self.pipe.setModel(m)
        self.pipe.curr_iter, self.pipe.selected_cam_idx, self.pipe.refine_lr_decay, self.pipe.refine_cache_mb = 0, -1, True, 16384
        return m


@pytest.fixture(scope="module")
def scene():
    sc = Scene()
    yield sc
    sc.cli.Shutdown()


def _params(m):
    torch.cuda.synchronize()
    p = m.getGaussianParms()
    return [getattr(p, n)().clone() for n in NAMES]


def _state(m):
    """the six parameter tensors, the twelve Adam moments, the step count and the means' rate"""
    return _params(m), [t.clone() for t in m.adamState()], m.adamStep(), m.meansLr()


def _assert_same_state(a, b, what):
    assert len(a[1]) == len(b[1]) == 12 and a[2] == b[2] and a[3] == b[3], (what, a[2], b[2], a[3], b[3])
    for k, (x, y) in enumerate(zip(a[0] + a[1], b[0] + b[1])):
        assert x.shape == y.shape and torch.equal(x, y), (what, k, float((x - y).abs().max()))


def _hand_loop(sc, m, n, seed, schedule=True, select=None):
    """gesTrainCams as the issue spells it: the selector's draws, updateSH, a trainStep WITHOUT next_cam, schedulersStep"""
    m.initOptimizers(n if schedule else -1, sc.pipe.scene_scale)
    sel = sc.h.RandomSelector(list(range(len(sc.cams))), seed)
    order = []
    for it in range(n):
        idx = sel.getNext()[1] if select is None else select
        order.append(idx)
        m.updateSH(it)
        L = sc.layers[idx]
        m.trainStep(sc.cams[idx], L["depth_map"], L["color_map"], L["depth_map_clamped"])
        m.schedulersStep()
    return order


def test_fixture_is_the_one_the_tests_name(scene):
    n = scene.tensors[0].shape[0]
    print("fixture: %d Gaussians, %d keyframes, %d cameras in the keyframes set" % (n, scene.keyframes, len(scene.cams)))
    assert 200 <= n <= 2000 and scene.keyframes >= 4 and len(scene.cams) >= scene.keyframes
    assert scene.tensors[4].shape[1:] == (15, 3)                          # sh_degree 3
    assert len({c.id for c in scene.cams}) == len(scene.cams)


def test_nine_iterations_equal_the_loop_written_here(scene):
    """pins the order of the draws, the run-ahead forward across the degree changes at iterations 2, 4 and 6 (the loop here never
    runs ahead) and the hand-over of the decayed rate"""
    a, b = scene.model(), None
    assert scene.pipe.gesTrainCams(scene.cams, 9, 5) == 9 and scene.pipe.curr_iter == 9
    got = _state(a)
    b = scene.model()
    order = _hand_loop(scene, b, 9, 5)
    assert len(set(order)) > 1
    _assert_same_state(got, _state(b), "gesTrainCams against the hand loop")
    assert a.degreesToUse == b.degreesToUse == 3 and got[2] == 9
    assert not torch.equal(got[0][0], scene.tensors[0])
    # caller-supplied base layers (the reference's file route): the same layers, the same result
    c = scene.model()
    assert scene.pipe.gesTrainCamsWithLayers(scene.cams, [dict(depth_map=L["depth_map"], color_map=L["color_map"]) for L in scene.layers], 9, 5) == 9
    _assert_same_state(got, _state(c), "caller-supplied base layers")
    # curr_iter is a member: a second call with the same count has nothing left to do
    assert scene.pipe.gesTrainCams(scene.cams, 9, 5) == 0
    log = scene.pipe.refineLog()
    assert log[-1][0] == 8 and np.isfinite(log[-1][1]) and log[-1][1] > 0


def test_python_mirror_is_bit_equal_to_the_cpp_host(scene):
    from gps_slam_amd.gs_model import Camera, SLAMGaussianModel
    from gps_slam_amd.slam_pipeline import SLAMPipeline
    a = scene.model()
    assert scene.pipe.gesTrainCams(scene.cams, 9, 5) == 9
    want = _state(a)
    pm = SLAMGaussianModel(dict(MODEL, fuse_sh_rest_adam=2), device=DEV)
    pm.add_params(dict(zip(("means", "scales", "quats", "featuresDc", "featuresRest", "opacities"), [t.clone() for t in scene.tensors])))
    pcams, differing = [], 0
    for c in scene.cams:
        pc = Camera(c.id, W, H, c.fx, c.fy, c.cx, c.cy, c.c2w.clone(), image=c.image, device=DEV)
        pc.c2w_slam = c.c2w_slam.clone()
        d = pc.toGPU()
        # (the two hosts invert the pose with different host arithmetic: the mirror gets the C++ camera's device pack, so that what is
        # compared is the loop)
        pack = torch.cat([c.viewmat().reshape(-1), c.K_dev().reshape(-1), c.cam_pos().reshape(-1)])
        differing += int((d["_pack"] != pack).sum())
        d["_pack"].copy_(pack)
        pcams.append(pc)
    print("camera packs: %d of %d floats differ between the hosts before the copy" % (differing, 28 * len(pcams)))
    pp = SLAMPipeline(None, pm, dict(scene_scale=scene.pipe.scene_scale), seed=SEED)
    layers = [dict(depth_map=L["depth_map"], color_map=L["color_map"]) for L in scene.layers]
    assert pp.gesTrainCams(pcams, 9, 5, base_layers=layers) == 9 and pp.curr_iter == 9
    torch.cuda.synchronize()
    N_ = pm.getGaussianNum()
    got = (list(pm.opt_gs_params.tensors()), [t[:N_] for t in pm._opt["m"]] + [t[:N_] for t in pm._opt["v"]], pm.adamStep(), pm.meansLr())
    _assert_same_state(want, got, "Python mirror against the C++ host")
    assert len(pp.refine_log) == 1 and pp.refine_log[0][0] == 8
    torch.testing.assert_close(pp.refine_log[0][1], scene.pipe.refineLog()[-1][1], rtol=1e-5, atol=0)


def test_sh_degree_grows_and_the_bases_above_it_stay_put(scene):
    """sh_degree_interval 2: degree 0 at iterations 0-1, 1 at 2-3, 2 at 4-5, 3 from 6 on.  While the degree in use is below 3 the
    featuresRest rows of the bases above it are bit-unchanged, their gradients are zero and their fresh moments are zero; at the
    first iteration of the next degree they move."""
    rest0 = scene.tensors[4]
    for n, live in ((2, 0), (3, 3), (4, 3), (5, 8), (6, 8), (7, 15)):       # iterations run -> featuresRest rows in use so far
        m = scene.model(fuse_sh_rest_adam=0)                                   # (the gradient reaches memory: grads()[4])
        assert scene.pipe.gesTrainCams(scene.cams, n, 5) == n
        torch.cuda.synchronize()
        rest = m.getGaussianParms().getFeaturesRest()
        st = m.adamState()
        assert torch.equal(rest[:, live:], rest0[:, live:]), n
        assert not st[4][:, live:].any() and not st[10][:, live:].any(), n     # exp_avg, exp_avg_sq of featuresRest
        assert not m.grads()[4][:, live:].any(), n
        assert m.degreesToUse == min(3, (n - 1) // 2)
        if live:
            newest = slice({3: 0, 8: 3, 15: 8}[live], live)                    # the bases of the degree reached last
            assert not torch.equal(rest[:, newest], rest0[:, newest]), n
            assert st[4][:, newest].any() and m.grads()[4][:, newest].any(), n
    # the fused featuresRest step (the default) leaves the same parameters
    a, b = scene.model(), scene.model(fuse_sh_rest_adam=0)
    scene.pipe.setModel(a)
    scene.pipe.curr_iter = 0
    scene.pipe.gesTrainCams(scene.cams, 5, 5)
    pa = _params(a)
    scene.pipe.setModel(b)
    scene.pipe.curr_iter = 0
    scene.pipe.gesTrainCams(scene.cams, 5, 5)
    for x, y in zip(pa, _params(b)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("n", [1, 7])
def test_one_optimiser_state_and_the_decayed_rate(scene, n):
    m = scene.model()
    assert scene.pipe.gesTrainCams(scene.cams, n, 3) == n
    assert m.adamStep() == n and m.hasScheduler()
    lr0 = float(np.float32(MODEL["means_lr"]) * np.float32(scene.pipe.scene_scale))
    assert m.meansLr() == reference_rates(lr0, n, n)[-1]
    assert abs(m.meansLr() / (0.01 * lr0) - 1.0) < 1e-6


def test_constant_rate_loop_equals_plain_train_steps(scene):
    """selected_cam_idx 0, no scheduler, sh_degree_interval 0: n iterations are n trainSteps on that camera after one initOptimizers"""
    n = 6
    a = scene.model(sh_degree_interval=0)
    scene.pipe.selected_cam_idx, scene.pipe.refine_lr_decay = 0, False
    assert scene.pipe.gesTrainCams(scene.cams, n, 5) == n
    got = _state(a)
    assert not a.hasScheduler()
    b = scene.model(sh_degree_interval=0)
    b.initOptimizers(-1, scene.pipe.scene_scale)
    L = scene.layers[0]
    for _ in range(n):
        b.trainStep(scene.cams[0], L["depth_map"], L["color_map"], L["depth_map_clamped"])
    _assert_same_state(got, _state(b), "constant-rate loop against plain steps")
    assert got[3] == float(np.float32(MODEL["means_lr"]) * np.float32(scene.pipe.scene_scale))


def _engine_digest(sc):
    torch.cuda.synchronize()
    t = sc.cli.getMainEngine().stateTensors()
    d = {k: digests.crc(t[k].cpu().numpy()) for k in ("vba", "hash", "visible_type", "visible_ids", "raycast", "depth", "icp_points")}
    d["counters"] = t["counters"].cpu()[:3].tolist()
    return d


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_refinement_raises_the_psnr_and_leaves_the_volume_alone(scene, seed):
    """a direction, not a number: mean PSNR of evalImages over the refined cameras, before and after 40 iterations"""
    scene.model(sh_degree_interval=0)
    volume = _engine_digest(scene)
    before = scene.pipe.evalImages(scene.cams).psnr_mean
    assert scene.pipe.gesTrainCams(scene.cams, 40, seed) == 40
    after = scene.pipe.evalImages(scene.cams).psnr_mean
    print("seed %d: mean PSNR over %d cameras %.3f dB -> %.3f dB after 40 iterations" % (seed, len(scene.cams), before, after))
    assert after > before, (before, after)
    assert _engine_digest(scene) == volume


def test_cache_budget_is_checked_before_anything_is_allocated(scene):
    m = scene.model()
    scene.pipe.refine_cache_mb = 1
    assert scene.pipe.refineCacheBytes(scene.all_cams) == N * W * H * 9 * 4 > 1 << 20
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match=r"12 cameras need 2 MiB on the device, refine_cache_mb allows 1"):
        scene.pipe.gesTrainCams(scene.all_cams, 5, 5)
    assert torch.cuda.memory_allocated() == allocated and scene.pipe.curr_iter == 0
    assert all(torch.equal(x, y) for x, y in zip(_params(m), scene.tensors))
    # the model and the pipeline remain usable
    m.initOptimizers(-1, scene.pipe.scene_scale)
    L = scene.layers[0]
    m.trainStep(scene.cams[0], L["depth_map"], L["color_map"], L["depth_map_clamped"])
    assert not torch.equal(_params(m)[0], scene.tensors[0])
    scene.pipe.refine_cache_mb = 16384
    assert scene.pipe.gesTrainCams(scene.all_cams, 2, 5) == 2                  # host cameras (refine_cams: all) go to the device inside
