"""SLAMPipeline::rawTrainCams, the classic 3DGS trainer with densification (host/slam_pipeline.hpp), on the device.

Shape: 64 x 48 images, three cameras of the tests/synth orbit (4 degrees apart), about 500 Gaussians back-projected from the
first camera's depth at every sixth pixel with scales and opacities spread so that every class of densifiyGs occurs; 30
iterations with densify_interval 10 and densify_start_iter 5 (events at iterations 10 and 20), reset_opacity_interval 15 (resets
at 0 and 15; the scale criterion of the prune is off at the first event and on at the second).  The thresholds are the
pair of a small grid around (0.002, 0.03) that leaves the decisions of both events furthest from their thresholds (1.5e-3
relative, against the 1e-4 the comparison with float64 needs).

The loop is written once more here from the bound pieces (`hand_loop`): it snapshots the statistics and the model in front of
every densification, runs the float64 oracle of tests/densify_cases.py on the snapshot and compares the model behind the call as
tests/test_densify_gpu.py does.  rawTrainCams itself must then end bit-identical to that loop, and to its own second run.

That needs a rasterizer backward whose sums have a fixed order: gps_raster_raw_bwd accumulates with float atomics and two runs
through it part in the last bits from the second iteration on (after 30 iterations up to 1.1e-06 per parameter, with or without
densification).  rawTrainCams therefore runs the model with ordered_raw_backward (gps_raster_raw_bwd_ordered), and so does the
loop here."""
import numpy as np
import pytest
import torch

from tests import densify_cases as dc
from tests import synth
from tests.test_densify_gpu import DEV, T, _host, check_model, model_arrays

pytestmark = pytest.mark.gpu
W, H, SEED, ITERS = 64, 48, 5, 30
SCENE_SCALE = 4.0
MODEL = dict(render_method="raw", capacity=4096, sh_degree=3, sh_degree_interval=4, densify_start_iter=5, densify_end_iter=1000,
             densify_interval=10, reset_opacity_interval=15, densify_grad_thres=0.0022, densify_large_thres=0.03,
             prune_opacity_thres=0.2)
EVENTS = (10, 20)


class Scene:
    def __init__(self):
        h = self.h = _host()
        seq = synth.make_sequence(W, H, 3, step_deg=4.0)
        self.cams = []
        for i in range(3):
            c = h.Camera(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], True, torch.as_tensor(seq["c2w"][i].astype(np.float32)))
            c.id = i
            c.image = torch.as_tensor(seq["rgb"][i].astype(np.float32) / 255.0).to(DEV)
            self.cams.append(c)
        # Gaussians from camera 0's depth at every sixth pixel
        rng = np.random.default_rng(SEED)
        depth = seq["depth"][0].astype(np.float64) / 1000.0
        ys, xs = np.divmod(np.arange(0, W * H, 6), W)
        d = depth[ys, xs]
        ok = d > 0
        ys, xs, d = ys[ok], xs[ok], d[ok]
        pc = np.stack([(xs - seq["cx"]) / seq["fx"] * d, (ys - seq["cy"]) / seq["fy"] * d, d], -1)
        c2w = seq["c2w"][0].astype(np.float64)
        n = len(d)
        means = pc @ c2w[:3, :3].T + c2w[:3, 3]
        factor = rng.uniform(0.5, 2.5, n)
        factor[rng.random(n) < 0.05] *= 5.0                                     # a few huge ones for the scale criterion
        scales = (d / seq["fx"] * factor)[:, None] * rng.uniform(0.5, 1.0, (n, 3))
        quats = rng.normal(size=(n, 4))
        rgb = seq["rgb"][0][ys, xs].astype(np.float64) / 255.0
        opac = rng.uniform(0.1, 0.9, n)
        f32 = np.float32
        self.tensors = [T(means.astype(f32)), T(np.log(scales).astype(f32)), T(quats.astype(f32)), T(((rgb - 0.5) / 0.28209479177387814).astype(f32)),
                        T(np.zeros((n, 15, 3), f32)), T(np.log(opac / (1 - opac)).astype(f32)[:, None])]
        self.pipe = h.SLAMPipeline(SEED)
        self.pipe.scene_scale = SCENE_SCALE

    def model(self, **extra):
        m = self.h.SLAMGaussianModel()
        m.loadConfig(dict(MODEL, **extra))
        m.getGaussianParms().add([t.clone() for t in self.tensors])
        self.pipe.setModel(m)
        self.pipe.curr_iter, self.pipe.selected_cam_idx = 0, -1
        return m


@pytest.fixture(scope="module")
def scene():
    return Scene()


def _state(m):
    params, mm, vv = model_arrays(m)
    return params + mm + vv, m.adamStep(), m.meansLr(), m.getGaussianNum()


def _same(a, b, what):
    assert a[1:] == b[1:], (what, a[1:], b[1:])
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        assert x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)), (what, k)


def hand_loop(sc, m, n, seed, densify=True, observe=None):
    """rawTrainCams from the bound pieces; at a densification the pieces of stepPostBackward one by one, with `observe` around
    densifiyGs"""
    m.initOptimizers(n, SCENE_SCALE)
    m.setDensifySeed(seed)
    m.ordered_raw_backward = True             # as rawTrainCams runs it: the rasterizer's backward without float atomics
    sel = sc.h.RandomSelector(list(range(len(sc.cams))), seed)
    losses = []
    for it in range(n):
        cam = sc.cams[sel.getNext()[1]]
        m.updateSH(it)
        res = m.rawForward(cam)
        if densify:
            res["means2d"].retain_grad()
        loss = m.computeLoss(res, cam, dict(ssim_weight=0.0, depth_weight=0.0))
        loss["total"].backward()
        losses.append(float(loss["total"].detach()))
        m.optimizersStep()
        m.optimizersZeroGrad()
        if densify:
            due = it % m.densify_interval == 0 and it > m.densify_start_iter and it < m.densify_end_iter
            if not due:
                m.stepPostBackward(res, cam, SCENE_SCALE, it)
            else:
                m.updateDensifyGrad(res, cam)
                before = observe("before", it, None) if observe else None
                counts = m.densifiyGs(SCENE_SCALE, it)
                if observe:
                    observe("after", it, (before, counts))
                for t in m.densifyStats():
                    t.zero_()
                if it % m.reset_opacity_interval == 0:
                    m.resetOpacities()
        m.schedulersStep()
        if observe:
            observe("end", it, None)
    return losses


def _thresholds(m, it):
    f = np.float32
    prune_scale = float(f(0.1) * f(SCENE_SCALE)) if it > m.reset_opacity_interval else float("inf")
    return float(f(m.densify_grad_thres)), float(f(m.densify_large_thres) * f(SCENE_SCALE)), float(f(m.prune_opacity_thres)), prune_scale


def test_fixture_is_the_one_the_tests_name(scene):
    n = scene.tensors[0].shape[0]
    assert 400 <= n <= 600 and len(scene.cams) == 3 and scene.tensors[4].shape[1:] == (15, 3)


def test_every_densification_against_the_oracle_and_the_loop_against_raw_train_cams(scene):
    m = scene.model()
    n0 = m.getGaussianNum()
    seen = {}

    def observe(when, it, extra):
        if when == "before":
            params, mm, vv = model_arrays(m)
            gs, vc = [t.cpu().numpy() for t in m.densifyStats()]
            return params, mm, vv, gs, vc
        if when == "after":
            (params, mm, vv, gs, vc), counts = extra
            z = m.lastSplitSamples()
            case = dc.case_from_arrays("iteration %d" % it, params, mm, vv, gs, vc, *_thresholds(m, it),
                                       samples=None if z is None else z.cpu().numpy())
            margins = dc.margin_report(case)
            print("iteration %d: %d Gaussians, %d rows seen, margins %s" % (it, case.N, int((vc > 0).sum()), margins))
            assert dc.check_margins(case), margins                    # every row is one float64 decides as float32 does
            exp = dc.oracle_index(case, case.sample_pool[:2 * int(counts[1])] if len(counts) else None)
            print("iteration %d: counts %s (M, n_split, n_split_surviving, n_dup_surviving, n_keep)" % (it, exp.counts.tolist()))
            assert counts == exp.counts.tolist() and m.getGaussianNum() == exp.M
            M, n_split, n_ss, n_ds, n_keep = exp.counts.tolist()
            # each class occurs: clones, split parents with surviving children, kept rows, pruned rows that were no split parent
            assert n_ds > 0 and n_ss > 0 and n_keep > 0 and n_keep + n_split < case.N, exp.counts.tolist()
            if np.isfinite(case.prune_scale):
                off = dc.oracle_index(dc.case_from_arrays("", params, mm, vv, gs, vc, *_thresholds(m, it)[:3], float("inf"), case.sample_pool))
                assert off.counts[4] > n_keep                               # the scale criterion prunes rows of its own
            check_model(case, exp, *model_arrays(m), what="iteration %d" % it)
            seen[it] = dict(exp=exp, after=model_arrays(m))
        if when == "end" and it - 1 in seen and "next" not in seen[it - 1]:
            seen[it - 1]["next"] = model_arrays(m)

    losses = hand_loop(scene, m, ITERS, SEED, observe=observe)
    assert sorted(seen) == list(EVENTS)
    assert m.getGaussianNum() == seen[EVENTS[-1]]["exp"].M != n0 and m.adamStep() == ITERS
    assert m.opacity_reset_log == [0, 15] and m.densify_log == []          # (the loop here ran the densifications' pieces itself)
    # the step behind an event moves the new rows, and their moments leave zero
    for it in EVENTS:
        exp, (p0, m0, v0), (p1, m1, v1) = seen[it]["exp"], seen[it]["after"], seen[it]["next"]
        new = exp.kind != 0
        assert new.sum() > 10
        for k in (0, 1, 3, 5):
            moved = (p1[k][new] != p0[k][new]).reshape(int(new.sum()), -1).any(1)
            assert moved.sum() > 0.5 * new.sum(), (it, k, int(moved.sum()), int(new.sum()))
            assert not m0[k][new].any() and m1[k][new].any() and v1[k][new].any()
    # the opacity reset at iteration 0 (0 % k == 0, the reference's behaviour): seen through a one-iteration run
    one = scene.model()
    hand_loop(scene, one, 1, SEED)
    top = float(torch.logit(torch.tensor(np.float32(2) * np.float32(MODEL["prune_opacity_thres"]))))
    op = model_arrays(one)[0][5]
    assert op.max() <= np.float32(top) and (op == np.float32(top)).sum() > 50 and float(scene.tensors[5].max()) > top
    assert one.opacity_reset_log == [0]
    # rawTrainCams is that loop: the same schedule with the same counts, the same optimiser bookkeeping, the same bits
    a = scene.model()
    scene.pipe.log_iter = 10
    try:
        first = len(scene.pipe.refineLog())
        assert scene.pipe.rawTrainCams(scene.cams, ITERS, SEED, True) == ITERS and scene.pipe.curr_iter == ITERS
        log = scene.pipe.refineLog()[first:]
    finally:
        scene.pipe.log_iter = 1000
    assert a.densify_log == [[it] + seen[it]["exp"].counts.tolist() for it in EVENTS], a.densify_log
    assert a.opacity_reset_log == [0, 15] and a.densify_events == 2
    assert (a.getGaussianNum(), a.adamStep(), a.meansLr(), a.degreesToUse) == (m.getGaussianNum(), ITERS, m.meansLr(), m.degreesToUse)
    _losses_agree(log, losses)
    _same(_state(a), _state(m), "rawTrainCams against the loop written here")
    assert a.ordered_raw_backward is False                                   # (the trainer's switch is its own)
    assert scene.pipe.rawTrainCams(scene.cams, ITERS, SEED, True) == 0       # curr_iter is a member: nothing left to do
    # another seed: other cameras, other samples
    c = scene.model()
    assert scene.pipe.rawTrainCams(scene.cams, ITERS, SEED + 1, True) == ITERS
    assert c.getGaussianNum() != a.getGaussianNum() or not np.array_equal(model_arrays(c)[0][0], model_arrays(a)[0][0])


def _losses_agree(log, losses):
    """the logged losses are the loop's, to the bit (both are float32 read back from the same computation)"""
    assert [e[0] for e in log] == [9, 19, 29]
    for it, value in log:
        assert np.isfinite(value) and value > 0 and value == losses[it], (it, value, losses[it])


def test_two_runs_with_one_seed_end_bit_identical(scene):
    """parameters, both moments, the step count, the rate and the Gaussian count after 30 iterations with two densifications; and
    the same without densification"""
    a = scene.model()
    assert scene.pipe.rawTrainCams(scene.cams, ITERS, SEED, True) == ITERS
    got = _state(a)
    b = scene.model()
    assert scene.pipe.rawTrainCams(scene.cams, ITERS, SEED, True) == ITERS
    again = _state(b)
    for k, (x, y) in enumerate(zip(got[0], again[0])):
        if x.shape == y.shape and x.size:
            print("tensor %d: largest difference between the two runs %.3g" % (k, float(np.abs(x.astype(np.float64) - y).max())))
    _same(again, got, "two runs with one seed")
    assert got[3] != scene.tensors[0].shape[0]
    plain = []
    for _ in range(2):
        m = scene.model()
        assert scene.pipe.rawTrainCams(scene.cams, ITERS, SEED, False) == ITERS
        plain.append(_state(m))
    _same(plain[1], plain[0], "two runs with one seed, no densification")


def test_without_densification_the_count_stays(scene):
    m = scene.model()
    n0 = m.getGaussianNum()
    scene.pipe.log_iter = 10
    try:
        first = len(scene.pipe.refineLog())
        assert scene.pipe.rawTrainCams(scene.cams, ITERS, SEED) == ITERS       # densify defaults to false
        log = scene.pipe.refineLog()[first:]
    finally:
        scene.pipe.log_iter = 1000
    assert m.getGaussianNum() == n0 and m.densify_events == 0 and m.adamStep() == ITERS and m.hasScheduler()
    assert m.densify_log == [] and m.opacity_reset_log == [] and m.densifyStats()[1].sum() == 0    # no statistics either
    b = scene.model()
    _losses_agree(log, hand_loop(scene, b, ITERS, SEED, densify=False))
    _same(_state(m), _state(b), "densify = false against the loop written here")
    assert not np.array_equal(model_arrays(m)[0][0], scene.tensors[0].cpu().numpy())
    # trainCams dispatches on the mode
    scene.model()
    scene.pipe.max_iterations = 3
    try:
        assert scene.pipe.trainCams(scene.cams, "raw") == 3
        with pytest.raises(RuntimeError, match="'raw' or 'ges'"):
            scene.pipe.trainCams(scene.cams, "mesh")
    finally:
        scene.pipe.max_iterations = 10000


def test_ges_model_refuses_raw_train_cams(scene):
    m = scene.model(render_method="ges")
    with pytest.raises(RuntimeError, match="render_method must be 'raw', got 'ges'"):
        scene.pipe.rawTrainCams(scene.cams, 5, SEED, True)
    assert scene.pipe.curr_iter == 0 and m.getGaussianNum() == scene.tensors[0].shape[0] and m.adamStep() == 0
    raw = scene.model()
    with pytest.raises(RuntimeError, match="render_method must be 'ges', got 'raw'"):
        scene.pipe.trainCams(scene.cams, "ges")
    assert raw.adamStep() == 0


def test_ordered_backward_is_the_atomic_one_to_rounding_and_itself_to_the_bit(scene):
    """ordered_raw_backward (gps_raster_raw_bwd_ordered): the gradients of gps_raster_raw_bwd summed in a fixed order.  Against the
    atomic version: the tolerance tests/test_host_cpp_gpu.py uses between two accumulation orders of the same kernels.  Against a
    second call: every bit, also of the retained means2d gradient the densification statistics read."""
    grads = {}
    for name, ordered in (("atomic", False), ("ordered", True), ("ordered again", True)):
        m = scene.model()
        m.initOptimizers(-1, SCENE_SCALE)
        m.ordered_raw_backward = ordered
        cam = scene.cams[1]
        res = m.rawForward(cam)
        res["means2d"].retain_grad()
        loss = m.computeLoss(res, cam, dict(ssim_weight=0.0, depth_weight=0.0))
        (loss["total"] + 0.1 * res["depth"].mean() + 0.05 * res["alpha"].mean()).backward()
        torch.cuda.synchronize()
        grads[name] = [g.cpu().numpy() for g in m.leafGrads()] + [res["means2d"].grad.cpu().numpy()]
    assert len(grads["ordered"]) == 7
    for k, (a, b) in enumerate(zip(grads["ordered"], grads["ordered again"])):
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), k
    for k, (a, b) in enumerate(zip(grads["ordered"], grads["atomic"])):
        assert np.abs(b).max() > 0, k
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5 * float(np.abs(b).max()), err_msg=str(k))
