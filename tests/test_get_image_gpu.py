"""ITMBasicEngine::GetImage on the device against the REFERENCE's own CPU engine (tests/golden/get_image.npz, written by
tests/golden/make_get_image_golden.py): every image type after every frame, byte for byte -- r, g, b for the normal types, whose
alpha the reference leaves to the previous render (here: 255 on a found pixel).  The kernels that need no volume are also run
alone on hand-made images against the float32 transcriptions of tests/get_image_cases.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import get_image_cases as cases
from tests.digests import engine_getter, frame_digest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "get_image.npz"))
GREY, IMAGENORMALS, VOLUME, NORMAL, CONFIDENCE = range(5)   # gps_render_type


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


@functools.lru_cache(maxsize=None)
def _sequence(tag):
    seq = cases.make_run(tag)
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    return seq, torch.as_tensor(rgba).to(DEV), torch.as_tensor(seq["depth"].astype(np.int16)).to(DEV)


class _Mirror:
    """the Python mirror behind the interface the checks use"""

    def __init__(self, tag):
        from gps_slam_amd.tsdf_engine import TsdfEngine
        seq = _sequence(tag)[0]
        self.eng = TsdfEngine(seq["W"], seq["H"], seq["fx"], seq["fy"], seq["cx"], seq["cy"], float(G["voxel"]), float(G["mu"]),
                              float(G["vf_min"]), float(G["vf_max"]), device=DEV, use_approximate_raycast=bool(G[tag + "_approx"]))
        self.tag = tag

    def frame(self, f):
        seq, rgb, dep = _sequence(self.tag)
        self.eng.ProcessFrame(rgb[f], dep[f], seq["c2w"][f])

    def image(self, name, c2w=None):
        return self.eng.GetImage("InfiniTAM_IMAGE_" + name, c2w=c2w).cpu().numpy()

    def age(self):
        return self.eng.age_pointCloud


class _Host:
    """the C++ host (pybind) behind the same interface"""

    def __init__(self, tag):
        h = _host()
        seq = _sequence(tag)[0]
        self.eng = h.ITMBasicEngine(seq["W"], seq["H"], seq["fx"], seq["fy"], seq["cx"], seq["cy"], float(G["voxel"]), float(G["mu"]),
                                    float(G["vf_min"]), float(G["vf_max"]))
        self.eng.turnOffTracking()
        self.eng.setUseApproximateRaycast(bool(G[tag + "_approx"]))
        self.tag = tag

    def frame(self, f):
        seq, rgb, dep = _sequence(self.tag)
        self.eng.pushGtPose(torch.as_tensor(seq["c2w"][f].astype(np.float32)))
        self.eng.ProcessFrame(rgb[f], dep[f])

    def image(self, name, c2w=None):
        return self.eng.GetImage(name, c2w=None if c2w is None else torch.as_tensor(np.asarray(c2w, np.float32))).cpu().numpy()

    def age(self):
        return self.eng.agePointCloud()


def _check_run(e):
    """every image type after every frame, in the fixture's call order"""
    tag = e.tag
    seq = _sequence(tag)[0]
    n, full = int(G[tag + "_n_frames"]), int(G[tag + "_full_frame"])
    for f in range(n):
        e.frame(f)
        assert e.age() == int(G[tag + "_ages"][f]), (tag, f)
        for k, name in enumerate(cases.LIVE_TYPES):
            img = e.image(name)
            assert img.shape == (seq["H"], seq["W"], 4) and img.dtype == np.uint8
            assert cases.image_crc(name, img) == G[tag + "_live_crc"][f, k], (tag, f, name)
            if f == full:
                assert cases.same_image(name, img, G[tag + "_full_live"][k]), (tag, f, name)
        for v, c2w in enumerate(cases.free_poses(seq["c2w"][f])):
            for k, name in enumerate(cases.FREE_TYPES):
                img = e.image(name, c2w)
                assert cases.image_crc(name, img) == G[tag + "_free_crc"][f, v, k], (tag, f, v, name)
                if f == full and not bool(G[tag + "_approx"]):
                    assert cases.same_image(name, img, G[tag + "_full_free"][v, k]), (tag, f, v, name)
                if name in cases.NORMAL_TYPES:   # ours: alpha 255 exactly where something is drawn
                    assert np.array_equal(img[..., 3] == 255, img[..., :3].any(-1)) and set(np.unique(img[..., 3])) <= {0, 255}


@pytest.mark.parametrize("tag", ["a", "b"])
def test_python_mirror_gives_the_references_images(tag):
    _check_run(_Mirror(tag))


def test_cpp_host_gives_the_references_images():
    _check_run(_Host("b"))


def test_approximate_raycast_run_renders_the_forward_projection():
    from gps_slam_amd._lib import check, lib
    e = _Mirror("f")
    _check_run(e)
    # the last frame is a forward frame: the live types read the forward projection, not the last full cast
    eng = e.eng
    assert eng.age_pointCloud > 0
    invM = eng.camPoses[-1][1]
    fwd, full_cast = eng.GetForwardProjection(), eng.GetLiveVertex()
    assert not torch.equal(fwd.view(torch.int32), full_cast.view(torch.int32))
    out = torch.zeros((eng.H, eng.W, 4), dtype=torch.uint8, device=DEV)
    for name, t in (("SCENERAYCAST", IMAGENORMALS), ("COLOUR_FROM_VOLUME", VOLUME), ("COLOUR_FROM_NORMAL", NORMAL),
                    ("COLOUR_FROM_CONFIDENCE", CONFIDENCE)):
        got = eng.GetImage(name)
        check(lib.gps_tsdf_render_image(C.byref(eng.state), fwd.data_ptr(), eng.W, eng.H, invM.ctypes.data, t, out.data_ptr(), eng._stream()), name)
        assert torch.equal(got, out), name
        check(lib.gps_tsdf_render_image(C.byref(eng.state), full_cast.data_ptr(), eng.W, eng.H, invM.ctypes.data, t, out.data_ptr(), eng._stream()), name)
        assert not torch.equal(got, out), name


# ------------------------------------------------------------------------------------------- the kernels alone
def _render_image_normals(rays, invM, voxel=0.02):
    from gps_slam_amd._lib import TsdfState, check, lib
    H, W = rays.shape[:2]
    s = TsdfState()
    s.voxel_size, s.fx, s.fy = voxel, 1.0, 1.0   # all this type reads of the state
    r = torch.as_tensor(np.ascontiguousarray(rays, np.float32)).to(DEV)
    out = torch.full((H, W, 4), 0x5A, dtype=torch.uint8, device=DEV)
    m = np.ascontiguousarray(invM, np.float32)
    check(lib.gps_tsdf_render_image(C.byref(s), r.data_ptr(), W, H, m.ctypes.data, IMAGENORMALS, out.data_ptr(), None), "gps_tsdf_render_image")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _surface(W, H):
    """a ray image of a tilted, slightly curved surface, one voxel per pixel: every pixel found, every normal towards the camera"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    z = 40.0 + 0.3 * xs + 0.2 * ys + 0.01 * xs * ys
    return np.stack([xs, ys, z.astype(np.float32), np.full_like(xs, 1.5)], -1)


INV_M = np.eye(4, dtype=np.float32).reshape(-1)   # column 2 = (0, 0, 1): the light is (0, 0, -1)


def test_image_normals_kernel_at_the_border():
    rays = _surface(7, 7)
    got = _render_image_normals(rays, INV_M)
    want = cases.grey_image_normals(rays, INV_M, 0.02)
    assert np.array_equal(got, want)
    assert got[3, 3, 0] > 51 and np.count_nonzero(got.any(-1)) == 1   # exactly one pixel, (3, 3), passes the border test
    rays = _surface(6, 6)                                                # none passes: every output is 0
    got = _render_image_normals(rays, INV_M)
    assert not got.any() and np.array_equal(got, cases.grey_image_normals(rays, INV_M, 0.02))


def test_image_normals_kernel_fallback_to_the_nearer_neighbours():
    W, H = 21, 19
    rays = _surface(W, H)
    # each of the four +-2 neighbours missing in turn; +-1 rescues the pixel
    # (no two holes one or three pixels apart in a row or column: no pixel loses a +-2 and a +-1 neighbour)
    centres = {(6, 5): (8, 5), (14, 5): (14, 7), (6, 13): (4, 13), (14, 14): (14, 12)}
    for (cx, cy), (hx, hy) in centres.items():
        rays[hy, hx, 3] = 0.0
    st = {}
    want = cases.grey_image_normals(rays, INV_M, 0.02, st)
    got = _render_image_normals(rays, INV_M)
    assert np.array_equal(got, want)
    assert st["length_fired"] == 0 and st["fallback_rejected"] == 0 and st["fallback_kept"] >= 4
    for (cx, cy), (hx, hy) in centres.items():
        assert got[cy, cx, 0] > 0          # kept, from the nearer neighbours
        assert not got[hy, hx].any()       # the hole itself is not found
    # one hole where +-1 is missing too: rejected; and a step in depth further than 0.15 m: the length test sends it to +-1
    rays = _surface(W, H)
    rays[9, 12, 3] = 0.0; rays[9, 11, 3] = 0.0
    rays[:, 17:, 2] += 12.0
    st = {}
    want = cases.grey_image_normals(rays, INV_M, 0.02, st)
    got = _render_image_normals(rays, INV_M)
    assert np.array_equal(got, want)
    assert not got[9, 10].any() and rays[9, 10, 3] > 0 and st["fallback_rejected"] >= 1 and st["length_fired"] >= 1
    # w == 0 exactly, w < 0 and a NaN w are all "not found"
    rays = _surface(W, H)
    rays[9, 9, 3] = -1.0; rays[9, 5, 3] = np.nan
    assert np.array_equal(_render_image_normals(rays, INV_M), cases.grey_image_normals(rays, INV_M, 0.02))
    # the light on the other side: nothing is drawn
    flipped = INV_M.copy(); flipped[10] = -1.0
    assert not _render_image_normals(_surface(W, H), flipped).any()


def _depth_colour(depth):
    from gps_slam_amd._lib import check, lib
    d = torch.as_tensor(np.ascontiguousarray(depth, np.float32).reshape(-1)).to(DEV)
    scratch = torch.full((int(lib.gps_tsdf_depth_to_rgba8_scratch_bytes()),), 0xC3, dtype=torch.uint8, device=DEV)   # any contents
    out = torch.full((d.numel(), 4), 0x5A, dtype=torch.uint8, device=DEV)
    for _ in range(2):   # the scratch of one call is the next call's: nothing carries over
        check(lib.gps_tsdf_depth_to_rgba8(d.data_ptr(), d.numel(), scratch.data_ptr(), out.data_ptr(), None), "gps_tsdf_depth_to_rgba8")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(np.shape(depth) + (4,))


def test_depth_to_rgba8():
    assert not _depth_colour(np.zeros(300, np.float32)).any()                       # all depths invalid
    assert not _depth_colour(np.full(300, -2.0, np.float32)).any()
    assert not _depth_colour(np.full(1000, 1.25, np.float32)).any()                 # a constant valid depth: min == max
    two = np.zeros(1000, np.float32); two[3] = 1.0; two[700] = 3.0                  # two values: the end colours
    got = _depth_colour(two)
    assert got[3].tolist() == [127, 255, 127, 255] and got[700].tolist() == [127, 0, 0, 255] and np.count_nonzero(got.any(-1)) == 2
    # a 100 x 75 ramp with invalid pixels (7,500 is no multiple of the workgroup size), and sizes around one workgroup
    ys, xs = np.meshgrid(np.arange(75, dtype=np.float32), np.arange(100, dtype=np.float32), indexing="ij")
    ramp = (0.4 + 0.03 * xs + 0.011 * ys).astype(np.float32)
    ramp[(xs.astype(int) * 5 + ys.astype(int) * 3) % 11 == 0] = 0.0
    ramp[10, 10] = -1.0
    want = cases.depth_to_uchar4(ramp)
    assert np.array_equal(_depth_colour(ramp), want)
    assert all(((want[..., c] > 0) & (want[..., c] < 255)).any() for c in range(3)) and (want[..., 3] == 0).any()
    for n in (1, 63, 255, 256, 257, 7499):
        flat = ramp.reshape(-1)[:n].copy()
        assert np.array_equal(_depth_colour(flat), cases.depth_to_uchar4(flat)), n


# ------------------------------------------------------------------------------------------- the engine around them
def test_host_image_and_device_tensor_hold_the_same_bytes():
    e = _Host("b")
    seq = _sequence("b")[0]
    assert e.eng.GetImage("SCENERAYCAST") is None                                  # no view yet ...
    assert (e.eng.GetImage("SCENERAYCAST", to_host=True).numpy() == 0xAB).all()    # ... and the caller's image is left untouched
    for f in range(3):
        e.frame(f)
    c2w = torch.as_tensor(cases.free_poses(seq["c2w"][2])[0])
    h = _host()
    for name in cases.TYPES:
        kw = dict(c2w=c2w) if name.startswith("FREECAMERA") else {}
        dev = e.eng.GetImage(name, **kw)
        host = e.eng.GetImage(name, to_host=True, **kw)
        assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (seq["H"], seq["W"], 4) and not host.is_cuda
        assert torch.equal(dev.cpu(), host), name
        assert dev.any(), name
        # by enumerator and by value as well as by name
        t = h.GetImageType.__members__["InfiniTAM_IMAGE_" + name]
        assert torch.equal(e.eng.GetImage(t, **kw), dev) and torch.equal(e.eng.GetImage(int(t), **kw), dev), name
    assert not e.eng.GetImage("UNKNOWN").any() and not e.eng.GetImage("UNKNOWN", to_host=True).any()
    with pytest.raises(Exception):
        e.eng.GetImage("SHADED")
    with pytest.raises(Exception):
        e.eng.GetImage("FREECAMERA_SHADED")   # a free camera needs a pose


def test_get_image_changes_nothing_the_frame_chain_reads():
    from tests.test_tsdf_gpu import EngineView
    tag = "b"
    seq = _sequence(tag)[0]
    plain, busy = _Mirror(tag), _Mirror(tag)
    W, H = seq["W"], seq["H"]
    for f in range(int(G[tag + "_n_frames"])):
        plain.frame(f); busy.frame(f)
        eng = busy.eng
        # counters 0..2: free voxel blocks, free excess entries, the length of the live visible list
        watched = lambda: dict(vis_ids=eng.visible_ids, vis_type=eng.visible_type, counters=eng.counters[:3], rays=eng.raycast,
                               minmax=eng.minmax, icp=eng.icp_points)
        before = {k: v.clone() for k, v in watched().items()}
        age = eng.age_pointCloud
        for name in cases.LIVE_TYPES:
            busy.image(name)
        for c2w in cases.free_poses(seq["c2w"][f]):
            for name in cases.FREE_TYPES:
                busy.image(name, c2w)
        for k, v in watched().items():
            assert torch.equal(before[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), (f, k)
        assert eng.age_pointCloud == age and eng.relocalisationCount == 0
        a, b = frame_digest(engine_getter(EngineView(plain.eng)), f, W, H), frame_digest(engine_getter(EngineView(busy.eng)), f, W, H)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (f, k)


def test_live_types_answer_the_cleared_keyframe_image_while_the_relocalisation_count_runs():
    from tests import synth
    h = _host()
    R = h.TrackingResult
    W, H, N, FAIL = 160, 120, 13, 1
    seq = synth.make_sequence(W, H, N, step_deg=0.3)
    rgba = torch.as_tensor(np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)).to(DEV)
    depth = torch.as_tensor(seq["depth"].astype(np.int16)).to(DEV)
    eng = h.ITMBasicEngine(W, H, seq["fx"], seq["fy"], seq["cx"], seq["cy"], 0.01, 0.04, 0.2, 10.0)
    eng.setFailureMode(h.FailureMode.FAILUREMODE_RELOCALISE)
    eng.forceTrackerResult(FAIL, R.TRACKING_FAILED)
    for f in range(FAIL + 1, N):
        eng.forceTrackerResult(f, R.TRACKING_GOOD)
    live = cases.LIVE_TYPES[2:]
    counts = []
    for f in range(N):
        eng.ProcessFrame(rgba[f], depth[f])
        counts.append(eng.relocalisationCount)
        images = {name: eng.GetImage(name) for name in live}
        rendered = eng.GetLiveImage()          # the live render image is rendered all the same
        assert rendered.any(), f
        if eng.relocalisationCount != 0:
            for name in live:
                assert not images[name].any(), (f, name)                 # kfRaycast: cleared, never written
            assert eng.GetImage("ORIGINAL_RGB").any() and eng.GetImage("ORIGINAL_DEPTH").any()   # the originals do not look at the count
        else:
            for name in live:
                assert images[name].any(), (f, name)
            assert torch.equal(images[live[-1]], rendered.view(H, W, 4))   # the last one rendered is what the live image holds
    assert counts == [0] * FAIL + [max(0, 10 - (f - FAIL)) for f in range(FAIL, N)] and counts[-2:] == [0, 0]
