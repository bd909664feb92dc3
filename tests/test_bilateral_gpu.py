"""The bilateral depth filter (ITMLibSettings::useBilateralFilter) on the device, against the REFERENCE's own view builder and CPU
engine with the option on, linked against a correctly rounded expf (tests/golden/bilateral.npz, written by
tests/golden/make_bilateral_golden.py): the kernel bit for bit, the engines' digests after every frame with given poses, the
tracker's poses within the tracker's tolerance, the relocaliser's code and GetImage's depth view from the filtered image, and
the option off."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import bilateral_cases as cases
from tests.digests import crc, engine_getter, frame_digest
from tests.test_oracle_tsdf import bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "bilateral.npz"))


def _filter_on_device(mm):
    """gps_tsdf_convert_filter_depth on an int16 [H, W] image, with a state that holds nothing but what the call reads and a
    scratch full of garbage -> float32 [H, W]"""
    from gps_slam_amd._lib import TsdfState, check, lib
    H, W = mm.shape
    d_mm = torch.as_tensor(np.ascontiguousarray(mm)).to(DEV)
    out = torch.full((H, W), 123.0, dtype=torch.float32, device=DEV)
    nbytes = int(lib.gps_tsdf_filter_scratch_bytes(W, H))
    assert nbytes == 2 * W * H * 4
    scratch = torch.full((nbytes + 64,), 0xC3, dtype=torch.uint8, device=DEV)   # any contents; 64 guard bytes behind it
    s = TsdfState()
    s.width, s.height, s.depth = W, H, out.data_ptr()
    check(lib.gps_tsdf_convert_filter_depth(C.byref(s), d_mm.data_ptr(), scratch.data_ptr(), None), "gps_tsdf_convert_filter_depth")
    torch.cuda.synchronize()
    assert (scratch[nbytes:] == 0xC3).all()
    return out.cpu().numpy()


def _assert_same_image(got, want, mm, what):
    """zero differing pixels; a difference is reported with the pixel, both values and the centre's converted depth"""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if len(bad):
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first (x %d, y %d): device %r (0x%08x), reference %r (0x%08x), input %d mm"
                             % (what, len(bad), x, y, got[y, x], got.view(np.uint32)[y, x], want[y, x], want.view(np.uint32)[y, x],
                                int(mm[y, x])))


@pytest.mark.parametrize("tag", sorted(cases.KERNEL_CASES))
def test_kernel_is_bit_equal_to_the_reference(tag):
    W, H = cases.KERNEL_CASES[tag]
    mm = cases.kernel_depth(tag)
    assert crc(mm) == G[tag + "_input_crc"]
    got, want = _filter_on_device(mm), G[tag + "_filtered"]
    ring = cases.ring_mask(H, W)
    assert (got[ring].view(np.uint32) == 0).all(), "the ring is 0.0f"
    assert ((cases.convert(mm) < 0)[~ring] == (got[~ring] == -1.0)).all(), "holes stay -1"
    _assert_same_image(got, want, mm, tag)
    if tag == "k4x7":
        assert (got.view(np.uint32) == 0).all()
    if tag == "k5x5":
        assert np.count_nonzero(got) == 1 and got[2, 2] > 0
    if tag == "k100x52":
        assert int(G["k_denormal_weights_pass1"]) > 0 and int(G["k_zero_weights_pass1"]) > 0   # what the image went through


def test_kernel_many_tiles_against_the_transcription():
    """a 131 x 67 image (5 x 9 tiles, both edges ragged, a depth step across tile borders) against the float32 transcription that
    test_bilateral_cpu.py pins to the reference"""
    W, H = 131, 67
    rng = np.random.default_rng(5)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mm = 800 + 5 * xs + 9 * ys + rng.integers(-6, 7, (H, W))
    mm[:, 64:] += 35
    mm[33:, :] += 1500
    mm[rng.random((H, W)) < 0.03] = 0
    mm = mm.astype(np.int16)
    _assert_same_image(_filter_on_device(mm), cases.filter5(mm), mm, "131x67")


@functools.lru_cache(maxsize=None)
def _sequence(tag):
    seq = cases.sequence(tag)
    rgba = np.concatenate([seq["rgb"], np.full(seq["rgb"].shape[:-1] + (1,), 255, np.uint8)], -1)
    return seq, torch.as_tensor(rgba).to(DEV), torch.as_tensor(seq["depth"].astype(np.int16)).to(DEV)


def _py_engine(tag, **kw):
    from gps_slam_amd.tsdf_engine import TsdfEngine
    seq = _sequence(tag)[0]
    return TsdfEngine(seq["W"], seq["H"], seq["fx"], seq["fy"], seq["cx"], seq["cy"], float(G["voxel"]), float(G["mu"]),
                      float(G["vf_min"]), float(G["vf_max"]), device=DEV, **kw)


def _cpp_engine(tag):
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    seq = _sequence(tag)[0]
    return h, h.ITMBasicEngine(seq["W"], seq["H"], seq["fx"], seq["fy"], seq["cx"], seq["cy"], float(G["voxel"]), float(G["mu"]),
                               float(G["vf_min"]), float(G["vf_max"]))


class _CppState:
    """the C++ engine's device state behind the attributes tests.test_tsdf_gpu.EngineView reads"""

    def __init__(self, eng, W, H):
        from gps_slam_amd.tsdf_engine import HASH_DT, VOXEL_DT
        self.W, self.H = W, H
        self._t = eng.stateTensors()
        self._hash_dt, self._voxel_dt = HASH_DT, VOXEL_DT
        for k, v in self._t.items():
            setattr(self, k, v)
        self.fv_minmax = self.fv_raycast = self.fv_colour = None   # (EngineView names them; nothing here reads the free view)

    def counters_host(self):
        return self.counters.cpu().numpy()

    def hash_host(self):
        return self.hash.cpu().numpy().view(self._hash_dt)

    def vba_host(self, ptrs):
        idx = torch.as_tensor(np.asarray(ptrs, dtype=np.int64), device=self.vba.device)
        return self.vba.view(-1, 512 * 8)[idx].cpu().numpy().view(self._voxel_dt).reshape(-1, 512)


def _check_digests(tag, f, view, W, H):
    got = frame_digest(engine_getter(view), f, W, H)
    for k, val in got.items():
        assert np.array_equal(np.asarray(val), G["%s_%s@%d" % (tag, k, f)]), (tag, k, f)


@pytest.mark.parametrize("tag", ["g", "f"])
def test_given_pose_runs_equal_the_reference_engine(tag):
    """Python mirror and C++ host, option on ("f": the approximate raycast on as well): after every frame the filtered depth,
    the block set, the voxel payload, the visible list, the min/max window, the live raycast, the ICP maps and the colour image"""
    from tests.test_tsdf_gpu import EngineView
    seq, rgb, dep = _sequence(tag)
    W, H, n, approx = seq["W"], seq["H"], int(G[tag + "_n_frames"]), bool(G[tag + "_approx"])
    eng_p = _py_engine(tag, use_bilateral_filter=True, use_approximate_raycast=approx)
    h, eng_c = _cpp_engine(tag)
    eng_c.turnOffTracking()
    assert eng_c.usesBilateralFilter() is False and eng_c.hasFilterScratch() is False
    eng_c.setUseBilateralFilter(True)
    eng_c.setUseApproximateRaycast(approx)
    view_p, view_c = EngineView(eng_p), EngineView(_CppState(eng_c, W, H))
    for f in range(n):
        M, invM = eng_p.ProcessFrame(rgb[f], dep[f], seq["c2w"][f])
        eng_c.pushGtPose(torch.as_tensor(seq["c2w"][f].astype(np.float32)))
        eng_c.ProcessFrame(rgb[f], dep[f])
        assert bits_equal(M, G[tag + "_M"][f]) and bits_equal(invM, G[tag + "_invM"][f])
        assert bits_equal(eng_c.lastPose().numpy()[0], G[tag + "_M"][f])
        assert eng_p.age_pointCloud == eng_c.agePointCloud() == int(G[tag + "_ages"][f])
        _check_digests(tag, f, view_p, W, H)
        _check_digests(tag, f, view_c, W, H)
        eng_p.runRaycast(); eng_c.runRaycast()
        assert crc(eng_p.GetLiveImage().cpu().numpy()) == G[tag + "_live_crc"][f], (tag, f, "colour image, Python")
        assert crc(eng_c.GetLiveImage().cpu().numpy()) == G[tag + "_live_crc"][f], (tag, f, "colour image, C++")
        for eng, img in ((eng_p, eng_p.GetImage("ORIGINAL_DEPTH")), (eng_c, eng_c.GetImage("ORIGINAL_DEPTH"))):
            assert crc(img.cpu().numpy()) == G[tag + "_img1_crc"][f], (tag, f, "GetImage(ORIGINAL_DEPTH)")
        if tag == "g" and f == int(G["g_full_frame"]):
            assert bits_equal(eng_p.depth.cpu().numpy().reshape(H, W), G["g_full_depth"])
            assert np.array_equal(eng_c.GetImage("ORIGINAL_DEPTH").cpu().numpy(), G["g_full_img1"])
    assert eng_c.hasFilterScratch() and eng_p._filter_scratch is not None
    # resetAll keeps the setting: frame 0 again gives frame 0's digests again
    eng_p.reset(); eng_c.resetAll()
    assert eng_p.use_bilateral_filter and eng_c.usesBilateralFilter()
    eng_p.ProcessFrame(rgb[0], dep[0], seq["c2w"][0])
    eng_c.ProcessFrame(rgb[0], dep[0])
    _check_digests(tag, 0, view_p, W, H)
    _check_digests(tag, 0, view_c, W, H)
    if approx:
        assert (G[tag + "_ages"] > 0).any()


def test_tracked_run_follows_the_reference_poses():
    """tracker on, option on, 160 x 120 (below that the reference's own tracker answers NaN poses, 64 x 48 included): the tracker
    aligns the FILTERED depth; poses within the tolerance of test_forward_render_gpu's tracked run (tree against scan-order sums:
    2e-5 on every matrix entry), through both hosts"""
    tag = "t"
    seq, rgb, dep = _sequence(tag)
    W, H = seq["W"], seq["H"]
    eng_p = _py_engine(tag, use_bilateral_filter=True)
    eng_p.turnOnTracking()
    h, eng_c = _cpp_engine(tag)
    eng_c.setUseBilateralFilter(True)
    for f in range(int(G[tag + "_n_frames"])):
        M, invM = eng_p.ProcessFrameTracked(rgb[f], dep[f])
        eng_c.ProcessFrame(rgb[f], dep[f])
        assert crc(eng_p.depth.cpu().numpy().reshape(H, W)) == G["%s_depth_f@%d" % (tag, f)], (f, "filtered depth")
        err = max(np.abs(M - G[tag + "_M"][f]).max(), np.abs(invM - G[tag + "_invM"][f]).max())
        pc = eng_c.lastPose().numpy()
        err_c = max(np.abs(pc[0] - G[tag + "_M"][f]).max(), np.abs(pc[1] - G[tag + "_invM"][f]).max())
        print("frame %d: pose error %.3g (Python mirror), %.3g (C++ host)" % (f, err, err_c))
        assert err < 2e-5 and err_c < 2e-5, (f, err, err_c)
        assert eng_p.age_pointCloud == eng_c.agePointCloud() == int(G[tag + "_ages"][f])
    moved = np.abs(G[tag + "_M"][-1] - G[tag + "_M"][0]).max()
    assert moved > 1e-3, "the sequence does not move: the tolerance would show nothing"


def test_relocalise_mode_and_get_image_read_the_filtered_depth():
    """FAILUREMODE_RELOCALISE with given poses through the C++ host: the view's depth, the false-colour depth image and the fern
    code of every frame (the reference's own fern table, through the device relocaliser) equal the reference's"""
    from gps_slam_amd.relocaliser import FernRelocaliser
    tag = "r"
    seq, rgb, dep = _sequence(tag)
    W, H, n = seq["W"], seq["H"], int(G[tag + "_n_frames"])
    h, eng = _cpp_engine(tag)
    eng.turnOffTracking()
    eng.setFailureMode(h.FailureMode.FAILUREMODE_RELOCALISE)
    eng.setUseBilateralFilter(True)
    depth = eng.stateTensors()["depth"].view(H, W)
    rl = FernRelocaliser(W, H, depth_range=(float(G["vf_min"]), float(G["vf_max"])), device=DEV)
    rl.set_ferns(G[tag + "_ferns_xy"], G[tag + "_ferns_thr"])
    rl.enable_debug_outputs()
    for f in range(n):
        eng.pushGtPose(torch.as_tensor(seq["c2w"][f].astype(np.float32)))
        eng.ProcessFrame(rgb[f], dep[f])
        assert eng.hasRelocaliser()
        assert crc(depth.cpu().numpy()) == G["%s_depth_f@%d" % (tag, f)], (f, "filtered depth")
        assert crc(eng.GetImage("ORIGINAL_DEPTH").cpu().numpy()) == G[tag + "_img1_crc"][f], (f, "GetImage(ORIGINAL_DEPTH)")
        pose = eng.lastPose().numpy()
        rl.process_frame(depth.contiguous(), pose[0], pose[1])
        torch.cuda.synchronize()
        assert np.array_equal(rl.code.cpu().numpy(), G[tag + "_codes"][f]), (f, "fern code")
    assert eng.relocaliserEntries() >= 1
    rl.close()


def test_off_is_off():
    """use_bilateral_filter=False, setUseBilateralFilter(False) and an engine that was never told: the same digests after every
    frame, and no scratch is ever allocated"""
    from tests.test_tsdf_gpu import EngineView
    tag = "g"
    seq, rgb, dep = _sequence(tag)
    W, H, n = seq["W"], seq["H"], int(G[tag + "_n_frames"])
    eng_off, eng_plain = _py_engine(tag, use_bilateral_filter=False), _py_engine(tag)
    h, eng_c = _cpp_engine(tag)
    eng_c.turnOffTracking()
    eng_c.setUseBilateralFilter(False)
    views = [EngineView(eng_off), EngineView(eng_plain), EngineView(_CppState(eng_c, W, H))]
    for f in range(n):
        eng_off.ProcessFrame(rgb[f], dep[f], seq["c2w"][f])
        eng_plain.ProcessFrame(rgb[f], dep[f], seq["c2w"][f])
        eng_c.pushGtPose(torch.as_tensor(seq["c2w"][f].astype(np.float32)))
        eng_c.ProcessFrame(rgb[f], dep[f])
        d = [frame_digest(engine_getter(v), f, W, H) for v in views]
        for k in d[0]:
            assert np.array_equal(np.asarray(d[0][k]), np.asarray(d[1][k])) and np.array_equal(np.asarray(d[0][k]), np.asarray(d[2][k])), (k, f)
        assert d[0]["depth_f"] == crc(cases.convert(seq["depth"][f].astype(np.int16)))   # the plain conversion
        assert d[0]["depth_f"] != G["%s_depth_f@%d" % (tag, f)]
    assert eng_off._filter_scratch is None and eng_plain._filter_scratch is None and eng_c.hasFilterScratch() is False
