"""CPU-side checks of the RGB-D calibration (no GPU): the new entry points exist with the declared signatures and report every
argument error before any device work; calib.txt reads to the fixture's numbers and writes the reference's bytes; calib_inv
and M_rgb of the host equal the reference's bit for bit; the numpy transcriptions of the two conversions agree with the
reference's images; the transcription of OUR registration passes the exact-shift case (tests/golden/rgbd_calib.npz, written by
tests/golden/make_rgbd_calib_golden.py from the reference's CPU engine)."""
import ctypes
import os

import numpy as np
import pytest

from tests import rgbd_calib_cases as cases
from tests.digests import crc

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "rgbd_calib.npz"))


def _lib():
    from gps_slam_amd import _build, _lib
    _build.build()
    return _lib.load_library()


def test_c_abi_exports_the_entry_points_with_the_declared_signatures():
    from gps_slam_amd import _build, _lib
    raw = ctypes.CDLL(_build.build())
    i32, vp = ctypes.c_int, ctypes.c_void_p
    S, T = ctypes.POINTER(_lib.TsdfState), ctypes.POINTER(_lib.TrackState)
    D, K = ctypes.POINTER(_lib.DepthCalib), ctypes.POINTER(_lib.ColourCamera)
    want = {"gps_tsdf_convert_depth_calib": (i32, [S, vp, D, vp]),
            "gps_tsdf_convert_filter_depth_calib": (i32, [S, vp, D, vp, vp]),
            "gps_rgbd_m_rgb": (i32, [vp, vp, vp]),
            "gps_tsdf_integrate_rgb": (i32, [S, vp, K, vp]),
            "gps_tsdf_frame_map_rgb": (i32, [S, T, i32, i32, vp, i32, K, vp]),
            "gps_tsdf_register_colour": (i32, [S, K, vp, vp])}
    for name, sig in want.items():
        assert hasattr(raw, name), name
        assert _lib.PROTOTYPES[name] == sig, name
    assert ctypes.sizeof(_lib.DepthCalib) == 12
    assert ctypes.sizeof(_lib.ColourCamera) == 8 + 16 + 64 + 8 and _lib.ColourCamera.rgb.offset == 88
    assert (_lib.DEPTH_CALIB_KINECT, _lib.DEPTH_CALIB_AFFINE) == (0, 1) == (cases.KINECT, cases.AFFINE)


def _state(**kw):
    """a gps_tsdf_state that passes the validity check: every pointer names (host) memory nothing may touch before the checks"""
    from gps_slam_amd._lib import TsdfState
    keep = np.zeros(64, np.uint8)
    s = TsdfState()
    s.width, s.height, s.fx, s.fy, s.cx, s.cy = 16, 12, 8.0, 8.0, 7.5, 5.5
    s.voxel_size, s.mu, s.view_frustum_min, s.view_frustum_max, s.max_w = 0.02, 0.08, 0.2, 10.0, 100
    s.n_blocks, s.n_buckets, s.n_excess = 64, 64, 16
    for name, typ in TsdfState._fields_:
        if typ is ctypes.c_void_p:
            setattr(s, name, keep.ctypes.data)
    for k, v in kw.items():
        setattr(s, k, v)
    return s, keep


def _camera(ptr, **kw):
    from gps_slam_amd._lib import ColourCamera
    c = ColourCamera()
    c.width, c.height, c.fx, c.fy, c.cx, c.cy = 24, 18, 12.0, 12.0, 11.5, 8.5
    c.depth_to_rgb[:] = np.eye(4, dtype=np.float32).reshape(16).tolist()
    c.rgb = ptr
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_argument_errors_come_before_any_device_work():
    from gps_slam_amd._lib import DepthCalib, TrackState
    lib = _lib()
    s, keep = _state()
    S = ctypes.byref(s)
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    ok = DepthCalib(cases.AFFINE, 0.0002, 0.01)
    D = ctypes.byref(ok)
    bad_calibs = [DepthCalib(2, 1.0, 1.0), DepthCalib(-1, 1.0, 1.0), DepthCalib(1 << 20, 1.0, 1.0), DepthCalib(cases.KINECT, 0.0, 0.0)]
    bad_states = [_state(width=0)[0], _state(height=0)[0], _state(width=-16)[0], _state(depth=None)[0]]
    # gps_tsdf_convert_depth_calib(state, raw, calib, stream)
    assert lib.gps_tsdf_convert_depth_calib(None, p, D, None) == -1
    assert lib.gps_tsdf_convert_depth_calib(S, None, D, None) == -1
    assert lib.gps_tsdf_convert_depth_calib(S, p, None, None) == -1
    assert lib.gps_tsdf_convert_depth_calib(S, p + 1, D, None) == -1     # a misaligned raw image
    # gps_tsdf_convert_filter_depth_calib(state, raw, calib, scratch, stream)
    assert lib.gps_tsdf_convert_filter_depth_calib(None, p, D, p, None) == -1
    assert lib.gps_tsdf_convert_filter_depth_calib(S, None, D, p, None) == -1
    assert lib.gps_tsdf_convert_filter_depth_calib(S, p, None, p, None) == -1
    assert lib.gps_tsdf_convert_filter_depth_calib(S, p, D, None, None) == -1
    assert lib.gps_tsdf_convert_filter_depth_calib(S, p, D, p + 2, None) == -1
    for c in bad_calibs:
        assert lib.gps_tsdf_convert_depth_calib(S, p, ctypes.byref(c), None) == -1
        assert lib.gps_tsdf_convert_filter_depth_calib(S, p, ctypes.byref(c), p, None) == -1
    for b in bad_states:
        assert lib.gps_tsdf_convert_depth_calib(ctypes.byref(b), p, D, None) == -1
        assert lib.gps_tsdf_convert_filter_depth_calib(ctypes.byref(b), p, D, p, None) == -1
    # the colour camera: gps_tsdf_integrate_rgb(state, M, cam, stream), gps_tsdf_register_colour(state, cam, out, stream),
    # gps_tsdf_frame_map_rgb(state, track state, fuse, reset_visible, fwd_block, approx, cam, stream)
    cam = _camera(p)
    K = ctypes.byref(cam)
    ts = TrackState()
    assert lib.gps_tsdf_integrate_rgb(None, p, K, None) == -1
    assert lib.gps_tsdf_integrate_rgb(S, None, K, None) == -1
    assert lib.gps_tsdf_integrate_rgb(S, p, None, None) == -1
    assert lib.gps_tsdf_register_colour(None, K, p, None) == -1
    assert lib.gps_tsdf_register_colour(S, None, p, None) == -1
    assert lib.gps_tsdf_register_colour(S, K, None, None) == -1
    assert lib.gps_tsdf_register_colour(S, K, p + 1, None) == -1
    assert lib.gps_tsdf_frame_map_rgb(None, ctypes.byref(ts), 1, 0, None, 0, K, None) == -1
    assert lib.gps_tsdf_frame_map_rgb(S, None, 1, 0, None, 0, K, None) == -1
    assert lib.gps_tsdf_frame_map_rgb(None, ctypes.byref(ts), 1, 0, None, 0, None, None) == -1   # NULL camera: today's call, today's checks
    for bad in (_camera(p, width=0), _camera(p, height=0), _camera(p, width=-3), _camera(None), _camera(p + 2)):
        B = ctypes.byref(bad)
        assert lib.gps_tsdf_integrate_rgb(S, p, B, None) == -1
        assert lib.gps_tsdf_register_colour(S, B, p, None) == -1
        assert lib.gps_tsdf_frame_map_rgb(S, ctypes.byref(ts), 1, 0, None, 0, B, None) == -1
    for hole in ("hash", "vba", "visible_ids"):   # the integration needs a scene
        b, _k = _state(**{hole: None})
        assert lib.gps_tsdf_integrate_rgb(ctypes.byref(b), p, K, None) == -1
    for b in bad_states:
        assert lib.gps_tsdf_register_colour(ctypes.byref(b), K, p, None) == -1
    assert lib.gps_rgbd_m_rgb(None, p, p) == -1 and lib.gps_rgbd_m_rgb(p, None, p) == -1 and lib.gps_rgbd_m_rgb(p, p, None) == -1
    assert not keep.any() and not buf.any()


def _calib_of(tag):
    from gps_slam_amd.rgbd_calib import read_rgbd_calib
    return read_rgbd_calib(os.path.join(HERE, "golden", "rgbd_calib_%s.txt" % tag))


@pytest.mark.parametrize("tag", sorted(cases.RUNS))
def test_calib_txt_reads_to_the_fixtures_numbers_and_writes_the_references_bytes(tag, tmp_path):
    from gps_slam_amd.rgbd_calib import format_rgbd_calib, write_rgbd_calib
    run = cases.RUNS[tag]
    intr_d, intr_c = cases.intrinsics(tag)
    c = _calib_of(tag)
    assert (c.intrinsics_rgb.width, c.intrinsics_rgb.height) == run["c"] and (c.intrinsics_d.width, c.intrinsics_d.height) == run["d"]
    f32 = lambda v: tuple(float(np.float32(x)) for x in v)
    assert c.intrinsics_rgb.params() == f32(intr_c) and c.intrinsics_d.params() == f32(intr_d)
    assert np.array_equal(c.trafo_rgb_to_depth.calib.view(np.uint32), cases.to_orutils(run["ext"]).view(np.uint32))
    assert np.array_equal(c.trafo_rgb_to_depth.calib_inv.view(np.uint32), G[tag + "_calib_inv"].view(np.uint32)), "calib_inv, bit for bit"
    typ, a, b = run["calib"]
    assert c.disparityCalib.GetType() == typ and c.disparityCalib.GetParams() == f32((a, b))
    # writing: the reference's bytes, from the struct and through a file
    text = open(os.path.join(HERE, "golden", "rgbd_calib_%s.txt" % tag)).read()
    assert format_rgbd_calib(c) == text
    write_rgbd_calib(str(tmp_path / "calib.txt"), c)
    assert open(str(tmp_path / "calib.txt")).read() == text


def test_disparity_calib_rules_of_the_reference():
    from gps_slam_amd.rgbd_calib import TRAFO_AFFINE, TRAFO_KINECT, DisparityCalib, parse_rgbd_calib
    d = DisparityCalib()
    assert d.GetType() == TRAFO_AFFINE and d.GetParams() == (float(np.float32(1.0) / np.float32(1000.0)), 0.0) and d.is_standard()
    d.SetFrom(0.0, 0.0, TRAFO_KINECT)   # both zero -> standard
    assert d.is_standard()
    d.SetFrom(1090.0, 0.0, TRAFO_KINECT)
    assert d.GetType() == TRAFO_KINECT and not d.is_standard()
    head = "4 3\n2 2\n1.5 1\n\n4 3\n2 2\n1.5 1\n\n1 0 0 0\n0 1 0 0\n0 0 1 0\n\n"
    assert parse_rgbd_calib(head + "0 0\n").disparityCalib.is_standard()                 # a bare pair is Kinect; both zero: standard
    assert parse_rgbd_calib(head + "1135.09 0.0819141\n").disparityCalib.GetType() == TRAFO_KINECT
    assert parse_rgbd_calib(head + "kinect 1135.09 0.0819141\n").disparityCalib.GetType() == TRAFO_KINECT
    assert parse_rgbd_calib(head + "affine 0.0002 0\n").disparityCalib.GetParams() == (float(np.float32(0.0002)), 0.0)
    with pytest.raises(ValueError):
        parse_rgbd_calib(head + "polynomial 1 2\n")
    with pytest.raises(ValueError):
        parse_rgbd_calib(head)


@pytest.mark.parametrize("tag", sorted(cases.RUNS))
def test_m_rgb_of_the_host_equals_the_references(tag):
    """gps_rgbd_m_rgb (the product the integration entry forms) and the numpy transcription, against calib_inv * M_d of the
    reference for every frame"""
    from gps_slam_amd.rgbd_calib import m_rgb
    _lib()
    inv = _calib_of(tag).trafo_rgb_to_depth.calib_inv
    for f in range(int(G[tag + "_n_frames"])):
        want = G[tag + "_M_rgb"][f]
        assert np.array_equal(m_rgb(inv, G[tag + "_M"][f]).view(np.uint32), want.view(np.uint32)), (tag, f)
        assert np.array_equal(cases.mat_mul(inv, G[tag + "_M"][f]).view(np.uint32), want.view(np.uint32)), (tag, f)
    if tag in cases.TWO_CAMERA_RUNS:
        assert not np.array_equal(G[tag + "_M_rgb"][0], G[tag + "_M"][0])


@pytest.mark.parametrize("size_tag", sorted(cases.CONV_SIZES))
@pytest.mark.parametrize("calib_tag", sorted(cases.CONV_CALIBS))
def test_conversion_transcriptions_agree_with_the_reference(size_tag, calib_tag):
    typ, a, b = cases.CONV_CALIBS[calib_tag]
    raw = cases.conv_raw(size_tag, calib_tag)
    assert crc(raw) == G["%s_%s_input_crc" % (size_tag, calib_tag)]
    want = G["%s_%s_plain" % (size_tag, calib_tag)]
    got = cases.convert(raw, typ, a, b, float(G["conv_fx"]))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if typ == cases.AFFINE and size_tag == "c100x52":
        assert (cases.convert_fused(raw, a, b).view(np.uint32) != want.view(np.uint32)).any(), "a contracted kernel would pass"


def test_runs_regenerate_and_their_depth_is_the_transcriptions():
    for tag in ("wide", "kinect", "tum"):
        run = cases.make_run(tag)
        assert [crc(run["rgb"]), crc(run["raw"]), crc(run["c2w"])] == G[tag + "_input_crc"].tolist(), tag
        typ, a, b = run["calib"]
        got = cases.convert(run["raw"][-1], typ, a, b, run["intr_d"][0])
        assert np.array_equal(got.view(np.uint32), G[tag + "_full_depth"].view(np.uint32)), tag
    assert int(G["wide_near_with_colour"]) > 0 and int(G["wide_near_without_colour"]) > 0
    assert int(G["narrow_near_with_colour"]) > 0 and int(G["narrow_near_without_colour"]) > 0


def test_registration_transcription_on_the_exact_shift_case():
    """the registration has no reference: its transcription is pinned on a case where every intermediate is exact in float32 and
    the expected image is the source moved by whole pixels"""
    depth_f, intr_d, inv, intr_c, rgb, want = cases.exact_shift_case()
    got = cases.register_colour(depth_f, intr_d, inv, intr_c, rgb)
    assert np.array_equal(got, want)
    assert (want[..., 3] == 255).any() and (want[..., 3] == 0).any()
    assert (got[5, 7] == 0).all()   # the invalid depth pixel


def _host():
    _lib()
    import gps_slam_amd._host as h
    return h


@pytest.mark.parametrize("tag", sorted(cases.RUNS))
def test_cpp_host_reads_and_writes_calib_txt_and_forms_the_references_matrices(tag, tmp_path):
    """the C++ host (readRGBDCalib / writeRGBDCalib, ITMExtrinsics::SetFrom, gps_rgbd_m_rgb through ITMRGBDCalib): the fixture's
    numbers, the reference's bytes, calib_inv and M_rgb bit for bit -- the same checks as for the Python host above"""
    h = _host()
    run = cases.RUNS[tag]
    intr_d, intr_c = cases.intrinsics(tag)
    path = os.path.join(HERE, "golden", "rgbd_calib_%s.txt" % tag)
    text = open(path).read()
    c = h.readRGBDCalib(path)
    f32 = lambda v: tuple(float(np.float32(x)) for x in v)
    assert c.intrinsicsRgb() == run["c"] + f32(intr_c) and c.intrinsicsD() == run["d"] + f32(intr_d)
    assert np.array_equal(np.array(c.calib(), np.float32).view(np.uint32), cases.to_orutils(run["ext"]).view(np.uint32))
    assert np.array_equal(np.array(c.calibInv(), np.float32).view(np.uint32), G[tag + "_calib_inv"].view(np.uint32))
    typ, a, b = run["calib"]
    assert c.disparityCalib() == (typ,) + f32((a, b))
    assert h.formatRGBDCalib(c) == text
    h.writeRGBDCalib(str(tmp_path / "calib.txt"), c)
    assert open(str(tmp_path / "calib.txt")).read() == text
    assert h.formatRGBDCalib(h.parseRGBDCalib(text)) == text
    for f in range(int(G[tag + "_n_frames"])):
        got = np.array(c.mRgb(G[tag + "_M"][f].tolist()), np.float32)
        assert np.array_equal(got.view(np.uint32), G[tag + "_M_rgb"][f].view(np.uint32)), (tag, f)


def test_cpp_host_disparity_calib_rules_of_the_reference():
    h = _host()
    c = h.ITMRGBDCalib()
    std = (cases.AFFINE, float(np.float32(1.0) / np.float32(1000.0)), 0.0)
    assert c.disparityCalib() == std
    c.setDisparityCalib(0.0, 0.0, cases.KINECT)   # both zero -> standard
    assert c.disparityCalib() == std
    c.setDisparityCalib(1090.0, 0.0, cases.KINECT)
    assert c.disparityCalib() == (cases.KINECT, 1090.0, 0.0)
    head = "4 3\n2 2\n1.5 1\n\n4 3\n2 2\n1.5 1\n\n1 0 0 0\n0 1 0 0\n0 0 1 0\n\n"
    assert h.parseRGBDCalib(head + "0 0\n").disparityCalib() == std
    assert h.parseRGBDCalib(head + "1135.09 0.0819141\n").disparityCalib()[0] == cases.KINECT
    assert h.parseRGBDCalib(head + "kinect 1135.09 0.0819141\n").disparityCalib()[0] == cases.KINECT
    assert h.parseRGBDCalib(head + "affine 0.0002 0\n").disparityCalib() == (cases.AFFINE, float(np.float32(0.0002)), 0.0)
    for bad in (head + "polynomial 1 2\n", head):
        with pytest.raises(RuntimeError):
            h.parseRGBDCalib(bad)
    assert np.array_equal(np.array(h.ITMRGBDCalib().calibInv(), np.float32), np.eye(4, dtype=np.float32).reshape(16))
