"""CPU-side checks of GetImage (no GPU): the new entry points exist with the declared signatures and report every argument error
before any device work; the pure decision function of the C++ host is the reference's switch (ITMBasicEngine.tpp:416-493) over
the whole table; the Python mirror's constants are the reference's enumerators; the fixture's inputs regenerate."""
import ctypes
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "get_image.npz")
(GREY, IMAGENORMALS, VOLUME, NORMAL, CONFIDENCE) = range(5)   # gps_render_type


def _lib():
    from gps_slam_amd import _build, _lib
    _build.build()
    return _lib.load_library()


def _host():
    _lib()
    import gps_slam_amd._host as h
    return h


def test_c_abi_exports_the_entry_points_with_the_declared_signatures():
    from gps_slam_amd import _build, _lib
    raw = ctypes.CDLL(_build.build())
    i32, i64, vp, S = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(_lib.TsdfState)
    want = {"gps_tsdf_render_image": (i32, [S, vp, i32, i32, vp, i32, vp, vp]),
            "gps_tsdf_depth_to_rgba8_scratch_bytes": (i64, []),
            "gps_tsdf_depth_to_rgba8": (i32, [vp, i32, vp, vp, vp]),
            "gps_tsdf_get_image": (i32, [S, vp, vp, i32, vp, vp])}
    for name, sig in want.items():
        assert hasattr(raw, name), name
        assert _lib.PROTOTYPES[name] == sig, name
    assert int(_lib.load_library().gps_tsdf_depth_to_rgba8_scratch_bytes()) >= 8


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


def test_argument_errors_come_before_any_device_work():
    lib = _lib()
    s, keep = _state()
    S = ctypes.byref(s)
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    # gps_tsdf_render_image(state, rays, width, height, invM, type, out, stream)
    for t in (GREY, IMAGENORMALS, VOLUME, NORMAL, CONFIDENCE):
        assert lib.gps_tsdf_render_image(None, p, 16, 12, p, t, p, None) == -1
        assert lib.gps_tsdf_render_image(S, None, 16, 12, p, t, p, None) == -1
        assert lib.gps_tsdf_render_image(S, p, 16, 12, None, t, p, None) == -1
        assert lib.gps_tsdf_render_image(S, p, 16, 12, p, t, None, None) == -1
        assert lib.gps_tsdf_render_image(S, p, 0, 12, p, t, p, None) == -1
        assert lib.gps_tsdf_render_image(S, p, 16, 0, p, t, p, None) == -1
        assert lib.gps_tsdf_render_image(S, p, -16, 12, p, t, p, None) == -1
    for t in (-1, 5, 11, 1 << 20):   # an unknown type
        assert lib.gps_tsdf_render_image(S, p, 16, 12, p, t, p, None) == -1
        assert lib.gps_tsdf_get_image(S, p, p, t, p, None) == -1
    # the flipped-normal request: focal lengths of opposite sign (ITMIntrinsics::FocalLengthSignsDiffer)
    for fx, fy in ((8.0, -8.0), (-8.0, 8.0)):
        flipped, _k = _state(fx=fx, fy=fy)
        assert lib.gps_tsdf_render_image(ctypes.byref(flipped), p, 16, 12, p, IMAGENORMALS, p, None) == -1
    # the volume types need a scene: a state with a missing table is refused
    for hole in ("hash", "vba"):
        bad, _k = _state(**{hole: None})
        for t in (GREY, VOLUME, NORMAL, CONFIDENCE):
            assert lib.gps_tsdf_render_image(ctypes.byref(bad), p, 16, 12, p, t, p, None) == -1
    # gps_tsdf_depth_to_rgba8(depth, n, scratch, out, stream)
    assert lib.gps_tsdf_depth_to_rgba8(None, 16, p, p, None) == -1
    assert lib.gps_tsdf_depth_to_rgba8(p, 16, None, p, None) == -1
    assert lib.gps_tsdf_depth_to_rgba8(p, 16, p, None, None) == -1
    assert lib.gps_tsdf_depth_to_rgba8(p, 0, p, p, None) == -1
    assert lib.gps_tsdf_depth_to_rgba8(p, -5, p, p, None) == -1
    # gps_tsdf_get_image(state, M, invM, type, out, stream): out may be NULL (the state's free-view image), the rest may not;
    # the image-normal type has no free-camera use
    assert lib.gps_tsdf_get_image(None, p, p, GREY, p, None) == -1
    assert lib.gps_tsdf_get_image(S, None, p, GREY, p, None) == -1
    assert lib.gps_tsdf_get_image(S, p, None, GREY, p, None) == -1
    assert lib.gps_tsdf_get_image(S, p, p, IMAGENORMALS, p, None) == -1
    bad, _k = _state(fv_raycast=None)
    assert lib.gps_tsdf_get_image(ctypes.byref(bad), p, p, GREY, None, None) == -1
    assert not keep.any() and not buf.any()


def _reference_switch(type_name, age, count):
    """ITMBasicEngine::GetImage's switch (ITMBasicEngine.tpp:400-497) -> (render type or None, ray source, output source)"""
    if type_name == "ORIGINAL_RGB":
        return None, "RAYS_NONE", "OUT_RGB"                              # :402-408
    if type_name == "ORIGINAL_DEPTH":
        return None, "RAYS_NONE", "OUT_DEPTH_COLOUR"                     # :409-415
    if type_name in ("SCENERAYCAST", "COLOUR_FROM_VOLUME", "COLOUR_FROM_NORMAL", "COLOUR_FROM_CONFIDENCE"):
        rays = "RAYS_LIVE_RAYCAST" if age <= 0 else "RAYS_FORWARD_PROJECTION"   # :423-426
        if type_name == "COLOUR_FROM_CONFIDENCE":                        # :430-443
            render = CONFIDENCE
        elif type_name == "COLOUR_FROM_NORMAL":
            render = NORMAL
        elif type_name == "COLOUR_FROM_VOLUME":
            render = VOLUME
        else:
            render = IMAGENORMALS
        return render, rays, "OUT_KF_RAYCAST" if count != 0 else "OUT_LIVE_RENDER"   # :455-459
    if type_name.startswith("FREECAMERA_"):
        render = GREY                                                    # :473-479
        if type_name == "FREECAMERA_COLOUR_FROM_VOLUME":
            render = VOLUME
        elif type_name == "FREECAMERA_COLOUR_FROM_NORMAL":
            render = NORMAL
        elif type_name == "FREECAMERA_COLOUR_FROM_CONFIDENCE":
            render = CONFIDENCE
        return render, "RAYS_FREE_RAYCAST", "OUT_FREE_RENDER"            # :486-492
    return None, "RAYS_NONE", "OUT_CLEARED"                              # :495-496, after out->Clear() (:399)


def test_decision_function_is_the_references_switch_over_the_whole_table():
    h = _host()
    from gps_slam_amd import tsdf_engine as E
    names = list(E.IMAGE_TYPE_NAMES)
    assert len(names) == 11 and names[-1] == "UNKNOWN"
    members = h.GetImageType.__members__
    assert [k for k, _ in sorted(members.items(), key=lambda kv: int(kv[1]))] == ["InfiniTAM_IMAGE_" + n for n in names]
    cells = 0
    for i, name in enumerate(names):
        t = members["InfiniTAM_IMAGE_" + name]
        assert int(t) == i == getattr(E, "InfiniTAM_IMAGE_" + name) == E.image_type_from(name) == E.image_type_from("InfiniTAM_IMAGE_" + name)
        for age in (-1, 0, 1, 6):
            for count in (0, 1, 10):
                d = h.decideOnGetImage(t, age, count)
                render, rays, out = _reference_switch(name, age, count)
                assert (d.renderType if d.renderType >= 0 else None, d.rays.name, d.out.name) == (render, rays, out), (name, age, count)
                cells += 1
    assert cells == 11 * 4 * 3
    # ... and the mirror routes the same render types
    for name in names:
        t = E.image_type_from(name)
        render = _reference_switch(name, 0, 0)[0]
        assert E._LIVE_RENDER.get(t, E._FREE_RENDER.get(t)) == render, name
    with pytest.raises(ValueError):
        E.image_type_from("SHADED")
    with pytest.raises(ValueError):
        E.image_type_from(11)


def test_host_surface_carries_get_image():
    h = _host()
    assert hasattr(h.ITMBasicEngine, "GetImage")
    from gps_slam_amd.tsdf_engine import TsdfEngine
    assert callable(TsdfEngine.GetImage)


def test_fixture_inputs_regenerate_and_hold_the_cases_the_gpu_tests_name():
    from tests import get_image_cases as cases
    from tests.digests import crc
    g = np.load(GOLD)
    assert list(g["types"]) == list(cases.TYPES) and sorted(cases.RUNS) == list(g["names"])
    for tag, (W, H, n, step, approx) in cases.RUNS.items():
        seq = cases.make_run(tag)
        assert (int(g[tag + "_W"]), int(g[tag + "_H"]), int(g[tag + "_n_frames"]), bool(g[tag + "_approx"])) == (W, H, n, approx)
        assert np.array_equal(g[tag + "_input_crc"], np.array([crc(seq["rgb"]), crc(seq["depth"]), crc(seq["c2w"])], np.uint32)), tag
        assert (seq["depth"] == 0).any(1).any(1).all()            # every frame has invalid depth pixels
        ages = g[tag + "_ages"]
        assert ((ages > 0).any() and (ages <= 0).any()) if approx else (ages <= 0).all()
        full = int(g[tag + "_full_frame"])
        assert (ages[full] > 0) == approx
        live = g[tag + "_full_live"]
        assert live.shape == (6, H, W, 4)
        for k in range(6):
            img = live[k][..., :3] if cases.TYPES[k] in cases.NORMAL_TYPES else live[k]
            assert crc(img) == g[tag + "_live_crc"][full, k]
        # the stored depth image is the transcription's answer on the frame's depth, and it shows every ramp and invalid pixels
        dep = cases.depth_to_uchar4(seq["depth"][full].astype(np.float32) * np.float32(0.001))
        assert np.array_equal(dep, live[1])
        assert all(((dep[..., c] > 0) & (dep[..., c] < 255)).any() for c in range(3)) and (dep[..., 3] == 0).any()
        # the shaded live view: drawn pixels, undrawn ones, nothing within two pixels of the border
        grey = live[2]
        assert (grey != 0).any() and (grey == 0).any() and not grey[:3].any() and not grey[-3:].any() and not grey[:, :3].any() and not grey[:, -3:].any()


def test_transcriptions_on_small_cases():
    """the numpy transcriptions the GPU tests compare the kernels with: cases whose answer is known by hand"""
    from tests import get_image_cases as cases
    assert not cases.depth_to_uchar4(np.zeros((3, 4), np.float32)).any()
    assert not cases.depth_to_uchar4(np.full((3, 4), 1.5, np.float32)).any()
    two = cases.depth_to_uchar4(np.array([1.0, 3.0, 0.0, -1.0], np.float32))
    # the ends of the scale: v = 0 -> (base(-0.5), base(0), base(0.5)) = (0.5, 1, 0.5); v = 1 -> (0.5, 0, 0)
    assert two.tolist() == [[127, 255, 127, 255], [127, 0, 0, 255], [0, 0, 0, 0], [0, 0, 0, 0]]
    # a plane facing the camera, 7 x 7: one pixel passes the border test; light = +z -> the normal (0, 0, -1) looks away ...
    ys, xs = np.meshgrid(np.arange(7, dtype=np.float32), np.arange(7, dtype=np.float32), indexing="ij")
    rays = np.stack([xs, ys, np.full_like(xs, 50.0), np.full_like(xs, 2.0)], -1)
    invM = np.eye(4, dtype=np.float32).reshape(-1)          # column 2 = (0, 0, 1): light = (0, 0, -1)
    img = cases.grey_image_normals(rays, invM, 0.02)
    assert img[3, 3].tolist() == [255] * 4 and np.count_nonzero(img.any(-1)) == 1
    flipped = invM.copy(); flipped[10] = -1.0
    assert not cases.grey_image_normals(rays, flipped, 0.02).any()
    assert not cases.grey_image_normals(rays[:6, :6], invM, 0.02).any()
