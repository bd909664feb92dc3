"""Per-frame exposure on the C ABI, host side only: the trailing fields of gps_splat_step as both hosts lay them out, and the slab
size the train step and gps_exposure_bwd share."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_splat_step_ends_with_the_exposure_fields_in_header_order():
    from gps_slam_amd._lib import SplatStep
    txt = open(os.path.join(ROOT, "include", "gps_slam_hip.h")).read()
    body = txt[txt.index("int32_t preprocessed;"):txt.index("} gps_splat_step;")]
    declared = re.findall(r"\*?(exposure\w*)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    names = [f[0] for f in SplatStep._fields_]
    assert names[names.index("preprocessed") + 1:] == declared
    assert dict(SplatStep._fields_)["exposure_lr"] is C.c_double


def test_slab_covers_the_tiles_and_the_operator_backward():
    from gps_slam_amd import _build, _lib
    _build.build()
    lib = _lib.load_library()
    assert lib.gps_exposure_slab_floats(640, 480) == 12 * 1200        # 40 x 30 tiles
    assert lib.gps_exposure_slab_floats(1200, 680) == 12 * 75 * 43
    assert lib.gps_exposure_slab_floats(64, 48) == 12 * 1024          # GPS_EXPOSURE_BWD_PARTIALS
    assert lib.gps_exposure_slab_floats(0, 48) == 0
