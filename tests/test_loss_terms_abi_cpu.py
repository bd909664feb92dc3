"""The loss-terms fields of gps_splat_step and the two gps_loss_terms exports on the C ABI, host side only: the ctypes mirror lays
the new fields out where the header declares them."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("ssim_weight", "depth_weight", "ref_depth_raw", "gt_depth", "depth", "loss_terms", "loss_ws")


def _header_struct_fields():
    """(name, is_pointer, C type) of every member of gps_splat_step, in declaration order"""
    txt = open(os.path.join(ROOT, "include", "gps_slam_hip.h")).read()
    end = txt.index("} gps_splat_step;")
    body = re.sub(r"/\*.*?\*/", "", txt[txt.rindex("typedef struct {", 0, end) + len("typedef struct {"):end], flags=re.S)
    out = []
    for decl in body.split(";"):
        m = re.match(r"\s*(const\s+)?(\w+)\s+(.*)", decl.strip(), flags=re.S)
        if not m:
            continue
        for item in m.group(3).split(","):
            item = item.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", item)
            out.append((arr.group(1) if arr else item.lstrip("*"), item.startswith("*"), m.group(2), int(arr.group(2)) if arr else 0))
    return out


def test_struct_mirror_has_the_loss_fields_at_the_headers_offsets():
    from gps_slam_amd._lib import SplatStep
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
    hdr = _header_struct_fields()
    # the header's layout, as a C compiler lays it out (natural alignment)
    hdr_struct = type("Hdr", (C.Structure,), {"_fields_": [
        (n, C.c_void_p if ptr else (ctype[t] * k if k else ctype[t])) for n, ptr, t, k in hdr]})
    names = [n for n, *_ in hdr]
    assert [f[0] for f in SplatStep._fields_] == names
    for f in FIELDS:
        assert f in names, f
        assert getattr(SplatStep, f).offset == getattr(hdr_struct, f).offset, f
        assert getattr(SplatStep, f).size == getattr(hdr_struct, f).size, f
    assert C.sizeof(SplatStep) == C.sizeof(hdr_struct)
    d = dict(SplatStep._fields_)
    assert d["ssim_weight"] is C.c_float and d["depth_weight"] is C.c_float
    # zero-initialised = off
    st = SplatStep()
    assert st.ssim_weight == 0.0 and st.depth_weight == 0.0 and not st.gt_depth and not st.loss_ws


def test_the_two_exports_are_declared_and_exported():
    from gps_slam_amd import _build, _lib
    assert "gps_loss_terms" in _lib.PROTOTYPES and "gps_loss_terms_workspace_floats" in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["gps_loss_terms"][1]) == 21
    _build.build()
    lib = _lib.load_library()
    tiles = lambda w, h: ((w + 31) // 32) * ((h + 31) // 32)
    for w, h in ((640, 480), (37, 50), (1200, 680)):   # per-tile, per-channel rows of 4 partial sums + the SSIM backward's 9 maps
        assert lib.gps_loss_terms_workspace_floats(w, h) == 12 * tiles(w, h) + 9 * w * h
    assert lib.gps_loss_terms_workspace_floats(0, 48) == 0


def test_oracle_inputs_of_the_gpu_cases_stay_under_the_exclusion_cap():
    """tests/test_loss_terms_gpu.py leaves pixels out of its gradient comparison whose L1 sign (|gt - rgb| < 1e-6) or depth validity
    (|depth| < 1e-6) the float64 oracle itself decides within rounding: at most 0.1 % of the pixels, for the seeded inputs of
    every case, and the inputs carry the edges the cases are about (holes in ref_depth, a block of zeros in gt_depth)."""
    from tests.test_loss_terms_gpu import SIZES, WEIGHTS, _case, _excluded
    for W, H in SIZES:
        for s, d in WEIGHTS:
            (rc, ws, base, ref, gt, gtd), o = _case(W, H, s, d)
            ex = _excluded(o, gt, d)
            assert int(ex.sum()) <= 1e-3 * W * H, (W, H, s, d, int(ex.sum()))
            assert bool(((gtd > 0) & (o["depth"] > 0)).any()) and bool((gtd == 0).any()) and bool((ref == 0).any())
            assert bool(o["terms"].isfinite().all()) and bool(o["v_rc"].isfinite().all()) and bool(o["v_ra"].isfinite().all())
