"""ITMRGBDCalib on the host (ITMLib/Objects/Camera/*): two intrinsics, trafo_rgb_to_depth with its inverse, the disparity
calibration, and the text format of ITMCalibIO.cpp.  Everything is float32, computed in the reference's operation order."""
import ctypes as C

import numpy as np

from ._lib import DEPTH_CALIB_AFFINE, DEPTH_CALIB_KINECT, ColourCamera, DepthCalib

TRAFO_KINECT, TRAFO_AFFINE = DEPTH_CALIB_KINECT, DEPTH_CALIB_AFFINE   # ITMDisparityCalib::TrafoType
_f = np.float32


class Intrinsics:
    """ITMIntrinsics: imgSize and projectionParamsSimple"""

    def __init__(self, width=640, height=480, fx=580.0, fy=580.0, cx=320.0, cy=240.0):
        self.SetFrom(width, height, fx, fy, cx, cy)

    def SetFrom(self, width, height, fx, fy, cx, cy):
        self.width, self.height = int(width), int(height)
        self.fx, self.fy, self.cx, self.cy = (float(_f(v)) for v in (fx, fy, cx, cy))

    def params(self):
        return self.fx, self.fy, self.cx, self.cy

    def __eq__(self, o):
        return (self.width, self.height) + self.params() == (o.width, o.height) + o.params()


class DisparityCalib:
    """ITMDisparityCalib: the standard calibration is affine, 1 / 1000, 0"""

    def __init__(self):
        self.SetStandard()

    def GetType(self):
        return self.type

    def GetParams(self):
        return self.a, self.b

    def SetFrom(self, a, b, trafo_type):
        a, b = float(_f(a)), float(_f(b))
        if a != 0.0 or b != 0.0:
            if trafo_type not in (TRAFO_KINECT, TRAFO_AFFINE):
                raise ValueError("DisparityCalib: unknown type %r" % (trafo_type,))
            self.a, self.b, self.type = a, b, int(trafo_type)
        else:
            self.SetStandard()

    def SetStandard(self):
        self.SetFrom(_f(1.0) / _f(1000.0), 0.0, TRAFO_AFFINE)

    def is_standard(self):
        return self.type == TRAFO_AFFINE and self.a == float(_f(1.0) / _f(1000.0)) and self.b == 0.0

    def as_struct(self):
        return DepthCalib(self.type, self.a, self.b)

    def __eq__(self, o):
        return (self.type, self.a, self.b) == (o.type, o.a, o.b)


class Extrinsics:
    """ITMExtrinsics: calib (colour camera -> depth camera) and calib_inv, float32[16] in ORUtils layout m[col * 4 + row]"""

    def __init__(self):
        self.SetFrom(np.eye(4, dtype=_f).reshape(16))

    def SetFrom(self, calib16):
        m = np.array(calib16, dtype=_f).reshape(16)
        inv = np.zeros(16, _f)
        inv[0] = inv[5] = inv[10] = inv[15] = _f(1.0)
        for r in range(3):
            for c in range(3):
                inv[r + 4 * c] = m[c + 4 * r]
        for r in range(3):   # ITMExtrinsics.h:36-40: three subtractions from 0
            dest = _f(0.0)
            for c in range(3):
                dest = _f(dest - _f(m[c + 4 * r] * m[c + 12]))
            inv[r + 12] = dest
        self.calib, self.calib_inv = m, inv

    def __eq__(self, o):
        return np.array_equal(self.calib, o.calib) and np.array_equal(self.calib_inv, o.calib_inv)


class RGBDCalib:
    """ITMRGBDCalib"""

    def __init__(self):
        self.intrinsics_rgb, self.intrinsics_d = Intrinsics(), Intrinsics()
        self.trafo_rgb_to_depth = Extrinsics()
        self.disparityCalib = DisparityCalib()

    def __eq__(self, o):
        return (self.intrinsics_rgb == o.intrinsics_rgb and self.intrinsics_d == o.intrinsics_d and
                self.trafo_rgb_to_depth == o.trafo_rgb_to_depth and self.disparityCalib == o.disparityCalib)

    def colour_camera(self, rgb_ptr=None):
        """gps_colour_camera of the colour camera (the image pointer is filled in per frame)"""
        k = self.intrinsics_rgb
        cam = ColourCamera()
        cam.width, cam.height = k.width, k.height
        cam.fx, cam.fy, cam.cx, cam.cy = k.params()
        cam.depth_to_rgb[:] = self.trafo_rgb_to_depth.calib_inv.tolist()
        cam.rgb = rgb_ptr
        return cam


def m_rgb(calib_inv16, M_d16):
    """M_rgb = calib_inv * M_d, ORUtils' Matrix4 * Matrix4 (gps_rgbd_m_rgb: float, on the host)"""
    from ._lib import check, lib
    a = np.ascontiguousarray(calib_inv16, dtype=_f)
    b = np.ascontiguousarray(M_d16, dtype=_f)
    out = np.zeros(16, _f)
    check(lib.gps_rgbd_m_rgb(a.ctypes.data, b.ctypes.data, out.ctypes.data), "gps_rgbd_m_rgb")
    return out


# ---------------------------------------------------------------- ITMCalibIO.cpp
def _tokens(text):
    return text.split()


def _float(tok):
    return float(_f(float(tok)))


def _read_intrinsics(t, pos):
    w, h = int(t[pos]), int(t[pos + 1])
    fx, fy, cx, cy = (_float(v) for v in t[pos + 2:pos + 6])
    return Intrinsics(w, h, fx, fy, cx, cy), pos + 6


def _read_extrinsics(t, pos):
    rows = [[_float(v) for v in t[pos + 4 * r:pos + 4 * r + 4]] for r in range(3)]
    if any(len(r) != 4 for r in rows):
        raise ValueError("calibration: truncated extrinsics")
    m = np.zeros(16, _f)
    for r in range(3):
        for c in range(4):
            m[c * 4 + r] = rows[r][c]
    m[15] = 1.0
    e = Extrinsics()
    e.SetFrom(m)
    return e, pos + 12


def _read_disparity(t, pos):
    word = t[pos]
    trafo = TRAFO_KINECT
    if word == "kinect":
        a, pos = _float(t[pos + 1]), pos + 2
    elif word == "affine":
        trafo = TRAFO_AFFINE
        a, pos = _float(t[pos + 1]), pos + 2
    else:
        a, pos = _float(word), pos + 1
    b = _float(t[pos])
    d = DisparityCalib()
    if a == 0.0 and b == 0.0:
        d.SetStandard()
    else:
        d.SetFrom(a, b, trafo)
    return d, pos + 1


def parse_rgbd_calib(text):
    """readRGBDCalib(std::istream &): colour intrinsics, depth intrinsics, extrinsics, disparity calibration"""
    t = _tokens(text)
    c = RGBDCalib()
    try:
        c.intrinsics_rgb, pos = _read_intrinsics(t, 0)
        c.intrinsics_d, pos = _read_intrinsics(t, pos)
        c.trafo_rgb_to_depth, pos = _read_extrinsics(t, pos)
        c.disparityCalib, pos = _read_disparity(t, pos)
    except (IndexError, ValueError) as e:
        raise ValueError("calibration: cannot read it (%s)" % e)
    return c


def read_rgbd_calib(file_name):
    with open(file_name) as f:
        return parse_rgbd_calib(f.read())


def _g(v):
    return "%g" % float(_f(v))   # operator<<(float) at the stream's default precision


def format_rgbd_calib(c):
    """writeRGBDCalib's bytes"""
    intr = lambda k: "%d %d\n%s %s\n%s %s\n" % (k.width, k.height, _g(k.fx), _g(k.fy), _g(k.cx), _g(k.cy))
    m = c.trafo_rgb_to_depth.calib
    ext = "".join("%s %s %s %s\n" % (_g(m[r]), _g(m[4 + r]), _g(m[8 + r]), _g(m[12 + r])) for r in range(3))
    d = c.disparityCalib
    disp = ("affine %s %s\n" if d.type == TRAFO_AFFINE else "%s %s\n") % (_g(d.a), _g(d.b))
    return intr(c.intrinsics_rgb) + "\n" + intr(c.intrinsics_d) + "\n" + ext + "\n" + disp


def write_rgbd_calib(file_name, c):
    with open(file_name, "w") as f:
        f.write(format_rgbd_calib(c))


def register_colour(depth_f, intrinsics_d, calib, rgb_u8):
    """Colour registered to the depth camera (gps_tsdf_register_colour; ours, not the reference's): depth_f float32 [Hd, Wd]
    device tensor in metres (<= 0 invalid), intrinsics_d (fx, fy, cx, cy), calib an RGBDCalib (its colour camera and extrinsics
    are used), rgb_u8 uint8 [Hc, Wc, 4] device tensor -> uint8 [Hd, Wd, 4], alpha 255 where a colour was found, 0 0 0 0
    elsewhere.  One launch on the current stream, no host read."""
    import torch
    from ._lib import TsdfState, check, lib
    assert depth_f.dtype == torch.float32 and depth_f.is_contiguous() and rgb_u8.dtype == torch.uint8 and rgb_u8.is_contiguous()
    k = calib.intrinsics_rgb
    assert tuple(rgb_u8.shape) == (k.height, k.width, 4), "register_colour: the colour image is not of the calibration's size"
    Hd, Wd = depth_f.shape
    s = TsdfState()
    s.width, s.height = Wd, Hd
    s.fx, s.fy, s.cx, s.cy = (float(v) for v in intrinsics_d)
    s.depth = depth_f.data_ptr()
    cam = calib.colour_camera(rgb_u8.data_ptr())
    out = torch.empty((Hd, Wd, 4), dtype=torch.uint8, device=depth_f.device)
    stream = C.c_void_p(torch.cuda.current_stream(depth_f.device).cuda_stream)
    check(lib.gps_tsdf_register_colour(C.byref(s), C.byref(cam), out.data_ptr(), stream), "gps_tsdf_register_colour")
    return out
