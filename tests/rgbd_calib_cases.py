"""What the RGB-D calibration fixture (tests/golden/rgbd_calib.npz), its generator and its tests share (data and numpy only): the
runs with a colour camera of its own and with calibrated depth, the conversion-only images, and float32 transcriptions of
ITMExtrinsics::SetFrom, ORUtils' Matrix4 * Matrix4, the two depth conversions (ITMViewBuilder_Shared.h:8-36), the calib.txt
format (ITMCalibIO.cpp) and of OUR colour registration (gps_tsdf_register_colour; the reference has none)."""
import numpy as np

from tests import synth

VOXEL, MU, VF_MIN, VF_MAX = 0.02, 0.08, 0.2, 10.0
KINECT, AFFINE = 0, 1   # ITMDisparityCalib::TrafoType


def _six(v):
    """a value the reference's text format keeps: six significant digits, as float32"""
    return np.float32(float("%.6g" % float(v)))


def _extrinsics(rot_deg, t):
    """trafo_rgb_to_depth.calib (points of the colour camera -> the depth camera), 4 x 4 float32 with entries of six digits:
    a rotation by rot_deg = (rx, ry, rz) degrees and a translation t in metres"""
    rx, ry, rz = np.deg2rad(np.asarray(rot_deg, np.float64))
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    T = np.eye(4, dtype=np.float32)
    R = Rz @ Ry @ Rx
    for r in range(3):
        for c in range(3):
            T[r, c] = _six(R[r, c])
        T[r, 3] = _six(t[r])
    return T


IDENT = np.eye(4, dtype=np.float32)
# run -> depth size, colour size, colour focal length (None: the depth camera's intrinsics), extrinsics, depth calibration
# (type, a, b), frames, orbit step, bilateral filter, given | track
RUNS = {
    "wide": dict(d=(64, 48), c=(96, 60), fc=40.0, ext=_extrinsics((0.5, -1.0, 0.3), (0.025, 0.004, -0.003)), calib=(AFFINE, 0.001, 0.0),
                 n=6, step=0.8, filt=False, mode="given"),
    "narrow": dict(d=(64, 48), c=(48, 36), fc=48.0, ext=_extrinsics((-0.4, 0.8, 0.0), (-0.03, 0.002, 0.005)), calib=(AFFINE, 0.001, 0.0),
                   n=6, step=0.8, filt=False, mode="given"),
    "kinect": dict(d=(64, 48), c=(64, 48), fc=None, ext=IDENT, calib=(KINECT, 1090.0, 3.0), n=6, step=0.8, filt=False, mode="given"),
    "tum": dict(d=(64, 48), c=(64, 48), fc=None, ext=IDENT, calib=(AFFINE, 0.0002, 0.01), n=6, step=0.8, filt=False, mode="given"),
    "filtered": dict(d=(64, 48), c=(64, 48), fc=None, ext=IDENT, calib=(AFFINE, 0.0002, 0.01), n=6, step=0.8, filt=True, mode="given"),
    # tracked: 160 x 120 -- below that the reference's own tracker answers NaN poses on this scene (64 x 48 included), as the
    # bilateral fixture found.  The step of 2.4 degrees is the generator's choice by ITS condition on the reference alone: the
    # reference's tracked poses must be defined well inside the tracker's bound of 2e-5, i.e. move by less than a quarter of it
    # when one raw pixel per frame changes by one unit (make_rgbd_calib_golden.tracked_sensitivity).  Measured on the reference's
    # CPU engine, worst frame of three seeded trials: step 0.4: 4.8e-5 (frame 3), 0.8: 7.3e-6, 1.2: 5.5e-6, 1.6: 1.2e-5,
    # 2.0: 3.7e-4, 2.4: 4.3e-6, 3.0: 1.6e-4, 4.0: 6.3e-6; 200 x 150 at 0.4: 3.1e-5 -- the reference's LM loop takes another branch
    # for such a change, and a pose that the reference itself does not hold to 2e-5 cannot be asked of the device to 2e-5
    "tum_t": dict(d=(160, 120), c=(160, 120), fc=None, ext=IDENT, calib=(AFFINE, 0.0002, 0.01), n=6, step=2.4, filt=False, mode="track"),
    # a second tracked orbit that meets the same condition (2.2 degrees: 3.7e-6 in its worst frame; further steps measured, worst
    # frame: 0.6: 1.4e-5, 1.0: 7.6e-6, 2.6: 1.5e-5, 2.8: 4.5e-4, 3.2: 6.4e-6, 3.6: 7.0e-6), so that one orbit is not the only evidence
    "tum_t2": dict(d=(160, 120), c=(160, 120), fc=None, ext=IDENT, calib=(AFFINE, 0.0002, 0.01), n=6, step=2.2, filt=False, mode="track"),
}
TWO_CAMERA_RUNS = ("wide", "narrow")
TRACKED_RUNS = ("tum_t", "tum_t2")
# conversion-only images: (W, H), both types each
CONV_SIZES = {"c5x5": (5, 5), "c67x3": (67, 3), "c100x52": (100, 52)}
CONV_CALIBS = {"affine": (AFFINE, 0.0002, 0.01), "kinect": (KINECT, 1090.0, 3.0)}
CONV_FX = 57.5   # intrinsics_d.fx of the conversion-only cases (the Kinect formula reads it)


def conv_raw(size_tag, calib_tag):
    """-> int16 [H, W] raw image of a conversion-only case: a tilted plane with seeded noise and, in scan order from pixel 0,
    the special values of its type (affine: 0, negative, 1, 32767; Kinect: a itself (t == 0), above a (depth < 0), 0, negative,
    32767)"""
    W, H = CONV_SIZES[size_tag]
    rng = np.random.default_rng(7000 + W * 100 + H)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    typ, a, b = CONV_CALIBS[calib_tag]
    if typ == AFFINE:
        d = 5000 + 31 * xs + 17 * ys + rng.integers(-40, 41, (H, W))
        special = [0, -7, 1, 32767, 0]
    else:
        d = 300 + 5 * xs + 3 * ys + rng.integers(-4, 5, (H, W))
        special = [int(a), int(a) + 9, 0, -20, 32767, int(a)]
    d = d.reshape(-1)
    for k, v in enumerate(special):
        d[(k * 5 + 1) % d.size] = v
    return d.reshape(H, W).astype(np.int16)


def convert(raw, typ, a, b, fx_d):
    """UpdateView's conversion, float32 operation for operation -> float32 [H, W]"""
    f = np.float32
    d = np.asarray(raw, np.int16).astype(f)
    a, b, fx_d = f(a), f(b), f(fx_d)
    with np.errstate(all="ignore"):
        if typ == AFFINE:
            return np.where(np.asarray(raw) <= 0, f(-1.0), d * a + b).astype(f)
        t = a - d
        depth = np.where(t == 0, f(0.0), (f(8.0) * b * fx_d) / t).astype(f)
        return np.where(depth > 0, depth, f(-1.0)).astype(f)


def convert_fused(raw, a, b):
    """what a contracted affine conversion would give: d * a + b rounded once"""
    d = np.asarray(raw, np.int16).astype(np.float64)
    v = (d * np.float64(np.float32(a)) + np.float64(np.float32(b))).astype(np.float32)   # (the product is exact in double)
    return np.where(np.asarray(raw) <= 0, np.float32(-1.0), v).astype(np.float32)


def punch_holes(depth):
    """depth [n, H, W] -> (copy with the holes at 0, mask of the rectangle, mask of the lattice): a rectangle that moves with
    the frame and a sparse lattice (synth's room is closed: every ray of it has a depth)"""
    d = depth.copy()
    n, H, W = d.shape
    rect, lat = np.zeros(d.shape, bool), np.zeros(d.shape, bool)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for f in range(n):
        x0, y0 = W // 5 + 2 * f, H // 2 + f
        rect[f, y0:y0 + H // 8, x0:x0 + W // 10] = True
        lat[f] = (xs * 7 + ys * 13 + f * 3) % 97 == 0
    d[rect | lat] = 0
    return d, rect, lat & ~rect


def intrinsics(tag):
    """-> (depth (fx, fy, cx, cy), colour (fx, fy, cx, cy)) of a run, every value of six digits"""
    r = RUNS[tag]
    (Wd, Hd), (Wc, Hc) = r["d"], r["c"]
    fd = 0.5 * Wd
    d = (fd, fd, (Wd - 1) / 2.0, (Hd - 1) / 2.0)
    c = d if r["fc"] is None else (r["fc"], r["fc"], (Wc - 1) / 2.0 + 0.25, (Hc - 1) / 2.0 - 0.5)
    return tuple(float(_six(v)) for v in d), tuple(float(_six(v)) for v in c)


def make_run(tag, same_camera=False):
    """-> dict of a run's inputs: Wd, Hd, Wc, Hc, intr_d, intr_c, ext (calib, 4 x 4 float32), calib (type, a, b), n, filt, mode,
    rgb uint8 [n, Hc, Wc, 4] rendered from the COLOUR camera's pose c2w_d @ ext, raw int16 [n, Hd, Wd] in the run's raw unit,
    c2w float32 [n, 4, 4] of the depth camera.  same_camera: the same depth and poses with the colour camera on the depth
    camera (the run the generator compares the two-camera volumes with)."""
    r = RUNS[tag]
    (Wd, Hd), (Wc, Hc) = r["d"], r["c"]
    intr_d, intr_c = intrinsics(tag)
    ext = r["ext"]
    if same_camera:
        Wc, Hc, intr_c, ext = Wd, Hd, intr_d, IDENT
    poses = synth.orbit_poses(r["n"], step_deg=r["step"])
    depth_mm, rgb = [], []
    for p in poses:
        depth_mm.append(synth.render_rgbd(p, *intr_d, Wd, Hd)[1])
        c = synth.render_rgbd(np.asarray(p, np.float64) @ ext.astype(np.float64), *intr_c, Wc, Hc)[0]
        rgb.append(np.concatenate([c, np.full((Hc, Wc, 1), 255, np.uint8)], -1))
    mm, rect, lat = punch_holes(np.stack(depth_mm).astype(np.int64))
    typ, a, b = r["calib"]
    z = mm / 1000.0
    with np.errstate(all="ignore"):
        if typ == AFFINE:
            raw = np.where(mm > 0, np.round((z - float(np.float32(b))) / float(np.float32(a))), 0)
        else:   # disparity; the rectangle is raw == a (t == 0), the lattice above a (a negative depth)
            raw = np.where(mm > 0, np.round(a - 8.0 * b * intr_d[0] / z), 0)
            raw[rect] = a
            raw[lat] = a + 10
    raw = np.clip(raw, -32768, 32767).astype(np.int16)
    return dict(Wd=Wd, Hd=Hd, Wc=Wc, Hc=Hc, intr_d=intr_d, intr_c=intr_c, ext=ext, calib=(typ, float(a), float(b)), n=r["n"],
                filt=r["filt"], mode=r["mode"], rgb=np.stack(rgb), raw=raw, c2w=np.stack(poses).astype(np.float32))


# ---------------------------------------------------------------- float32 transcriptions (ORUtils layout: m[col * 4 + row])
def to_orutils(T):
    """4 x 4 (row, col) -> float32[16] in ORUtils layout"""
    return np.ascontiguousarray(np.asarray(T, np.float32).T).reshape(16)


def calib_inv(calib16):
    """ITMExtrinsics::SetFrom (ITMExtrinsics.h:28-40): the transpose of the rotation, and -(R^T t) as three subtractions from 0"""
    f = np.float32
    m = np.asarray(calib16, f)
    inv = np.zeros(16, f)
    inv[0] = inv[5] = inv[10] = inv[15] = f(1.0)
    for r in range(3):
        for c in range(3):
            inv[r + 4 * c] = m[c + 4 * r]
    for r in range(3):
        dest = f(0.0)
        for c in range(3):
            dest = f(dest - f(m[c + 4 * r] * m[c + 12]))
        inv[r + 12] = dest
    return inv


def mat_mul(lhs16, rhs16):
    """ORUtils Matrix4 * Matrix4 (Matrix.h:117-123): r(x, y) = ((((0 + l(0,y) r(x,0)) + l(1,y) r(x,1)) + ...), float32"""
    f = np.float32
    l, r = np.asarray(lhs16, f), np.asarray(rhs16, f)
    out = np.zeros(16, f)
    for x in range(4):
        for y in range(4):
            acc = f(0.0)
            for k in range(4):
                acc = f(acc + f(l[k * 4 + y] * r[x * 4 + k]))
            out[x * 4 + y] = acc
    return out


def register_colour(depth_f, intr_d, inv16, intr_c, rgb):
    """OUR registration (gps_tsdf_register_colour), float32 operation for operation: depth_f float32 [Hd, Wd], rgb uint8
    [Hc, Wc, 4] -> uint8 [Hd, Wd, 4]"""
    f = np.float32
    depth_f = np.asarray(depth_f, f)
    Hd, Wd = depth_f.shape
    Hc, Wc = rgb.shape[:2]
    fx, fy, cx, cy = (f(v) for v in intr_d)
    fxc, fyc, cxc, cyc = (f(v) for v in intr_c)
    m = np.asarray(inv16, f)
    ys, xs = np.meshgrid(np.arange(Hd, dtype=f), np.arange(Wd, dtype=f), indexing="ij")
    with np.errstate(all="ignore"):
        z = depth_f
        X = z * ((xs - cx) / fx)
        Y = z * ((ys - cy) / fy)
        one = f(1.0)
        px = ((m[0] * X + m[4] * Y) + m[8] * z) + m[12] * one
        py = ((m[1] * X + m[5] * Y) + m[9] * z) + m[13] * one
        pz = ((m[2] * X + m[6] * Y) + m[10] * z) + m[14] * one
        u = fxc * px / pz + cxc
        v = fyc * py / pz + cyc
        ok = (z > 0) & (pz > 0) & (u >= 1) & (u <= Wc - 2) & (v >= 1) & (v <= Hc - 2)
        u, v = np.where(ok, u, one), np.where(ok, v, one)
        qx, qy = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        dx, dy = (u - qx.astype(f)).astype(f), (v - qy.astype(f)).astype(f)
        src = rgb[..., :3].astype(f)
        a = src[qy, qx]
        b = np.where((dx != 0)[..., None], src[qy, qx + 1], f(0))
        c = np.where((dy != 0)[..., None], src[qy + 1, qx], f(0))
        d = np.where(((dx != 0) & (dy != 0))[..., None], src[qy + 1, qx + 1], f(0))
        dx, dy = dx[..., None], dy[..., None]
        val = ((a * (one - dx) * (one - dy) + b * dx * (one - dy)) + c * (one - dx) * dy) + d * dx * dy
        byte = np.clip((val + f(0.5)).astype(np.int64), 0, 255).astype(np.uint8)
    out = np.zeros((Hd, Wd, 4), np.uint8)
    out[..., :3] = np.where(ok[..., None], byte, 0)
    out[..., 3] = np.where(ok, 255, 0)
    return out


def exact_shift_case():
    """a fronto-parallel plane at 2 m seen by two cameras with focal length 32 and whole-pixel principal points, the colour
    camera translated so that the image moves by (+4, +2) pixels: every intermediate of the registration is exact in float32.
    -> (depth_f [48, 64], intr_d, inv16, intr_c, rgb [48, 64, 4], expected [48, 64, 4])"""
    Wd, Hd = 64, 48
    intr = (32.0, 32.0, 32.0, 24.0)
    depth_f = np.full((Hd, Wd), 2.0, np.float32)
    depth_f[5, 7] = -1.0     # an invalid pixel
    inv = np.eye(4, dtype=np.float32)
    inv[0, 3], inv[1, 3] = 0.25, 0.125   # u = 32 (X + 0.25) / 2 + 32 = x + 4; v = y + 2
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (Hd, Wd, 4)).astype(np.uint8)
    rgb[..., 3] = 255
    want = np.zeros((Hd, Wd, 4), np.uint8)
    for y in range(Hd):
        for x in range(Wd):
            u, v = x + 4, y + 2
            if depth_f[y, x] > 0 and 1 <= u <= Wd - 2 and 1 <= v <= Hd - 2:
                want[y, x, :3] = rgb[v, u, :3]
                want[y, x, 3] = 255
    return depth_f, intr, to_orutils(inv), intr, rgb, want


# ---------------------------------------------------------------- calib.txt (ITMCalibIO.cpp)
def _g(v):
    return "%g" % float(np.float32(v))   # operator<<(float) with the stream's default precision of six


def calib_text(Wc, Hc, intr_c, Wd, Hd, intr_d, calib16, typ, a, b):
    """writeRGBDCalib's text"""
    m = np.asarray(calib16, np.float32)
    intr = lambda W, H, k: "%d %d\n%s %s\n%s %s\n" % (W, H, _g(k[0]), _g(k[1]), _g(k[2]), _g(k[3]))
    ext = "".join("%s %s %s %s\n" % (_g(m[r]), _g(m[4 + r]), _g(m[8 + r]), _g(m[12 + r])) for r in range(3))
    disp = ("affine %s %s\n" if typ == AFFINE else "%s %s\n") % (_g(a), _g(b))
    return intr(Wc, Hc, intr_c) + "\n" + intr(Wd, Hd, intr_d) + "\n" + ext + "\n" + disp
