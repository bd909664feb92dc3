"""What the GetImage fixture (tests/golden/get_image.npz), its generator and its tests share (data and numpy only): the sequences
with their depth holes, the free-camera poses, the order of the GetImage calls, and float32 transcriptions of the two image
passes that need no volume -- processPixelGrey_ImageNormals and DepthToUchar4."""
import numpy as np

from tests import synth
from tests.scenes import look_at_c2w

# the order of ITMMainEngine::GetImageType; the fixture calls the first six after every frame, then the last four at each free pose
TYPES = ("ORIGINAL_RGB", "ORIGINAL_DEPTH", "SCENERAYCAST", "COLOUR_FROM_VOLUME", "COLOUR_FROM_NORMAL", "COLOUR_FROM_CONFIDENCE",
         "FREECAMERA_SHADED", "FREECAMERA_COLOUR_FROM_VOLUME", "FREECAMERA_COLOUR_FROM_NORMAL", "FREECAMERA_COLOUR_FROM_CONFIDENCE")
LIVE_TYPES, FREE_TYPES = TYPES[:6], TYPES[6:]
NORMAL_TYPES = ("COLOUR_FROM_NORMAL", "FREECAMERA_COLOUR_FROM_NORMAL")   # compared on r, g, b (drawPixelNormal leaves the alpha)

VOXEL, MU, VF_MIN, VF_MAX = 0.02, 0.08, 0.2, 10.0
# run -> (W, H, frames, step_deg, useApproximateRaycast): the sequences of the forward-render fixture; "f" is "a" with the option on
RUNS = {"a": (100, 75, 12, 0.2, False), "b": (64, 48, 8, 0.8, False), "f": (100, 75, 12, 0.2, True)}


def image_crc(type_name, img):
    """the digest the fixture stores for an image [H, W, 4] of a type: of r, g, b alone for the normal types"""
    from tests.digests import crc
    img = np.asarray(img)
    return crc(img[..., :3]) if type_name in NORMAL_TYPES else crc(img)


def same_image(type_name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    return np.array_equal(got[..., :3], want[..., :3]) if type_name in NORMAL_TYPES else np.array_equal(got, want)


def punch_holes(depth):
    """depth [n, H, W] -> a copy with invalid (0) pixels: synth's room is closed, every ray of it has a depth.  A rectangle that
    moves with the frame and a sparse lattice."""
    d = depth.copy()
    n, H, W = d.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for f in range(n):
        x0, y0 = W // 5 + 2 * f, H // 2 + f
        d[f, y0:y0 + H // 8, x0:x0 + W // 10] = 0
        d[f][(xs * 7 + ys * 13 + f * 3) % 97 == 0] = 0
    return d


def make_run(tag):
    """-> synth sequence dict of the run with holes punched into the depth"""
    W, H, n, step, _ = RUNS[tag]
    seq = synth.make_sequence(W, H, n, step_deg=step)
    seq["depth"] = punch_holes(seq["depth"])
    return seq


def free_poses(c2w):
    """the two free cameras after a frame at c2w: the frame's camera turned 12 degrees about its y axis and moved by
    (0.15, -0.05, 0.10) m in its own frame; and a camera elsewhere in the room that sees surfaces nobody has fused yet"""
    a = np.deg2rad(12.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[:3, 3] = [0.15, -0.05, 0.10]
    near = (np.asarray(c2w, np.float64) @ T).astype(np.float32)
    far = look_at_c2w((1.6, -0.3, -1.9), (0.3, 0.1, 0.9))
    return [near, far]


def _base(v):
    """base() (ITMVisualisationEngine.cpp:11-17) == baseCol (ITMVisualisationEngine_Shared.h:351-363), float32"""
    f = np.float32
    v = v.astype(f)
    up = (v - f(-0.75)) * f(1.0) / f(0.5) + f(0.0)
    down = (v - f(0.25)) * f(-1.0) / f(0.5) + f(1.0)
    return np.where(v <= f(-0.75), f(0), np.where(v <= f(-0.25), up, np.where(v <= f(0.25), f(1), np.where(v <= f(0.75), down, f(0))))).astype(f)


def depth_to_uchar4(depth):
    """IITMVisualisationEngine::DepthToUchar4 (ITMVisualisationEngine.cpp:19-57), float32 operation for operation -> uint8 [..., 4]"""
    f = np.float32
    d = np.asarray(depth, f)
    out = np.zeros(d.shape + (4,), np.uint8)
    ok = d > 0
    if not ok.any():
        return out
    lo, hi = d[ok].min(), d[ok].max()
    if lo == hi:
        return out
    scale = f(1.0) / (hi - lo)
    v = (np.where(ok, d, lo) - lo) * scale
    for c, off in enumerate((f(-0.5), f(0.0), f(0.5))):
        out[..., c] = np.where(ok, (_base(v + off) * f(255.0)).astype(np.uint8), 0)
    out[..., 3] = np.where(ok, 255, 0)
    return out


def grey_image_normals(rays, invM, voxel_size, stats=None):
    """processPixelGrey_ImageNormals<true, false> (ITMVisualisationEngine_Shared.h:257-344, 482-499) over a ray image [H, W, 4],
    float32 operation for operation, pixel by pixel -> uint8 [H, W, 4].  Every neighbour read goes through an index check: a read
    outside the image raises.  stats (a dict): pixels that took the +-1 fallback and were kept / rejected, and how often the
    length test fired."""
    f = np.float32
    r = np.asarray(rays, f)
    H, W = r.shape[:2]
    invM = np.asarray(invM, f).reshape(-1)
    light = (-invM[8], -invM[9], -invM[10])
    vs = f(voxel_size)
    out = np.zeros((H, W, 4), np.uint8)
    st = dict(fallback_kept=0, fallback_rejected=0, length_fired=0, border=0, angle_rejected=0)

    def at(x, y):
        assert 0 <= x < W and 0 <= y < H, ("neighbour read outside the image", x, y)
        return r[y, x]

    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if not r[y, x, 3] > 0:
                    continue
                if y <= 2 or y >= H - 3 or x <= 2 or x >= W - 3:
                    st["border"] += 1
                    continue
                xp, yp, xm, ym = at(x + 2, y), at(x, y + 2), at(x - 2, y), at(x, y - 2)
                plus1 = False
                if xp[3] <= 0 or yp[3] <= 0 or xm[3] <= 0 or ym[3] <= 0:
                    plus1 = True
                else:
                    dx, dy = xp - xm, yp - ym
                    la = dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]
                    lb = dy[0] * dy[0] + dy[1] * dy[1] + dy[2] * dy[2]
                    ld = lb if la < lb else la
                    if ld * vs * vs > f(0.15) * f(0.15):
                        plus1 = True
                        st["length_fired"] += 1
                if plus1:
                    xp, yp, xm, ym = at(x + 1, y), at(x, y + 1), at(x - 1, y), at(x, y - 1)
                    dx, dy = xp - xm, yp - ym
                    if xp[3] <= 0 or yp[3] <= 0 or xm[3] <= 0 or ym[3] <= 0:
                        st["fallback_rejected"] += 1
                        continue
                nx = -(dx[1] * dy[2] - dx[2] * dy[1])
                ny = -(dx[2] * dy[0] - dx[0] * dy[2])
                nz = -(dx[0] * dy[1] - dx[1] * dy[0])
                ns = f(1.0) / np.sqrt(nx * nx + ny * ny + nz * nz, dtype=f)
                nx, ny, nz = nx * ns, ny * ns, nz * ns
                angle = nx * light[0] + ny * light[1] + nz * light[2]
                if not angle > 0.0:
                    st["angle_rejected"] += 1
                    if plus1:
                        st["fallback_rejected"] += 1
                    continue
                if plus1:
                    st["fallback_kept"] += 1
                out[y, x, :] = np.uint8((f(0.8) * angle + f(0.2)) * f(255.0))
    if stats is not None:
        stats.update(st)
    return out
