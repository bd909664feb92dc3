"""Seeded synthetic inputs shared by the oracle tests and the GPU parity tests (data only)."""
import numpy as np


def look_at_c2w(eye, target, up=(0.0, -1.0, 0.0)):
    """OpenCV-style camera (x right, y down, z forward) -> 4x4 camera-to-world."""
    eye = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, -np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, d, f, eye
    return c2w.astype(np.float32)


def intrinsics(W, H):
    fx = fy = 0.5 * W  # 90 deg HFOV as in SURVEY 8(d)
    return np.array([[fx, 0, (W - 1) / 2.0], [0, fy, (H - 1) / 2.0], [0, 0, 1]], np.float32)


def random_gaussians(N, seed=1234, depth_range=(1.0, 4.0), spread=2.5, scale_range=(0.003, 0.05), sh_k=16):
    """Gaussians scattered in front of a camera at the origin looking down +z."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(*depth_range, N)
    x = rng.uniform(-spread, spread, N) * z / depth_range[1]
    y = rng.uniform(-spread * 0.75, spread * 0.75, N) * z / depth_range[1]
    means = np.stack([x, y, z], 1).astype(np.float32)
    quats = rng.normal(size=(N, 4)).astype(np.float32)
    ls = rng.uniform(np.log(scale_range[0]), np.log(scale_range[1]), (N, 3))
    ls[:, 2] += np.log(0.3)
    log_scales = ls.astype(np.float32)
    opac_logit = rng.normal(0.0, 1.5, (N, 1)).astype(np.float32)
    sh = np.zeros((N, sh_k, 3), np.float32)
    sh[:, 0] = (rng.uniform(0.05, 0.95, (N, 3)) - 0.5) / 0.28209479177387814
    sh[:, 1:] = rng.normal(0, 0.05, (N, sh_k - 1, 3))
    return dict(means=means, quats=quats, log_scales=log_scales, opac_logit=opac_logit, sh=sh.astype(np.float32))


def default_camera(W, H, seed=0):
    rng = np.random.default_rng(seed)
    eye = rng.normal(0, 0.05, 3)
    c2w = look_at_c2w(eye, [0.05, -0.03, 3.0])
    return c2w, intrinsics(W, H)


def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = {"x": (1, 2), "y": (2, 0), "z": (0, 1)}[axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _wide_pose():
    Rc = _rot("y", 35.0) @ _rot("x", -20.0) @ _rot("z", 25.0)
    return Rc, np.array([0.4, -0.3, 0.2])


def wide_camera(W, H):
    """A camera none of whose symmetries hide an exchange: fx != fy, the principal point off the centre on both axes, a pose
    rotated about all three axes and translated.  -> (c2w [4, 4], K [3, 3]) float32, like default_camera."""
    Rc, t = _wide_pose()
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = Rc, t
    K = np.array([[0.45 * W, 0, 0.41 * W], [0, 0.7 * W, 0.58 * H], [0, 0, 1]])
    return c2w.astype(np.float32), K.astype(np.float32)


WIDE_NEAR = 0.15  # depths below this are drawn for N // 20 rows of wide_gaussians (down to -1: behind the camera)


def wide_gaussians(N, W, H, seed, sh_k=16):
    """Gaussians for wide_camera(W, H) that reach every arm of the projection's field-of-view clamp: x/z and y/z go to 1.6 times
    the larger clamp limit of their axis on both sides, depths from 0.15 to 5 with N // 20 rows between -1 and 0.15 (behind the
    camera, and around any near plane a test puts there), scales from 1 % to 50 % of the depth so that the clamped rows still
    overlap the image and some radii pass 100 px.  The rows behind the camera are scattered, so a prefix of the scene has the same
    mix.  Keys as random_gaussians, plus `scales` (= exp(log_scales))."""
    rng = np.random.default_rng(seed)
    _, K = wide_camera(W, H)
    fx, fy, cx, cy = (float(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    Rc, t = _wide_pose()
    z = rng.uniform(WIDE_NEAR, 5.0, N)
    z[rng.permutation(N)[:N // 20]] = rng.uniform(-1.0, WIDE_NEAR, N // 20)
    limx = max((W - cx) / fx, cx / fx) + 0.15 * W / fx
    limy = max((H - cy) / fy, cy / fy) + 0.15 * H / fy
    xr = rng.uniform(-1.6 * limx, 1.6 * limx, N)
    yr = rng.uniform(-1.6 * limy, 1.6 * limy, N)
    p_cam = np.stack([xr * z, yr * z, z], 1)
    means = (p_cam @ Rc.T + t).astype(np.float32)
    quats = rng.normal(size=(N, 4)).astype(np.float32)
    scales = np.exp(rng.uniform(np.log(0.01), np.log(0.5), (N, 3))) * np.clip(z, WIDE_NEAR, 5.0)[:, None]
    log_scales = np.log(scales).astype(np.float32)
    opac_logit = rng.normal(0.0, 1.5, (N, 1)).astype(np.float32)
    sh = np.zeros((N, sh_k, 3), np.float32)
    sh[:, 0] = (rng.uniform(0.05, 0.95, (N, 3)) - 0.5) / 0.28209479177387814
    sh[:, 1:] = rng.normal(0, 0.05, (N, sh_k - 1, 3))
    return dict(means=means, quats=quats, log_scales=log_scales, scales=np.exp(log_scales), opac_logit=opac_logit, sh=sh)


def wide_clamp_classes(means, viewmat, K, W, H, near=0.01, edge=1e-3):
    """Float64 classification of the rows of a scene against the projection's clamp limits and near plane:
    -> dict of [N] bools  xp, xn, yp, yn (x/z or y/z beyond that limit), on_limit (within `edge` relative of any limit: the backward
    is discontinuous there), behind (z < near), on_near (|z - near| < 1e-4 near)."""
    vm, K = np.asarray(viewmat, np.float64), np.asarray(K, np.float64)
    pc = np.asarray(means, np.float64) @ vm[:3, :3].T + vm[:3, 3]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    lims = dict(xp=(W - cx) / fx + 0.15 * W / fx, xn=cx / fx + 0.15 * W / fx,
                yp=(H - cy) / fy + 0.15 * H / fy, yn=cy / fy + 0.15 * H / fy)
    with np.errstate(all="ignore"):
        r = dict(xp=pc[:, 0] / pc[:, 2], xn=-pc[:, 0] / pc[:, 2], yp=pc[:, 1] / pc[:, 2], yn=-pc[:, 1] / pc[:, 2])
    out = {k: r[k] > lims[k] for k in lims}
    out["on_limit"] = np.zeros(pc.shape[0], bool)
    for k in lims:
        out["on_limit"] |= np.abs(r[k] - lims[k]) < edge * lims[k]
    out["behind"] = pc[:, 2] < near
    out["on_near"] = np.abs(pc[:, 2] - near) < 1e-4 * near
    return out


def assert_wide_scene_reaches_every_branch(cls, radii, big=False):
    """The conditions every test on the wide scene asserts on the oracle's forward, so that a change to the generator cannot
    empty a branch; `big`: also >= 50 rows with an unclamped radius above 100."""
    vis = np.asarray(radii) > 0
    cx, cy = cls["xp"] | cls["xn"], cls["yp"] | cls["yn"]
    for k in ("xp", "xn", "yp", "yn"):
        assert (vis & cls[k]).sum() >= 200, (k, int((vis & cls[k]).sum()))
    assert (vis & cx & cy).sum() >= 100, int((vis & cx & cy).sum())
    assert cls["behind"].sum() >= 100, int(cls["behind"].sum())
    assert (vis & cls["on_limit"]).sum() <= 0.01 * vis.sum(), int((vis & cls["on_limit"]).sum())
    assert cls["on_near"].sum() <= 3, int(cls["on_near"].sum())
    if big:
        assert (np.asarray(radii) > 100).sum() >= 50


def pose_inv(c2w):
    R, t = c2w[:3, :3], c2w[:3, 3]
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, :3] = R.T
    w2c[:3, 3] = -R.T @ t
    return w2c


def ulp_jitter(a, rng, ulps=1.0):
    """a float32 array with every element moved by a random relative amount of at most `ulps` * 2^-23 (integers untouched)"""
    a = np.asarray(a)
    if a.dtype.kind != "f":
        return a
    return (a.astype(np.float64) * (1.0 + rng.uniform(-1.0, 1.0, a.shape) * ulps * 2.0 ** -23)).astype(np.float32)


def condition_budget(fn, inputs, base, trials=3, seed=0, factor=32.0, floor=2e-5):
    """Per-ROW error budget of a float32 adjoint `fn(*inputs) -> tuple of [N, ...] arrays` from its own sensitivity: the outputs
    are re-evaluated `trials` times with every float input jittered by <= 1 ulp; a row's budget is
        factor * max_trials max_columns |fn(jittered) - base|  +  floor * max_columns |base|
    -- an ill-conditioned row (the projection adjoint inverts the 2x2 conic; gradients cancel) gets exactly the slack its own
    amplification of input rounding justifies, a well-conditioned one gets a few ulps.  -> list of [N] budgets, one per output."""
    rng = np.random.default_rng(seed)
    worst = [np.zeros(b.shape[0]) for b in base]
    for _ in range(trials):
        out = fn(*[ulp_jitter(a, rng) for a in inputs])
        for k, (o, b) in enumerate(zip(out, base)):
            d = np.abs(o.astype(np.float64) - b.astype(np.float64)).reshape(b.shape[0], -1).max(1)
            worst[k] = np.maximum(worst[k], d)
    return [factor * w + floor * np.abs(b).reshape(b.shape[0], -1).max(1) for w, b in zip(worst, base)]


def radius_is_borderline(conics, rel=2e-4):
    """[N] bool: the projection's radius = ceil(3 sqrt(lambda_max)) (fully_fused_projection_fwd.cu:165-167) is decided within
    `rel` of an integer -- the only Gaussians whose radius (or cull decision) float rounding may move.  lambda_max from the conic
    (= inverse of the blurred 2-D covariance), in float64."""
    a, b, c = (conics[:, k].astype(np.float64) for k in range(3))
    det_c = a * c - b * b
    with np.errstate(all="ignore"):
        ca, cb, cc = c / det_c, -b / det_c, a / det_c      # covariance
        det = ca * cc - cb * cb
        mid = 0.5 * (ca + cc)
        v = 3.0 * np.sqrt(mid + np.sqrt(np.maximum(0.01, mid * mid - det)))
    return ~np.isfinite(v) | (np.abs(v - np.round(v)) < rel * np.maximum(v, 1.0))


def bwd_class_lists(means2d, radii, tile_size, tw, th, bands=16):
    """The strip backward's work lists as the binning writes them (splat_bin.hpp: bwd_key): per class k (smallest 4 << k >= radius,
    the last class takes the rest) the visible Gaussians ordered by (band of the box's first tile row, id)."""
    r = np.asarray(radii)
    m = np.asarray(means2d, np.float32)
    ts = np.float32(tile_size)
    tr, tx, ty = r.astype(np.float32) / ts, m[:, 0] / ts, m[:, 1] / ts
    x0 = np.clip(np.floor(tx - tr), 0, tw); x1 = np.clip(np.ceil(tx + tr), 0, tw)
    y0 = np.clip(np.floor(ty - tr), 0, th); y1 = np.clip(np.ceil(ty + tr), 0, th)
    n_tiles = ((y1 - y0) * (x1 - x0)).astype(np.int64)
    band = np.where(n_tiles > 0, np.minimum(y0.astype(np.int64) * bands // th, bands - 1), 0)
    cls = np.where(r > 0, np.searchsorted(np.array([4, 8, 16, 32]), r, side="left"), -1)
    out = []
    for k in range(5):
        ids = np.nonzero(cls == k)[0]
        out.append(ids[np.argsort(band[ids], kind="stable")])
    return out
