"""Built-on-purpose cases for the two tile binnings: the sorted-key path (csrc/splat_bin.hip) and the superblock path
(csrc/splat_bin_sb.hip + the histogram pass of csrc/splat_fused.hip).

No GPU import here: tests/test_binning_cases_cpu.py vets the case set against the C oracle without a GPU, and
tests/test_binning_edges_gpu.py runs the same cases through ops.isect_tiles_no_depth / ops.isect_tiles and SLAMGaussianModel.

A case is a dict: `name`, `W`, `H` (tile size 16), `m2` float32 [N, 2] and `radii` int32 [N] (sorted-key cases, optionally
`depths` float32 [N]) or `scene` (model-path cases: the parameter rows of scene_from_layout, `design_radii` the radii they
project to), and `expect`: the properties the case was built to have, by name (check_expect asserts them on a binning result,
the oracle's or the kernels').  Everything is built from a seeded numpy generator; where a count is given it is constructed,
not searched for.

Two things in the model-path set differ from a naive reading of "N Gaussians, radius r":
  * the projection blurs every covariance by eps2d = 0.3 and takes lambda_max = mid + sqrt(max(0.01, mid^2 - det)), so the
    smallest radius a visible Gaussian can have is ceil(3 sqrt(0.4)) = 2: the model-path radii start at 2, not 1;
  * a Gaussian has at most ONE pair per tile, so a superblock of 512 Gaussians holds at most 512 pairs of one tile, and the
    scatter's chunk is SCAT_THREADS * SCAT_ITEMS = 2,048 pairs.  The case `chunk_in_one_tile` (131,073 invisible + 2,000 in one
    tile, superblocks of 512) therefore pins "a full superblock in one bin behind 256 empty superblocks"; >= 1,024 pairs of one
    tile in one superblock, across a chunk boundary, need superblocks of 1,024: `chunk_in_one_tile_sb1024` (N = 264,120, shift
    2) has one superblock whose 1,024 Gaussians all sit in one tile and one whose 1,024 Gaussians all cover the same four
    tiles (1,024 pairs per tile, 512 in either of its two chunks).  A whole chunk in one bin would need superblocks of 2,048,
    N > 524,288: left out for its size.
"""
import numpy as np

TS = 16
MAX_RADIUS = 100          # SLAMGaussianModel.max_gs_radii
FX = 100.0                # focal length of the model-path camera
SB_MAX, SB_MAX_TILES, BIN_BLOCK = 512, 4096, 256   # splat_bin.hpp
WIDE_MAX_BINS, SORT_TILE = 4096, 2048              # splat_bin.hip
SCAT_CHUNK = 2048                                  # splat_bin_sb.hip: SCAT_THREADS * SCAT_ITEMS


def grid(W, H):
    return (W + TS - 1) // TS, (H + TS - 1) // TS


def tile_id_bits(n_tiles):
    """splat_bin.hip: bits_total"""
    b = 1
    while (1 << b) < n_tiles:
        b += 1
    return b


def sb_shift_for(N):
    """splat_bin.hpp: the smallest power of two of 256-Gaussian blocks with <= SB_MAX superblocks"""
    s = 0
    while (((N + 255) // 256 + (1 << s) - 1) >> s) > SB_MAX:
        s += 1
    return s


def n_superblocks(N):
    s = sb_shift_for(N)
    return ((N + 255) // 256 + (1 << s) - 1) >> s


def sb_supported(N, tw, th):
    """splat_bin_sb.hip: sb_supported, without the device's LDS opt-in (160 KB are there on the MI355X)"""
    n_tiles = tw * th
    if N <= 0 or n_tiles > SB_MAX_TILES or tw > 255 or th > 255:
        return False
    sb_size = BIN_BLOCK << sb_shift_for(N)
    return (n_tiles + (9 * n_tiles + 1) // 2 + 2 * sb_size + 2) * 4 <= 160 * 1024


def tile_boxes(m2, radii, tw, th):
    """splat_bin.hpp: tile_bbox in float32 -> x0, y0, x1, y1 (int64), zero-size for radius 0"""
    r = np.asarray(radii)
    m = np.asarray(m2, np.float32)
    ts = np.float32(TS)
    tr, tx, ty = r.astype(np.float32) / ts, m[:, 0] / ts, m[:, 1] / ts
    x0 = np.clip(np.floor(tx - tr), 0, tw).astype(np.int64); x1 = np.clip(np.ceil(tx + tr), 0, tw).astype(np.int64)
    y0 = np.clip(np.floor(ty - tr), 0, th).astype(np.int64); y1 = np.clip(np.ceil(ty + tr), 0, th).astype(np.int64)
    vis = r > 0
    return x0 * vis, y0 * vis, x1 * vis, y1 * vis


def tiles_of(m2, radii, tw, th):
    x0, y0, x1, y1 = tile_boxes(m2, radii, tw, th)
    return (x1 - x0) * (y1 - y0)


def in_tile(rng, n, tx, ty, margin=4.0):
    """n centres inside tile (tx, ty), `margin` px away from its border"""
    return np.stack([TS * np.asarray(tx) + rng.uniform(margin, TS - margin, n),
                     TS * np.asarray(ty) + rng.uniform(margin, TS - margin, n)], 1)


# ------------------------------------------------------------------------------------------------------ sorted-key cases
def _case(name, W, H, m2, radii, expect, depths=None):
    c = dict(name=name, W=W, H=H, m2=np.ascontiguousarray(m2, np.float32), radii=np.ascontiguousarray(radii, np.int32),
             expect=dict(expect))
    if depths is not None:
        c["depths"] = np.ascontiguousarray(depths, np.float32)
    return c


TILE_COUNT_GRIDS = ((1, 1, 1), (2, 1, 1), (64, 64, 12), (65, 64, 13), (181, 128, 15), (256, 256, 16))   # tw, th, bits


def tile_count_cases(seed=11):
    out = []
    for k, (tw, th, bits) in enumerate(TILE_COUNT_GRIDS):
        rng = np.random.default_rng(seed + k)
        W, H, N = TS * tw, TS * th, 3000
        m2 = np.stack([rng.uniform(-20, W + 20, N), rng.uniform(-20, H + 20, N)], 1)
        radii = rng.integers(1, 41, N)
        radii[rng.uniform(size=N) < 0.3] = 0
        # first tile, last tile, last tile row, last tile column: single-tile Gaussians
        corners = [(0, 0), (tw - 1, th - 1), (tw // 2, th - 1), (tw - 1, th // 2)]
        ids = [7, 300, 1500, N - 1]
        for i, (tx, ty) in zip(ids, corners):
            m2[i] = in_tile(rng, 1, tx, ty)[0]
            radii[i] = 3
        touched = sorted({ty * tw + tx for tx, ty in corners})
        out.append(_case("tiles_%dx%d" % (tw, th), W, H, m2, radii,
                         dict(bits=bits, n_tiles=tw * th, tiles_touched=touched, one_pass=tw * th <= WIDE_MAX_BINS)))
    return out


ISECT_COUNTS = (0, 1, 2047, 2048, 2049, 4096)


def isect_count_cases(seed=23):
    """96 x 64: n_isects exactly as listed = the tiles of one filler + single-tile Gaussians, invisible ones in between"""
    W, H = 96, 64
    tw, th = grid(W, H)
    out = []
    for k, n in enumerate(ISECT_COUNTS):
        rng = np.random.default_rng(seed + k)
        rows = []   # (x, y, r)
        if n >= 2:
            rows.append((40.0, 30.0, 20))   # the filler
        f = int(tiles_of(np.array([[40.0, 30.0]]), np.array([20]), tw, th)[0]) if n >= 2 else 0
        assert f <= n
        singles = n - f
        c = in_tile(rng, singles, rng.integers(0, tw, singles), rng.integers(0, th, singles), margin=7.5)
        rows += [(x, y, int(r)) for (x, y), r in zip(c, rng.integers(1, 8, singles))]
        n_inv = max(500 if n == 0 else 0, len(rows) // 3)
        rows += [(float(rng.uniform(0, W)), float(rng.uniform(0, H)), 0) for _ in range(n_inv)]
        a = np.array(rows, np.float64)[rng.permutation(len(rows))]
        out.append(_case("n_isects_%d" % n, W, H, a[:, :2], a[:, 2], dict(n_isects=n, n_visible=n - f + (1 if n >= 2 else 0))))
    return out


def pile_up_case(seed=31):
    """one key, five 2,048-item sort blocks, every wave's 512 items equal"""
    rng = np.random.default_rng(seed)
    N, W, H = 10000, 640, 480
    m2 = in_tile(rng, N, 17, 11, margin=7.0)
    radii = rng.integers(1, 7, N)
    inv = np.array([5, 511, 512, 2047, 2048, 4100, 6143, 8192, 9000, 9998])
    radii[inv] = 0
    return _case("pile_up", W, H, m2, radii, dict(n_isects=N - inv.size, one_tile=11 * 40 + 17, n_visible=N - inv.size,
                                                  sort_blocks=5))


def whole_grid_case(seed=37):
    """Gaussians 0, 255, 256, 599: all 4,096 tiles each; 257..511 invisible; block 3 (768..1023) all invisible between
    blocks with tiles (block 1 holds Gaussian 256, so the all-zero block needs rows of its own: N = 1,100, not 600)"""
    rng = np.random.default_rng(seed)
    N, W, H = 1100, 1024, 1024
    m2 = np.stack([rng.uniform(0, W, N), rng.uniform(0, H, N)], 1)
    radii = rng.integers(1, 11, N)
    big = np.array([0, 255, 256, 599])
    m2[big] = (W / 2 + 0.25, H / 2 - 0.25)
    radii[big] = 2000
    radii[257:512] = 0
    radii[768:1024] = 0
    return _case("whole_grid", W, H, m2, radii, dict(tiles_per_gauss=(big, np.full(4, 4096)), zero_block=3, min_len=4))


def off_image_case(seed=41):
    """50 x 37 (4 x 3 tiles, ragged): centres up to 200 px outside each side of the tile grid, the box clipped to one tile
    column, one tile row, one tile, or nothing (r > 0 with zero tiles: still counted as visible)"""
    rng = np.random.default_rng(seed)
    W, H = 50, 37
    tw, th = grid(W, H)
    GW, GH = TS * tw, TS * th
    rows, ids, tiles = [], [], []

    def add(x, y, r, t):
        ids.append(len(rows)); tiles.append(t); rows.append((x, y, r))

    for d in (1, 5, 16, 17, 50, 100, 199, 200):
        for frac in (0.0, 0.25):
            for k in (1, 8, 16):
                r, e = d + k, d + frac
                if r >= 40:   # (> half the grid either way: the box spans the whole grid along the other axis)
                    add(-e, GH / 2 + 0.5, r, th); add(GW + e, GH / 2 + 0.5, r, th)          # one tile column
                    add(GW / 2 + 0.5, -e, r, tw); add(GW / 2 + 0.5, GH + e, r, tw)          # one tile row
                for cx, cy in ((-e, -e), (GW + e, -e), (-e, GH + e), (GW + e, GH + e)):     # one tile
                    add(cx, cy, r, 1)
            for r in (d, d - 1):                                                            # nothing, r > 0
                if r > 0:
                    add(-e, GH / 2, r, 0); add(GW + e, GH / 2, r, 0); add(GW / 2, -e, r, 0); add(GW / 2, GH + e, r, 0)
                    add(-e, -e, r, 0); add(GW + e, GH + e, r, 0)
    n_design = len(rows)
    n_empty = sum(1 for t in tiles if t == 0)
    for _ in range(300):
        rows.append((float(rng.uniform(-20, W + 20)), float(rng.uniform(-20, H + 20)), int(rng.integers(0, 30))))
    perm = rng.permutation(len(rows))
    a = np.array(rows, np.float64)[perm]
    pos = np.empty(len(rows), np.int64); pos[perm] = np.arange(len(rows))
    ids = pos[np.array(ids)]
    c = _case("off_image", W, H, a[:, :2], a[:, 2], dict(tiles_per_gauss=(ids, np.array(tiles)), n_designed=n_design))
    # (random rows may add empty boxes of their own: the exact number is restated from the boxes)
    c["expect"]["n_empty_visible"] = int(((c["radii"] > 0) & (tiles_of(c["m2"], c["radii"], tw, th) == 0)).sum())
    assert c["expect"]["n_empty_visible"] >= n_empty > 0 and set(tiles) == {0, 1, tw, th}
    return c


ONE_BYTE_DEPTHS = np.array([0x40404041, 0x40404140, 0x40414040, 0x41404040], np.uint32)   # 0x40404040 with one byte moved


def depth_cases(seed=53):
    W, H = 96, 64
    out = []

    def scene(rng, N, invisible=0.0):
        m2 = np.stack([rng.uniform(-10, W + 10, N), rng.uniform(-10, H + 10, N)], 1)
        radii = rng.integers(1, 21, N)
        radii[rng.uniform(size=N) < invisible] = 0
        return m2, radii

    rng = np.random.default_rng(seed)
    m2, radii = scene(rng, 10000)
    out.append(_case("depth_all_equal", W, H, m2, radii, dict(n_depths=1, n_visible=10000), np.full(10000, 2.5)))
    rng = np.random.default_rng(seed + 1)
    m2, radii = scene(rng, 10000, 0.1)
    d = ONE_BYTE_DEPTHS[rng.integers(0, 4, 10000)].view(np.float32)
    out.append(_case("depth_one_byte", W, H, m2, radii, dict(n_depths=4), d))
    rng = np.random.default_rng(seed + 2)
    m2, radii = scene(rng, 5000, 0.1)
    d = (10.0 ** rng.uniform(-30, 30, 5000)).astype(np.float32)
    d[rng.permutation(5000)[:100]] = np.arange(1, 101, dtype=np.uint32).view(np.float32)   # denormals 1.4e-45 ..
    d[rng.permutation(5000)[:50]] = (10.0 ** rng.uniform(-44, -38.5, 50)).astype(np.float32)
    out.append(_case("depth_wide_range", W, H, m2, radii, dict(denormals=True), d))
    rng = np.random.default_rng(seed + 3)
    m2, radii = scene(rng, 3000, 1.1)
    out.append(_case("depth_all_invisible", W, H, m2, radii, dict(n_isects=0, n_visible=0), rng.uniform(1, 4, 3000)))
    return out


_SORTED = {}


def sorted_key_cases():
    if not _SORTED:
        for c in tile_count_cases() + isect_count_cases() + [pile_up_case(), whole_grid_case(), off_image_case()]:
            _SORTED[c["name"]] = c
    return _SORTED


_DEPTH = {}


def depth_key_cases():
    if not _DEPTH:
        for c in depth_cases():
            _DEPTH[c["name"]] = c
    return _DEPTH


# ------------------------------------------------------------------------------------------------------ model-path cases
MIN_MODEL_RADIUS = 2


def scene_from_layout(px, py, radius_px, W, H, seed=0, sh_k=16):
    """Gaussians on the plane z = 1 (z = -1: radius_px 0, behind the camera) of a camera at the origin looking down +z, fx = fy =
    100, principal point at the image centre, whose projection has centre (px, py) and -- before the clamp to max_gs_radii -- radius
    radius_px (>= 2).  Isotropic scale s, identity quaternion: the blurred 2-D covariance is (100 s)^2 (I + p p^T) + 0.3 I with
    p = (x, y), the projection's lambda_max = mid + sqrt(max(0.01, mid^2 - det)) and radius = ceil(3 sqrt(lambda_max)).  s is
    chosen so that 3 sqrt(lambda_max) = radius_px - 0.5 (1.95 for radius 2): half a pixel from both neighbouring integers.
    -> dict(means, quats, log_scales, scales, opac_logit, sh, c2w, K)"""
    px, py, r = np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(radius_px, np.int64)
    N = r.shape[0]
    assert ((r == 0) | (r >= MIN_MODEL_RADIUS)).all()
    rng = np.random.default_rng(seed + 977)
    cx, cy = W / 2.0, H / 2.0
    x, y = (px - cx) / FX, (py - cy) / FX
    q = x * x + y * y
    v = np.where(r <= 2, 1.95, r - 0.5)            # (rows behind the camera: any scale)
    A = ((v / 3.0) ** 2 - 0.3) / (1.0 + q)            # lambda_max = l1 where the eigenvalues differ by >= 0.2
    A2 = ((v / 3.0) ** 2 - 0.4) / (1.0 + 0.5 * q)     # else mid + 0.1
    A = np.where(A * q / 2.0 >= 0.1, A, A2)
    assert (A > 0).all()
    s = np.sqrt(A) / FX
    vis = r > 0
    means = np.stack([x, y, np.where(vis, 1.0, -1.0)], 1).astype(np.float32)
    quats = np.zeros((N, 4), np.float32); quats[:, 0] = 1.0
    scales = np.repeat(s[:, None], 3, 1).astype(np.float32)
    sh = np.zeros((N, sh_k, 3), np.float32)
    sh[:, 0] = (rng.uniform(0.05, 0.95, (N, 3)) - 0.5) / 0.28209479177387814
    sh[:, 1:] = rng.normal(0, 0.05, (N, sh_k - 1, 3))
    K = np.array([[FX, 0, cx], [0, FX, cy], [0, 0, 1]], np.float32)
    return dict(means=means, quats=quats, log_scales=np.log(scales), scales=scales,
                opac_logit=rng.normal(0.0, 1.5, (N, 1)).astype(np.float32), sh=sh, c2w=np.eye(4, dtype=np.float32), K=K)


def _model_case(name, W, H, px, py, r, expect, seed=0):
    r = np.asarray(r, np.int64)
    e = dict(expect)
    N = r.shape[0]
    tw, th = grid(W, H)
    e.setdefault("sb_shift", sb_shift_for(N))
    e.setdefault("n_sb", n_superblocks(N))
    e.setdefault("superblock_path", sb_supported(N, tw, th))
    return dict(name=name, W=W, H=H, N=N, scene=scene_from_layout(px, py, r, W, H, seed=seed),
                design_radii=np.minimum(r, MAX_RADIUS).astype(np.int32), expect=e)


def _scatter(rng, N, W, H, r_lo, r_hi, invisible, geometric=False, margin=0.5):
    px, py = rng.uniform(margin, W - margin, N), rng.uniform(margin, H - margin, N)
    r = np.minimum(r_lo + rng.geometric(0.15, N) - 1, r_hi) if geometric else rng.integers(r_lo, r_hi + 1, N)
    r[rng.uniform(size=N) < invisible] = 0
    return px, py, r


def _one_tile(seed=101):
    rng = np.random.default_rng(seed)
    c = in_tile(rng, 3000, 20, 15)
    return _model_case("one_tile", 640, 480, c[:, 0], c[:, 1], np.full(3000, 3), dict(n_isects=3000, one_tile=15 * 40 + 20,
                       sb_pairs_one_tile=256, sb_shift=0, n_sb=12))


def _one_tile_wide(seed=102):
    rng = np.random.default_rng(seed)
    N = 2048
    px, py = 320 + rng.uniform(-6, 6, N), 240 + rng.uniform(-6, 6, N)
    # 150 before the clamp: radius 100, 13 or 14 tiles each way
    return _model_case("one_tile_wide", 640, 480, px, py, np.full(N, 150), dict(tiles_each=(13 * 13, 13 * 14, 14 * 14), chunks_per_sb_min=20,
                       sb_shift=0, n_sb=8))


def _chunk_in_one_tile(seed=103):
    rng = np.random.default_rng(seed)
    n0, n1 = 131073, 2000
    c = in_tile(rng, n0 + n1, 2, 1)
    r = np.concatenate([np.zeros(n0, np.int64), np.full(n1, 3)])
    return _model_case("chunk_in_one_tile", 96, 64, c[:, 0], c[:, 1], r, dict(n_isects=n1, one_tile=1 * 6 + 2, sb_shift=1, n_sb=260,
                       empty_sb_in_front=256, sb_pairs_one_tile=512))


def _chunk_in_one_tile_sb1024(seed=104):
    rng = np.random.default_rng(seed)
    n0 = 255 * 1024
    c = in_tile(rng, n0 + 3000, 2, 1)
    r = np.concatenate([np.zeros(n0, np.int64), np.full(3000, 3)])
    c[n0 + 1024:n0 + 2048] = (48, 32) + rng.uniform(-1, 1, (1024, 2))   # on the corner of tiles (2, 1), (3, 1), (2, 2), (3, 2): all four
    return _model_case("chunk_in_one_tile_sb1024", 96, 64, c[:, 0], c[:, 1], r, dict(n_isects=3000 + 3 * 1024, sb_shift=2, n_sb=258,
                       empty_sb_in_front=255, sb_pairs_one_tile=1024, tiles_exact=[8, 9, 14, 15], sb_two_chunks=(256, 1024)))


def _alternating_rows(seed=105):
    rng = np.random.default_rng(seed)
    N, W, H = 4096, 640, 480
    tw, th = grid(W, H)
    odd = np.arange(N) & 1
    c = in_tile(rng, N, rng.integers(0, tw, N), np.where(odd, th - 1, 0))
    return _model_case("alternating_rows", W, H, c[:, 0], c[:, 1], np.full(N, 3), dict(n_isects=N, full_band=True, sb_shift=0, n_sb=16))


def _one_row(seed=106):
    rng = np.random.default_rng(seed)
    px, py, r = _scatter(rng, 4096, 4080, 16, 2, 40, 0.1, margin=4.0)
    return _model_case("one_row", 4080, 16, px, py, r, dict(superblock_path=True, full_band=True))


def _too_wide(seed=107):
    rng = np.random.default_rng(seed)
    px, py, r = _scatter(rng, 2000, 4096, 16, 2, 40, 0.1, margin=4.0)
    return _model_case("too_wide", 4096, 16, px, py, r, dict(superblock_path=False))


def _grid_4096(seed=108):
    rng = np.random.default_rng(seed)
    px, py, r = _scatter(rng, 20000, 1024, 1024, 2, 100, 0.1)
    return _model_case("grid_4096", 1024, 1024, px, py, r, dict(superblock_path=True, n_tiles=4096, bits=12))


def _grid_4160(seed=109):
    rng = np.random.default_rng(seed)
    px, py, r = _scatter(rng, 20000, 1040, 1024, 2, 100, 0.1)
    return _model_case("grid_4160", 1040, 1024, px, py, r, dict(superblock_path=False, n_tiles=4160, bits=13))


BLOCK_EDGE_N = (1, 255, 256, 257, 511, 512, 513, 131072, 131073, 262144, 262145)
_BLOCK_EDGE_SB = {1: (0, 1), 255: (0, 1), 256: (0, 1), 257: (0, 2), 511: (0, 2), 512: (0, 2), 513: (0, 3), 131072: (0, 512),
                  131073: (1, 257), 262144: (1, 512), 262145: (2, 257)}


def _block_edges(N):
    rng = np.random.default_rng(200 + N % 1009)
    px, py, r = _scatter(rng, N, 96, 64, 2, 40, 0.0, geometric=True)
    r[rng.permutation(N)[:N // 4]] = 0     # a quarter invisible, exactly
    if N > 3:
        r[1], r[2] = 2, 40
    r[-1] = 5
    shift, n_sb = _BLOCK_EDGE_SB[N]
    last = (N - 1) % (256 << shift) + 1
    return _model_case("block_edges_%d" % N, 96, 64, px, py, r, dict(sb_shift=shift, n_sb=n_sb, last_sb_size=last, last_visible=True),
                       seed=N)


def _uniform_lengths(seed=110, extra=0, name="uniform_lengths"):
    rng = np.random.default_rng(seed)
    W, H = 640, 480
    tw, th = grid(W, H)
    t = np.repeat(np.arange(tw * th), 8)
    if extra:
        t = np.concatenate([t, np.zeros(extra, np.int64)])
    t = t[rng.permutation(t.size)]
    c = in_tile(rng, t.size, t % tw, t // tw)
    e = dict(n_isects=t.size, max_len=8 + extra)
    e.update(dict(all_class0=True) if not extra else dict(class63_tiles=[0]))
    return _model_case(name, W, H, c[:, 0], c[:, 1], np.full(t.size, 3), e)


MODEL_BUILDERS = {"one_tile": _one_tile, "one_tile_wide": _one_tile_wide, "chunk_in_one_tile": _chunk_in_one_tile,
                  "chunk_in_one_tile_sb1024": _chunk_in_one_tile_sb1024, "alternating_rows": _alternating_rows, "one_row": _one_row,
                  "too_wide": _too_wide, "grid_4096": _grid_4096, "grid_4160": _grid_4160, "uniform_lengths": _uniform_lengths,
                  "long_tile": lambda: _uniform_lengths(extra=2100, name="long_tile")}
MODEL_BUILDERS.update({"block_edges_%d" % n: (lambda n_=n: _block_edges(n_)) for n in BLOCK_EDGE_N})
_MODEL = {}


def model_case(name):
    """the case (built once, shared, never modified)"""
    if name not in _MODEL:
        _MODEL[name] = MODEL_BUILDERS[name]()
    return _MODEL[name]


# ------------------------------------------------------------------------------------------------- the expected properties
def check_expect(case, radii, tpg, flat, offs, N=None):
    """Assert the properties in case["expect"] on one binning result: radii / tiles_per_gauss [N], the sorted Gaussian ids
    `flat` [n_isects] and the tile offsets [n_tiles] -- the oracle's (CPU vetting) or the kernels' (GPU tests)."""
    e = case["expect"]
    tw, th = grid(case["W"], case["H"])
    T = tw * th
    radii, tpg, flat = np.asarray(radii), np.asarray(tpg).reshape(-1), np.asarray(flat).reshape(-1)
    offs = np.asarray(offs).reshape(-1).astype(np.int64)
    N = radii.shape[0] if N is None else N
    n = flat.shape[0]
    assert offs.shape[0] == T and int(tpg.sum()) == n
    length = np.diff(np.concatenate([offs, [n]]))
    tile = np.repeat(np.arange(T), length)          # tile of every pair
    name = case["name"]
    if "n_isects" in e:
        assert n == e["n_isects"], (name, n)
    if "n_visible" in e:
        assert int((radii > 0).sum()) == e["n_visible"], name
    if "bits" in e:
        assert tile_id_bits(T) == e["bits"] and T == e["n_tiles"], name
    if "one_pass" in e:
        assert (T <= WIDE_MAX_BINS) == e["one_pass"], name
    if "one_tile" in e:
        assert n > 0 and (tile == e["one_tile"]).all(), name
    if "tiles_touched" in e:
        assert set(e["tiles_touched"]) <= set(np.unique(tile).tolist()), name
    if "tiles_exact" in e:
        assert e["tiles_exact"] == np.unique(tile).tolist(), name
    if "sort_blocks" in e:
        assert (n + SORT_TILE - 1) // SORT_TILE == e["sort_blocks"], name
    if "max_len" in e:
        assert int(length.max()) == e["max_len"], (name, int(length.max()))
    if "min_len" in e:
        assert int(length.min()) >= e["min_len"], name      # (whole-grid Gaussians: every tile has at least these)
    if "tiles_per_gauss" in e:
        ids, want = e["tiles_per_gauss"]
        assert np.array_equal(tpg[ids], want), (name, tpg[ids][:16], want[:16])
    if "n_empty_visible" in e:
        assert int(((radii > 0) & (tpg == 0)).sum()) == e["n_empty_visible"], name
    if "zero_block" in e:
        blk = np.add.reduceat(tpg, np.arange(0, tpg.shape[0], BIN_BLOCK))
        b = e["zero_block"]
        assert blk[b] == 0 and blk[b - 1] > 0 and blk[b + 1] > 0 and (tpg[b * BIN_BLOCK:(b + 1) * BIN_BLOCK] == 0).all(), name
    if "tiles_each" in e:
        assert set(np.unique(tpg).tolist()) <= set(e["tiles_each"]) and len(np.unique(tpg)) >= 1, (name, np.unique(tpg))
    if "all_class0" in e:
        assert (length >> 5 == 0).all() and (length > 0).all(), name
    if "class63_tiles" in e:
        assert np.nonzero(np.minimum(63, length >> 5) == 63)[0].tolist() == e["class63_tiles"] and length[0] >= 2048, name
    if "last_visible" in e:
        assert radii[N - 1] > 0 and tpg[N - 1] > 0, name
    # superblocks
    shift, n_sb = sb_shift_for(N), n_superblocks(N)
    if "sb_shift" in e:
        assert (shift, n_sb) == (e["sb_shift"], e["n_sb"]), (name, shift, n_sb)
    if "last_sb_size" in e:
        assert N - (n_sb - 1) * (BIN_BLOCK << shift) == e["last_sb_size"], name
    sb = flat.astype(np.int64) >> (8 + shift)       # superblock of every pair
    pairs_sb = np.bincount(sb, minlength=n_sb)
    if "empty_sb_in_front" in e:
        k = e["empty_sb_in_front"]
        assert (pairs_sb[:k] == 0).all() and pairs_sb[k] > 0, name
    if "sb_pairs_one_tile" in e:
        most = int(np.bincount(sb * T + tile).max())
        assert most == e["sb_pairs_one_tile"], (name, most)
    if "sb_two_chunks" in e:   # a superblock with two chunks, each tile's pairs half in either
        k, per_tile = e["sb_two_chunks"]
        assert pairs_sb[k] == 2 * SCAT_CHUNK and (np.bincount(tile[sb == k])[e["tiles_exact"]] == per_tile).all(), name
    if "chunks_per_sb_min" in e:
        assert (pairs_sb // SCAT_CHUNK >= e["chunks_per_sb_min"]).all(), (name, pairs_sb)
    if e.get("full_band"):
        row = tile // tw
        for k in range(n_sb):
            rows_k = row[sb == k]
            assert rows_k.size and rows_k.min() == 0 and rows_k.max() == th - 1, (name, k)


def check_superblock_route(case):
    tw, th = grid(case["W"], case["H"])
    assert sb_supported(case["N"], tw, th) == case["expect"]["superblock_path"], case["name"]
