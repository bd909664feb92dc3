"""Built-on-purpose cases for the strip backward (csrc/splat_raster_bwd.hip) and a plain float64 reference of the operation.

No GPU import here: tests/test_strip_cases_cpu.py vets the case set against the C oracle without a GPU, and
tests/test_strip_backward_cases_gpu.py runs the same cases through gps_raster_ges_bwd_strips with caller-made class lists.

The operation (gsplat rasterize_to_pixels_bwd_ges_new_parallel.cu:18-201): every visible Gaussian visits the pixels of its
2r x 2r box, columns int(x) - r + 1 .. int(x) + r and rows likewise (int() truncates toward zero, :83-96), clipped to the
image; a pixel contributes when sigma >= 0, alpha = min(0.999, o exp(-sigma)) >= 1/255 and the Gaussian's depth is not
behind ref_depth + delta; the conic / mean / opacity gradients exist only where o exp(-sigma) <= 0.999.

A case is a dict of float32 / int32 arrays plus explicit class lists (`lists`: five int32 arrays, class k = the smallest k
with 4 << k >= r, the last class takes every r > 32) and `tags` (name -> Gaussian ids) naming the Gaussians that stand for a
situation, so that the CPU test can assert that the situation is really there.  Gaussian 0 of every case is invisible
(radius 0, in no list) although its other values are those of a large opaque Gaussian in the middle of the image: a task
lane with no list entry reads record 0.
"""
import math

import numpy as np

REL, BAND, SIG = 2e-5, 1e-5, 2 * 2.0 ** -23   # the constants of test_raster_ges_fwd_bwd
PER_TASK = (16, 8, 4, 2, 1)                   # Gaussians per wave task of class k
T255 = float(np.float32(1.0) / np.float32(255.0))
C999 = float(np.float32(0.999))
NEAR, FAR, DELTA = 2.5, 1000.0, 0.1           # ref_depth checkerboard; cut = 2.6 on near cells
ARRAYS = ("m2", "conics", "colors", "opac", "radii", "ref_depth")


def bwd_class(r):
    return 0 if r <= 4 else 1 if r <= 8 else 2 if r <= 16 else 3 if r <= 32 else 4


# ----------------------------------------------------------------------------------------------------------- reference
class _Terms:
    """One Gaussian over its clipped box: per-pixel terms of the ten sums and their absolute-value bounds."""
    __slots__ = ("js", "is_", "x0", "y0", "on", "unc", "t", "a", "wgt", "near", "clamp_only")


def _terms(g, m2, conics, colors, opac, radii, ref_depth, W, H, delta, v_rc, v_ra, band):
    r = int(radii[g])
    if r <= 0:
        return None
    x, y = float(m2[g, 0]), float(m2[g, 1])
    x0, y0 = int(x) - r + 1, int(y) - r + 1            # int(): toward zero
    js = np.arange(max(x0, 0), min(x0 + 2 * r, W))
    is_ = np.arange(max(y0, 0), min(y0 + 2 * r, H))
    if js.size == 0 or is_.size == 0:
        return None
    ca, cb, cc = (float(v) for v in conics[g])
    o, depth = float(opac[g]), float(colors[g, 3])
    rgb = colors[g].astype(np.float64)
    dx = (x - (js + 0.5))[None, :]
    dy = (y - (is_ + 0.5))[:, None]
    sigma = 0.5 * (ca * dx * dx + cc * dy * dy) + cb * dx * dy
    vis = np.exp(-sigma)
    a = o * vis
    alpha = np.minimum(C999, a)
    cut = ref_depth[is_[:, None], js[None, :]].astype(np.float64) + float(np.float32(delta))
    vc = v_rc[is_[:, None], js[None, :]].astype(np.float64)       # [h, w, 4]
    va = v_ra[is_[:, None], js[None, :]].astype(np.float64)
    T = _Terms()
    T.js, T.is_, T.x0, T.y0 = js, is_, x0, y0
    T.on = (sigma >= 0.0) & (alpha >= T255) & ~(depth > cut)
    T.unc = T.on & (a <= C999)
    v_alpha = (vc * rgb).sum(-1) + va
    va_abs = np.abs(vc * rgb).sum(-1) + np.abs(va)
    vs, vs_abs = -a * v_alpha, a * va_abs
    t = np.zeros((10,) + sigma.shape)
    ab = np.zeros_like(t)
    for q in range(4):
        t[q] = alpha * vc[..., q]
        ab[q] = np.abs(t[q])
    t[4], ab[4] = 0.5 * vs * dx * dx, 0.5 * vs_abs * dx * dx
    t[5], ab[5] = vs * dx * dy, vs_abs * np.abs(dx * dy)
    t[6], ab[6] = 0.5 * vs * dy * dy, 0.5 * vs_abs * dy * dy
    t[7], ab[7] = vs * (ca * dx + cb * dy), vs_abs * (np.abs(ca * dx) + np.abs(cb * dy))
    t[8], ab[8] = vs * (cb * dx + cc * dy), vs_abs * (np.abs(cb * dx) + np.abs(cc * dy))
    t[9], ab[9] = vis * v_alpha, vis * va_abs
    T.t, T.a = t, ab
    T.wgt = 0.5 * (abs(ca) * dx * dx + abs(cc) * dy * dy) + np.abs(cb * dx * dy)
    T.near, T.clamp_only = _borderline(sigma, a, alpha, depth, cut, band)
    return T


def _borderline(sigma, a, alpha, depth, cut, band):
    """decisions another rounding of exp could take the other way: alpha on 1/255, depth on the cut -> near; o vis on 0.999
    (accepted either way, only the conic / mean / opacity terms hang on it) -> clamp_only"""
    cand = (sigma >= 0.0) & (alpha >= (1.0 - band) * T255) & (depth <= cut + band * np.abs(cut))
    near = cand & ((np.abs(a - T255) <= band * T255) | (np.abs(depth - cut) <= band * np.abs(cut)))
    return near, cand & ~near & (np.abs(a - C999) <= band * C999)


def borderline_pairs(case, band):
    """[(gaussian, row, column, kind)] as box_backward_f64 lists them, for another band (decisions only, no sums)"""
    pairs = []
    W, H = case["W"], case["H"]
    for g in range(case["radii"].size):
        r = int(case["radii"][g])
        x, y = float(case["m2"][g, 0]), float(case["m2"][g, 1])
        x0, y0 = int(x) - r + 1, int(y) - r + 1
        js, is_ = np.arange(max(x0, 0), min(x0 + 2 * r, W)), np.arange(max(y0, 0), min(y0 + 2 * r, H))
        if r <= 0 or js.size == 0 or is_.size == 0:
            continue
        ca, cb, cc = (float(v) for v in case["conics"][g])
        dx, dy = (x - (js + 0.5))[None, :], (y - (is_ + 0.5))[:, None]
        sigma = 0.5 * (ca * dx * dx + cc * dy * dy) + cb * dx * dy
        a = float(case["opac"][g]) * np.exp(-sigma)
        cut = case["ref_depth"][is_[:, None], js[None, :]].astype(np.float64) + float(np.float32(case["delta"]))
        near, clamp_only = _borderline(sigma, a, np.minimum(C999, a), float(case["colors"][g, 3]), cut, band)
        for kind, mask in (("cut", near), ("clamp", clamp_only)):
            pairs += [(g, int(is_[i]), int(js[j]), kind) for i, j in zip(*np.nonzero(mask))]
    return pairs


def box_backward_f64(m2, conics, colors, opac, radii, ref_depth, W, H, delta, v_rc, v_ra, band=BAND):
    """-> dict: sums[N,10] in row layout {v_colors[4], v_conics[3], v_means2d[2], v_opacity}; scale[N,10] = sum |terms|;
    sig_scale[N,10] = sum |terms| weighted by sum |terms of sigma|; flip[N,10] = what the borderline pairs could contribute;
    pairs = [(gaussian, row, column, kind)] with kind 'cut' (alpha on 1/255 or depth on the cut) or 'clamp' (o vis on 0.999:
    entries 4..9 only); flip_gauss = the ids that have a pair; rows[N] = number of image rows with a contributing pixel,
    row_lo / row_hi[N] the first and last of them."""
    N = radii.shape[0]
    out = {k: np.zeros((N, 10)) for k in ("sums", "scale", "sig_scale", "flip")}
    out["rows"] = np.zeros(N, np.int64)
    out["row_lo"], out["row_hi"] = np.zeros(N, np.int64), np.full(N, -1, np.int64)   # first / last contributing image row
    pairs = []
    for g in range(N):
        T = _terms(g, m2, conics, colors, opac, radii, ref_depth, W, H, delta, v_rc, v_ra, band)
        if T is None:
            continue
        m = np.concatenate([np.repeat(T.on[None], 4, 0), np.repeat(T.unc[None], 6, 0)], 0)
        out["sums"][g] = (T.t * m).sum((1, 2))
        out["scale"][g] = (T.a * m).sum((1, 2))
        out["sig_scale"][g] = (T.a * m * T.wgt[None]).sum((1, 2))
        fm = np.concatenate([np.repeat(T.near[None], 4, 0), np.repeat((T.near | T.clamp_only)[None], 6, 0)], 0)
        out["flip"][g] = (T.a * fm).sum((1, 2))
        out["rows"][g] = int(T.on.any(1).sum())
        if T.on.any():
            out["row_lo"][g], out["row_hi"][g] = T.is_[T.on.any(1)][[0, -1]]
        for kind, mask in (("cut", T.near), ("clamp", T.clamp_only)):
            for i, j in zip(*np.nonzero(mask)):
                pairs.append((g, int(T.is_[i]), int(T.js[j]), kind))
    out["pairs"] = pairs
    out["flip_gauss"] = sorted({p[0] for p in pairs})
    return out


def reference(case, band=BAND):
    return box_backward_f64(case["m2"], case["conics"], case["colors"], case["opac"], case["radii"], case["ref_depth"],
                            case["W"], case["H"], case["delta"], case["v_rc"], case["v_ra"], band)


def column_share_f64(case, g, offset):
    """The share of box columns `offset` and `offset + r` (the two columns one lane of the strip kernel walks) in Gaussian
    g's ten sums, and the number of contributing pixels in them."""
    T = _terms(g, *(case[k] for k in ARRAYS), case["W"], case["H"], case["delta"], case["v_rc"], case["v_ra"], BAND)
    share = np.zeros(10)
    if T is None:
        return share, 0
    r = int(case["radii"][g])
    sel = np.isin(T.js - T.x0, (offset, offset + r))[None, :]
    m = np.concatenate([np.repeat((T.on & sel)[None], 4, 0), np.repeat((T.unc & sel)[None], 6, 0)], 0)
    return (T.t * m).sum((1, 2)), int((T.on & sel).sum())


def contributing_columns(case, g):
    """Box column offsets (0 .. 2r - 1) of Gaussian g that hold a contributing pixel."""
    T = _terms(g, *(case[k] for k in ARRAYS), case["W"], case["H"], case["delta"], case["v_rc"], case["v_ra"], BAND)
    return np.zeros(0, np.int64) if T is None else (T.js - T.x0)[T.on.any(0)]


def clamped_pixels(case, g):
    """[(row, column)] where Gaussian g contributes with the 0.999 clamp active."""
    T = _terms(g, *(case[k] for k in ARRAYS), case["W"], case["H"], case["delta"], case["v_rc"], case["v_ra"], BAND)
    return [] if T is None else [(int(T.is_[i]), int(T.js[j])) for i, j in zip(*np.nonzero(T.on & ~T.unc))]


def tolerance(ref):
    """(rounding part, with the borderline pairs' contribution): the project's bound of test_raster_ges_fwd_bwd"""
    base = REL * ref["scale"] + SIG * ref["sig_scale"] + 1e-30
    return base, base + 1.001 * ref["flip"]


# --------------------------------------------------------------------------------------------------------------- cases
def _k(o):
    """contour half-extent of {alpha >= 1/255} in standard deviations"""
    return math.sqrt(2.0 * math.log(255.0 * o))


def wide(r, o):
    """isotropic, alpha >= 1/255 on the whole box: the box limits it"""
    s = (1.5 * r + 2.0) / _k(o)
    return s * s, 0.0, s * s


def narrow(r, o):
    """isotropic, the ellipse ends at a third of the box: the record's bounds trim rows and columns"""
    s = max(r / 3.0, 0.45) / _k(o)
    return s * s, 0.0, s * s


def aniso(r, o, tall=False, rho=0.5):
    """cb != 0, x and y extents 4 : 1 (tall: 1 : 4), the longer one 0.8 r"""
    e_long = max(0.8 * r, 1.0) / _k(o)
    e_short = e_long / 4.0
    sx, sy = (e_short, e_long) if tall else (e_long, e_short)
    return sx * sx, rho * sx * sy, sy * sy


class Scene:
    def __init__(self, name, W, H, seed):
        self.name, self.W, self.H, self.seed = name, W, H, seed
        self.rng = np.random.default_rng(seed)
        self.g = []
        self.lists = [[] for _ in range(5)]
        self.tags = {}
        # Gaussian 0: invisible (radius 0, in no list); its record is what lanes without a list entry read
        self.add(W / 2 + 0.3, H / 2 + 0.4, 0, wide(20, 0.9), o=0.9, depth=1.7, listed=False)

    def depth(self):
        rng = self.rng
        return float(rng.uniform(1.5, NEAR + DELTA - 0.05) if rng.uniform() < 0.6 else rng.uniform(NEAR + DELTA + 0.05, 4.5))

    def add(self, x, y, r, cov, o=None, depth=None, tag=None, listed=True):
        o = float(self.rng.uniform(0.35, 0.95)) if o is None else o
        if callable(cov):
            cov = cov(r, o)
        sxx, sxy, syy = cov
        det = sxx * syy - sxy * sxy
        assert det > 0
        i = len(self.g)
        rgb = self.rng.uniform(0.0, 1.0, 3)
        self.g.append((x, y, syy / det, -sxy / det, sxx / det, rgb[0], rgb[1], rgb[2], self.depth() if depth is None else depth, o, r))
        if listed and r > 0:
            self.lists[bwd_class(r)].append(i)
        for t in ([tag] if isinstance(tag, str) else (tag or [])):
            self.tags.setdefault(t, []).append(i)
        return i

    def interior(self, r):
        """a centre where the box fits (along an axis the image is too short for: near the middle)"""
        W, H, u = self.W, self.H, self.rng.uniform
        x = u(r, W - r - 1) if W - r - 1 > r else W / 2 + u(-3, 3)
        y = u(r, H - r - 1) if H - r - 1 > r else H / 2 + u(-3, 3)
        return float(x), float(y)

    def shuffle_lists(self):
        for L in self.lists:
            self.rng.shuffle(L)

    def finish(self, family):
        a = np.array(self.g, np.float64)
        W, H = self.W, self.H
        ii, jj = np.mgrid[0:H, 0:W]
        ref_depth = np.where(((ii // 2) + (jj // 3)) % 2 == 0, NEAR, FAR).astype(np.float32)   # 3 x 2 pixel cells
        rng = np.random.default_rng(self.seed + 1000003)
        case = {"name": self.name, "family": family, "W": W, "H": H, "delta": DELTA, "seed": self.seed,
                "m2": a[:, 0:2].astype(np.float32), "conics": a[:, 2:5].astype(np.float32),
                "colors": a[:, 5:9].astype(np.float32), "opac": a[:, 9].astype(np.float32), "radii": a[:, 10].astype(np.int32),
                "ref_depth": ref_depth, "v_rc": rng.normal(size=(H, W, 4)).astype(np.float32),
                "v_ra": rng.normal(size=(H, W)).astype(np.float32),
                "lists": [np.array(L, np.int32) for L in self.lists], "tags": {k: list(v) for k, v in self.tags.items()}}
        cut = np.float32(NEAR) + np.float32(DELTA)
        assert (np.abs(case["colors"][:, 3] - cut) >= 1e-3).all() and (np.abs(case["colors"][:, 3] - (FAR + DELTA)) >= 1e-3).all()
        N = a.shape[0]
        for k, L in enumerate(case["lists"]):
            assert ((L > 0) & (L < N)).all() and len(set(L.tolist())) == L.size
            assert all(bwd_class(int(case["radii"][i])) == k and case["radii"][i] > 0 for i in L)
        return case


LADDER = (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 100, 127, 128, 129, 192, 193)


def ladder_cases(seed=1):
    s = Scene("ladder", 448, 320, seed)
    for r in LADDER:
        for n, (shape, kw) in enumerate((("wide", wide), ("narrow", narrow), ("aniso", lambda r_, o_, n_=r: aniso(r_, o_, tall=bool(n_ & 1))))):
            x, y = s.interior(r)
            s.add(x, y, r, kw, tag=["r%d" % r, shape, "r%d_%s" % (r, shape)])
    s.shuffle_lists()
    return [s.finish("ladder")]


EDGE_RADII = (3, 12, 40, 100)


def _edge_scene(name, W, H, seed):
    s = Scene(name, W, H, seed)
    for r in EDGE_RADII:
        f = 0.37 * r
        mid_x, mid_y = W / 2 + 0.23, H / 2 + 0.31
        places = [("left", f, mid_y), ("right", W - f - 0.2, mid_y), ("top", mid_x, f + 0.1), ("bottom", mid_x, H - f - 0.3),
                  ("corner_tl", f, f + 0.2), ("corner_tr", W - f - 0.4, f), ("corner_bl", f + 0.1, H - f), ("corner_br", W - f, H - f - 0.1),
                  ("neg_x_03", -0.3, mid_y), ("neg_x_17", -1.7, mid_y), ("neg_y_03", mid_x, -0.3), ("neg_y_17", mid_x, -1.7),
                  ("neg_xy", -0.3, -1.7), ("neg_yx", -1.7, -0.3), ("past_right", W + 1.6, mid_y), ("past_bottom", mid_x, H + 0.7),
                  ("on_integer", float(int(mid_x)), float(int(mid_y))), ("on_half", int(mid_x) + 0.5, int(mid_y) + 0.5),
                  ("outside_left", -r - 2.5, mid_y), ("outside_below", mid_x, H + r + 3.25), ("outside_corner", W + r + 1.5, -r - 4.5)]
        for n, (tag, x, y) in enumerate(places):
            s.add(x, y, r, wide, tag=[tag, "wide"])
            s.add(x, y, r, lambda r_, o_, n_=n: aniso(r_, o_, tall=bool(n_ & 1)), tag=[tag, "aniso"])
    s.shuffle_lists()
    return s.finish("edges")


def edge_cases(seed=2):
    return [_edge_scene("edges_448x320", 448, 320, seed), _edge_scene("edges_33x17", 33, 17, seed + 1)]


SPANS = (0, 1, 2, 3, 4, 5, 9, 13)


def span_cases(seed=3):
    """class-4 Gaussians (one per workgroup task, its rows dealt to four waves) with exactly k contributing rows"""
    W, H = 448, 320
    s = Scene("spans", W, H, seed)
    for r in (40, 70):
        for n, k in enumerate(SPANS):
            x = float(int(s.rng.uniform(r, W - r)) + 0.6)
            o = 0.8
            if k == 0:
                s.add(x, -r - 3.5 if n & 1 else H + r + 2.5, r, wide, o=o, depth=1.8, tag="span0")
                continue
            # centre 0.2 px inside the first (last) image row's centre, contour half-height k - 0.5: rows 0 .. k - 1 (H - k .. H - 1)
            for top in (True, False):
                y = 0.7 if top else H - 0.7
                ex, ey = 0.8 * r / _k(o), (k - 0.5) / _k(o)
                s.add(x, y, r, (ex * ex, 0.0, ey * ey), o=o, depth=1.8, tag="span%d" % k)
    s.shuffle_lists()
    return [s.finish("spans")]


def mixed_cases(seed=4):
    """list neighbours of one wave task: disjoint row ranges, different radii of the class, an empty span"""
    W, H = 448, 320
    s = Scene("mixed", W, H, seed)
    for k, (r_lo, r_hi) in enumerate(((1, 4), (5, 8), (9, 16), (17, 32))):
        u = s.rng.uniform
        x = lambda: float(u(r_hi, W - r_hi))
        d = lambda: float(u(1.5, NEAR))   # in front of every cut: the row ranges are the boxes
        ids = [s.add(x(), r_hi - 0.6, r_hi, wide, depth=d(), tag="mixed_top"), s.add(x(), H - r_lo + 0.3, r_lo, wide, depth=d(), tag="mixed_bottom"),
               s.add(x(), H / 2 + 7.3, r_lo, wide, depth=d(), tag="mixed_r_lo"), s.add(x(), H / 2 - 9.6, r_hi, aniso, depth=d(), tag="mixed_r_hi"),
               s.add(x(), -r_hi - 5.5, r_hi, wide, depth=d(), tag="mixed_empty"),
               s.add(x(), H / 2 + 0.4, (r_lo + r_hi) // 2, narrow, depth=d(), tag="mixed_mid"),
               s.add(x(), H / 2 + 30.1, r_hi, (r_hi * r_hi / 4.0, 0.0, r_hi * r_hi / 4.0), o=0.0, depth=d(), tag="mixed_empty"),
               s.add(x(), 0.4 * H, r_lo, wide, depth=d(), tag="mixed_mid")]
        assert s.lists[k] == ids      # this order IS the case: pairs (top, bottom), (r_lo, r_hi), (empty, mid), (empty, mid)
    return [s.finish("mixed")]


def _list_counts(kind):
    return [(0, 1, p - 1, p, p + 1, 8 * p + 1, 8 * 3 * p - 1)[kind] for p in PER_TASK]


SKEWED_COUNTS = (1, 8 * 8 + 1, 3, 2 * 17, 9)   # tasks per class: 1, 9, 1, 17, 9
LIST_KINDS = ("0", "1", "per_task-1", "per_task", "per_task+1", "8*per_task+1", "8*3*per_task-1")


def list_cases(seed=5):
    """every class at the same kind of count; plus 1,545 class-4 entries (more than the launch has workgroups)"""
    cases = []
    cls_r = ((1, 4), (5, 8), (9, 16), (17, 32), (33, 40))
    for kind in range(7):
        W, H = 224, 160
        s = Scene("lists_" + LIST_KINDS[kind], W, H, seed + kind)
        shapes = (wide, narrow, aniso)
        for k, n in enumerate(_list_counts(kind)):
            for _ in range(n):
                r = int(s.rng.integers(cls_r[k][0], cls_r[k][1] + 1))
                s.add(float(s.rng.uniform(-4, W + 4)), float(s.rng.uniform(-4, H + 4)), r, shapes[int(s.rng.integers(3))])
        for r in (3, 12, 40):   # visible, in no list: their rows must stay untouched
            s.add(W / 2 + 0.1 * r, H / 2 - 0.2 * r, r, wide, listed=False, tag="unlisted")
        s.shuffle_lists()
        c = s.finish("lists")
        assert [L.size for L in c["lists"]] == _list_counts(kind)
        cases.append(c)
    # classes with different task counts: an XCD past the end of a short list still has tasks of a long one
    W, H = 224, 160
    s = Scene("lists_skewed", W, H, seed + 8)
    for k, n in enumerate(SKEWED_COUNTS):
        for _ in range(n):
            r = int(s.rng.integers(cls_r[k][0], cls_r[k][1] + 1))
            s.add(float(s.rng.uniform(-4, W + 4)), float(s.rng.uniform(-4, H + 4)), r, (wide, narrow, aniso)[int(s.rng.integers(3))])
    s.add(W / 2 + 0.3, H / 2 - 0.7, 12, wide, listed=False, tag="unlisted")
    s.shuffle_lists()
    cases.append(s.finish("lists"))
    W, H = 640, 480
    s = Scene("lists_1545_class4", W, H, seed + 7)
    for n in range(1545):
        r = 33 + n % 8
        s.add(float(s.rng.uniform(0, W)), float(s.rng.uniform(0, H)), r, (narrow, aniso, wide)[n % 3 if n % 16 else 2])
    s.add(W / 2, H / 2, 50, wide, listed=False, tag="unlisted")
    s.shuffle_lists()
    cases.append(s.finish("lists"))
    return cases


def value_cases(seed=6):
    W, H = 224, 160
    s = Scene("values", W, H, seed)
    for r in (3, 12, 27, 40, 70):
        x, y = s.interior(r)
        s.add(x, y, r, (r * r / 4.0, 0.0, r * r / 4.0), o=0.0, tag="opac0")
        x, y = s.interior(r)
        s.add(x, y, r, (r * r / 4.0, 0.0, r * r / 4.0), o=1.0 / 256.0, tag="opac_below_cut")
        x, y = s.interior(r)
        s.add(x, y, r, wide, o=0.5, tag="opac_half")
        # opacity 1 on a pixel centre: o vis = 1 > 0.999 there, exp(-1 / (2 s^2)) <= 0.97 at the neighbours
        x, y = s.interior(r)
        sd = min(4.0, max(1.2, r / 3.0))
        s.add(int(x) + 0.5, int(y) + 0.5, r, (sd * sd, 0.0, sd * sd), o=1.0, depth=1.9, tag="opac1")
    s.shuffle_lists()
    return [s.finish("values")]


FAMILIES = {"ladder": ladder_cases, "edges": edge_cases, "spans": span_cases, "mixed": mixed_cases, "lists": list_cases,
            "values": value_cases}
_CACHE = {}


def family(name):
    """the cases of a family with their float64 reference (computed once, shared, never modified)"""
    if name not in _CACHE:
        cases = FAMILIES[name]()
        for c in cases:
            c["ref"] = reference(c)
        _CACHE[name] = cases
    return _CACHE[name]
