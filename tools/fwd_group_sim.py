"""Trip counts of the record forward (raster_ges_fwd_pk_kernel, splat_raster_fwd_pk.inc) when the lanes of a wave are split into
groups that each walk only the survivors whose pixel bounds touch the group -- the host-side estimate behind the per-group
survivor lists (LABBOOK.md section 23).  CPU only.

Input: the recorded {alpha >= 1/255} bounds of profiles/r05_extents_640x480_1000f.npz (width x rows of every visible Gaussian),
placed at uniform positions in the image.  The kernel's own structure is kept: 16 x 16 tiles, list order shuffled, batches of
GPS_FWD_BATCH = 512 entries, per 16 x 8 half the survivors of the batch, split in GPS_FWD_LIST_SPLIT = 4 equal parts (one wave
each).  A wave's trips = the longest list among its lane groups; `trips` sums them over all waves, `longest part` sums per
(tile, batch) the largest wave, which is what the tile's lock-step phases wait for.  Both relative to one group per wave.

usage: python tools/fwd_group_sim.py [extents.npz] [seed]"""
import os
import sys

import numpy as np

BATCH, SPLIT = 512, 4
SHAPES = [(16, 8), (8, 8), (16, 2), (8, 4), (4, 8), (4, 4)]   # lane groups of a 16 x 8 half, pixels wide x high


def simulate(path, seed=0):
    d = np.load(path)
    W, H = int(d["W"]), int(d["H"])
    w, h = d["width"].astype(np.int64), d["rows"].astype(np.int64)
    keep = (w > 0) & (h > 0)
    w, h = np.minimum(w[keep], W), np.minimum(h[keep], H)
    rng = np.random.default_rng(seed)
    x0 = (rng.uniform(size=w.size) * (W - w + 1)).astype(np.int64)
    y0 = (rng.uniform(size=h.size) * (H - h + 1)).astype(np.int64)
    x1, y1 = x0 + w - 1, y0 + h - 1
    tw, th = (W + 15) // 16, (H + 15) // 16
    lists = [[] for _ in range(tw * th)]
    for k in range(w.size):
        for ty in range(y0[k] // 16, y1[k] // 16 + 1):
            for tx in range(x0[k] // 16, x1[k] // 16 + 1):
                lists[ty * tw + tx].append(k)
    trips = np.zeros(len(SHAPES))
    longest = np.zeros(len(SHAPES))
    for t, ids in enumerate(lists):
        if not ids:
            continue
        ids = rng.permutation(np.asarray(ids))
        X0, Y0 = 16 * (t % tw), 16 * (t // tw)
        for b in range(0, ids.size, BATCH):
            e = ids[b:b + BATCH]
            worst = np.zeros(len(SHAPES))
            for half in range(2):
                ylo, yhi = Y0 + 8 * half, Y0 + 8 * half + 7
                s = e[(y0[e] <= yhi) & (y1[e] >= ylo)]   # survivors of the half (x always overlaps: the entry is in the tile's list)
                for p in range(SPLIT):
                    part = s[p * s.size // SPLIT:(p + 1) * s.size // SPLIT]
                    for k, (gw, gh) in enumerate(SHAPES):
                        n = 0
                        for gy in range(8 // gh):
                            for gx in range(16 // gw):
                                hit = ((x0[part] <= X0 + gw * gx + gw - 1) & (x1[part] >= X0 + gw * gx) &
                                       (y0[part] <= ylo + gh * gy + gh - 1) & (y1[part] >= ylo + gh * gy))
                                n = max(n, int(hit.sum()))
                        trips[k] += n
                        worst[k] = max(worst[k], n)
            longest += worst
    return W, H, int(w.size), float(w.mean()), float(h.mean()), sum(len(l) for l in lists), trips, longest


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "r05_extents_640x480_1000f.npz")
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    W, H, n, mw, mh, entries, trips, longest = simulate(path, seed)
    print("%s: %dx%d, %d bounds, mean %.1f x %.1f px, %d list entries" % (os.path.basename(path), W, H, n, mw, mh, entries))
    print("| lane groups per wave (px, w x h) | trips vs one group | longest part vs one group |")
    print("|---|---|---|")
    for k, (gw, gh) in enumerate(SHAPES):
        print("| %d x (%dx%d) | %.3f | %.3f |" % (128 // (gw * gh), gw, gh, trips[k] / trips[0], longest[k] / longest[0]))


if __name__ == "__main__":
    main()
