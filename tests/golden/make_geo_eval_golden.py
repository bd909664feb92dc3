"""Generates tests/golden/geo_eval_ref.npz from the REFERENCE'S OWN PYTHON (loaded from /root/reference in the build container; it
cannot travel, so its outputs are committed as data):

  * scripts/geo_general.py: accuracy, completion, accuracy_ratio, completion_ratio (scipy cKDTree queries between two clouds) --
    the reconstruction metrics eval_pcd reports.  The module imports open3d, trimesh and tqdm at its top for the file I/O of
    eval_pcd; the four functions called here need numpy and scipy only, so empty stand-in modules take those three names.
  * scripts/ate_general.py: align(model, data) -- the rigid alignment behind its "ATE RMSE" line (which is the MEAN error).

Inputs: a 2 x 1.5 x 1 m box shell as ground truth; a noisy reconstruction of it with one end missing plus a small blob 35 m away
(so that queries run through the ring search AND the bounded-work fallback of gps_nn_query).  The clouds are float32 and are
stored as such next to their generator's parameters; the per-query distances are scipy's, float64, on exactly those values.

Run from the repo root:  python tests/golden/make_geo_eval_golden.py"""
import importlib.util
import os
import sys
import types

import numpy as np
from scipy.spatial import cKDTree

REF = "/root/reference/scripts"
PARAMS = dict(seed=20261018, box=(2.0, 1.5, 1.0), n_gt=6000, n_rec=4400, cut_x=1.55, noise=0.008, n_blob=40, blob_at=(35.0, 0.5, 0.5),
              blob_sigma=0.05, dist_th=0.03, n_poses=40, pose_noise=0.01)


def _load(name):
    for stand_in in ("open3d", "trimesh", "tqdm"):
        if stand_in not in sys.modules:
            m = types.ModuleType(stand_in)
            m.tqdm = lambda it, *a, **k: it
            sys.modules[stand_in] = m
    spec = importlib.util.spec_from_file_location("refpy_" + name, os.path.join(REF, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def box_shell(rng, n, box):
    """n uniform points on the surface of [0,bx] x [0,by] x [0,bz] (faces picked by area)"""
    bx, by, bz = box
    areas = np.array([by * bz, by * bz, bx * bz, bx * bz, bx * by, bx * by])
    face = rng.choice(6, size=n, p=areas / areas.sum())
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    p = np.zeros((n, 3))
    for f in range(6):
        m = face == f
        axis, side = f // 2, f % 2
        a, b = [k for k in range(3) if k != axis]
        p[m, axis] = side * box[axis]
        p[m, a] = u[m] * box[a]
        p[m, b] = v[m] * box[b]
    return p


def main():
    geo, ate = _load("geo_general"), _load("ate_general")
    P = PARAMS
    rng = np.random.default_rng(P["seed"])
    gt = box_shell(rng, P["n_gt"], P["box"]).astype(np.float32)
    rec = box_shell(rng, P["n_rec"], P["box"])
    rec = rec[rec[:, 0] < P["cut_x"]]                                   # one end of the box was never observed
    rec = rec + rng.normal(scale=P["noise"], size=rec.shape)
    blob = np.asarray(P["blob_at"]) + rng.normal(scale=P["blob_sigma"], size=(P["n_blob"], 3))
    rec = np.concatenate([rec, blob]).astype(np.float32)
    gt64, rec64 = gt.astype(np.float64), rec.astype(np.float64)
    d_acc, i_acc = cKDTree(gt64).query(rec64)      # rec -> gt, as accuracy()
    d_comp, i_comp = cKDTree(rec64).query(gt64)    # gt -> rec, as completion()
    th = P["dist_th"]
    acc, comp = geo.accuracy(gt64, rec64), geo.completion(gt64, rec64)
    acc_r, comp_r = geo.accuracy_ratio(gt64, rec64, dist_th=th), geo.completion_ratio(gt64, rec64, dist_th=th)
    assert acc == np.mean(d_acc) and comp == np.mean(d_comp)            # the distances stored ARE what the module averages
    assert acc_r == np.mean((d_acc < th).astype(np.float32)) and comp_r == np.mean((d_comp < th).astype(np.float32))
    Pp, Rr = acc_r * 100, comp_r * 100                                   # eval_pcd :71-76
    out = dict(gt=gt, rec=rec, d_acc=d_acc, d_comp=d_comp, dist_th=np.float64(th),
               accuracy_cm=np.float64(acc * 100), completion_cm=np.float64(comp * 100),
               accuracy_ratio=np.float64(Pp), completion_ratio=np.float64(Rr), f1=np.float64(2 * Pp * Rr / (Pp + Rr)),
               count_acc=np.int64((d_acc < th).sum()), count_comp=np.int64((d_comp < th).sum()))
    out.update({"param_" + k: np.asarray(v) for k, v in P.items()})
    # trajectory: a smooth ground-truth path; the estimate is a rigidly moved copy of it with drift and noise
    n = P["n_poses"]
    t = np.linspace(0.0, 1.0, n)
    gt_c2w = np.tile(np.eye(4), (n, 1, 1))
    gt_c2w[:, :3, 3] = np.stack([2.0 * np.cos(2.5 * t), 1.5 * np.sin(2.5 * t), 0.3 * t + 1.2], 1)
    ang = 0.4
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    est_c2w = gt_c2w.copy()
    est_c2w[:, :3, 3] = gt_c2w[:, :3, 3] @ Rz.T + np.array([0.5, -0.25, 0.1]) + rng.normal(scale=P["pose_noise"], size=(n, 3)) \
        + 0.02 * t[:, None] * np.array([1.0, 0.5, -0.5])
    rot, trans, trans_error = ate.align(gt_c2w[:, :3, 3].T, est_c2w[:, :3, 3].T)   # evaluate(): align(gt, est)
    out.update(ate_gt_c2w=gt_c2w, ate_est_c2w=est_c2w, ate_rot=np.asarray(rot), ate_trans=np.asarray(trans).reshape(3),
               ate_trans_error=np.asarray(trans_error), ate_mean_cm=np.float64(trans_error.mean() * 100.0))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "geo_eval_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    print("rec %d gt %d | acc %.4f cm comp %.4f cm | P %.3f R %.3f | max d_acc %.2f m max d_comp %.3f m | ATE mean %.4f cm"
          % (len(rec), len(gt), acc * 100, comp * 100, Pp, Rr, d_acc.max(), d_comp.max(), trans_error.mean() * 100))
    for d, name in ((d_acc, "acc"), (d_comp, "comp")):
        print("  %s: %d of %d reference distances within 2^-21 relative of the threshold" % (name, int((np.abs(d - th) <= 2.0 ** -21 * d).sum()), len(d)))


if __name__ == "__main__":
    sys.exit(main())
