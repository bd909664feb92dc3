"""Geometry and trajectory evaluation: the reference's scripts/geo_general.py (accuracy, completion, their ratios and F1 between a
reconstructed and a ground-truth cloud) and scripts/ate_general.py (rigidly aligned trajectory error), without leaving the library.

    nearest_distances   the KD-tree query of geo_general.py:9-34 as device work (gps_nn_index_build / gps_nn_query: exact)
    sample_surface      trimesh.sample.sample_surface as eval_pcd uses it: area-weighted points on a triangle mesh
    eval_pcd            geo_general.py:37-90 on two point tensors
    ate                 ate_general.py:29-61 (host only, float64)

The nearest-neighbour search is the only hot part and is a HIP kernel; sampling and the means run once per evaluation and are
plain torch / numpy.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import check, lib


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def nearest_distances(query, ref, return_stats=False):
    """For every row of query[Q,3] the distance to, and the index of, the nearest row of ref[R,3] (float32 device tensors) on the
    current stream -> (dist float32[Q], index int32[Q]) [, stats int32[2] = queries finished by the grid / by the brute force].
    Exact; ties go to the lowest index; a non-finite query gets (+inf, -1)."""
    for name, t in (("query", query), ("ref", ref)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 3):
            raise ValueError("%s must be a float32 device tensor [n,3]" % name)
    query, ref = query.contiguous(), ref.contiguous()
    Q, R = int(query.shape[0]), int(ref.shape[0])
    if R == 0:
        raise ValueError("nearest_distances: the reference set is empty")
    dev = query.device
    dist2 = torch.empty(Q, dtype=torch.float32, device=dev)
    index = torch.empty(Q, dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    ib, qb = int(lib.gps_nn_index_workspace_bytes(R)), int(lib.gps_nn_query_workspace_bytes(Q))
    iws = torch.empty(ib, dtype=torch.uint8, device=dev)
    qws = torch.empty(qb, dtype=torch.uint8, device=dev)
    check(lib.gps_nn_index_build(R, ref.data_ptr(), iws.data_ptr(), ib, _stream(dev)), "gps_nn_index_build")
    check(lib.gps_nn_query(R, iws.data_ptr(), Q, query.data_ptr(), dist2.data_ptr(), index.data_ptr(), stats.data_ptr(),
                           qws.data_ptr(), qb, _stream(dev)), "gps_nn_query")
    dist = torch.sqrt(dist2)
    return (dist, index, stats) if return_stats else (dist, index)


def surface_uniforms(n, seed):
    """the [n,3] float64 uniforms sample_surface draws for `seed`: column 0 picks the triangle, 1 and 2 the point in it"""
    return torch.rand((int(n), 3), dtype=torch.float64, generator=torch.Generator().manual_seed(int(seed)))


def sample_surface(triangles, n, seed=0, uniforms=None):
    """n area-weighted points on triangles[T,3,3] (trimesh.sample.sample_surface: cumulative areas, searchsorted on a uniform, a
    point from two more, reflected into the triangle) -> (points float32[n,3], triangle index int64[n]) on the triangles' device.
    Areas, the cumulative sum and the point are float64.  The same uniforms give the same points."""
    tri = triangles.to(torch.float64)
    if tri.dim() != 3 or tuple(tri.shape[1:]) != (3, 3) or tri.shape[0] == 0:
        raise ValueError("triangles must be [T,3,3] with T > 0")
    u = surface_uniforms(n, seed) if uniforms is None else uniforms.to(torch.float64)
    u = u.to(tri.device)
    p0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = 0.5 * torch.sqrt(cx * cx + cy * cy + cz * cz)
    cum = torch.cumsum(area, 0)
    face = torch.searchsorted(cum, u[:, 0] * cum[-1]).clamp_(max=tri.shape[0] - 1)
    a, b = u[:, 1], u[:, 2]
    flip = (a + b) > 1.0
    a, b = torch.where(flip, 1.0 - a, a), torch.where(flip, 1.0 - b, b)
    pts = p0[face] + a[:, None] * e1[face] + b[:, None] * e2[face]
    return pts.to(torch.float32), face


def eval_pcd(rec_points, gt_points, transform=None, dist_thres=(0.03,), sample_nums=1000000, seed=0):
    """eval_pcd of geo_general.py on two clouds (float32 device tensors [n,3]): rec_points is transformed (4x4, float64) and
    sub-sampled without replacement to min(P, sample_nums); accuracy = mean distance rec -> gt and completion = gt -> rec in
    centimetres (means in float64); per threshold the ratios of distances below it in percent and F1 = 2PR / (P + R)."""
    rec = rec_points
    if transform is not None:
        T = torch.as_tensor(np.asarray(transform, dtype=np.float64).reshape(4, 4), device=rec.device)
        rec = (rec.to(torch.float64) @ T[:3, :3].T + T[:3, 3]).to(torch.float32)
    P = int(rec.shape[0])
    if P == 0 or int(gt_points.shape[0]) == 0:
        raise ValueError("eval_pcd: empty point set")
    if P > sample_nums:   # (all P points otherwise: the reference's permutation of them changes no metric)
        pick = torch.randperm(P, generator=torch.Generator().manual_seed(int(seed)))[:sample_nums]
        rec = rec[pick.to(rec.device)]
    rec, gt = rec.contiguous(), gt_points.contiguous()
    d_acc = nearest_distances(rec, gt)[0].to(torch.float64)
    d_comp = nearest_distances(gt, rec)[0].to(torch.float64)
    out = dict(accuracy_cm=float(d_acc.mean()) * 100.0, completion_cm=float(d_comp.mean()) * 100.0,
               accuracy_ratio=[], completion_ratio=[], f1=[], dist_thres=[float(t) for t in dist_thres],
               n_rec=int(rec.shape[0]), n_gt=int(gt.shape[0]))
    for th in out["dist_thres"]:
        p = 100.0 * int((d_acc < th).sum()) / d_acc.numel()
        r = 100.0 * int((d_comp < th).sum()) / d_comp.numel()
        out["accuracy_ratio"].append(p)
        out["completion_ratio"].append(r)
        out["f1"].append(2.0 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


def mesh_vertices(triangles, n):
    """the cloud the reference's script reads from the PLY this package writes: all 3 n vertices of the first n triangle
    rows (p0 p1 p2 of ITMMesh::Triangle), duplicates included"""
    return triangles[:n, 0:3].reshape(-1, 3).contiguous()


def eval_mesh(engine, gt_points_or_triangles, transform=None, dist_thres=(0.03,), sample_nums=1000000, seed=0,
              max_triangles=1 << 24):
    """TsdfEngine.EvalMesh: MeshScene(), then eval_pcd of its vertices against ground-truth points [n,3], or against sample_nums
    points sampled from ground-truth triangles [T,3,3]"""
    tri, counts = engine.MeshScene(max_triangles)
    n = int(counts[0].item())
    if n == 0:
        raise ValueError("EvalMesh: the scene has no triangles")
    gt = gt_points_or_triangles
    if gt.dim() == 3:
        gt = sample_surface(gt.to(tri.device), sample_nums, seed)[0]
    return eval_pcd(mesh_vertices(tri, n), gt.to(tri.device, torch.float32), transform, dist_thres, sample_nums, seed)


def ate(est_c2w, gt_c2w):
    """ate_general.py: align(gt, est) -- zero-centre, 3x3 SVD, reflection fix -- on the translations of two [n,4,4] pose lists
    (float64 on the host) -> dict(ate_mean_cm, ate_rmse_cm, trans_error[n] in metres, rot, trans).  ate_mean_cm is the number the
    reference prints as "ATE RMSE" (it is the MEAN of the per-frame errors); ate_rmse_cm is their root mean square."""
    est = np.asarray(torch.as_tensor(est_c2w).cpu() if torch.is_tensor(est_c2w) else est_c2w, dtype=np.float64)
    gt = np.asarray(torch.as_tensor(gt_c2w).cpu() if torch.is_tensor(gt_c2w) else gt_c2w, dtype=np.float64)
    if est.ndim != 3 or est.shape[1:] != (4, 4) or gt.ndim != 3 or gt.shape[1:] != (4, 4):
        raise ValueError("ate: poses must be [n,4,4]")
    if est.shape[0] != gt.shape[0]:
        raise ValueError("ate: %d estimated poses against %d ground-truth poses" % (est.shape[0], gt.shape[0]))
    if est.shape[0] < 3:
        raise ValueError("ate: at least three poses are needed for a rigid alignment")
    model, data = gt[:, :3, 3].T, est[:, :3, 3].T   # align(model = gt, data = est), [3,n]
    mm, dm = model.mean(1, keepdims=True), data.mean(1, keepdims=True)
    W = (model - mm) @ (data - dm).T
    U, _, Vh = np.linalg.svd(W.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1.0
    rot = U @ S @ Vh
    trans = dm - rot @ mm
    err = rot @ model + trans - data
    te = np.sqrt((err * err).sum(0))
    return dict(ate_mean_cm=float(te.mean() * 100.0), ate_rmse_cm=float(np.sqrt((te * te).mean()) * 100.0), trans_error=te,
                rot=rot, trans=trans[:, 0])
