"""CPU-side checks of the geometry / trajectory evaluation surface (no GPU): the C-ABI symbols and both hosts' entry points
exist with agreeing signatures, sample_surface is the area-weighted sampler it claims to be, and ate is the reference's
alignment (tests/golden/geo_eval_ref.npz, written by tests/golden/make_geo_eval_golden.py from scripts/ate_general.py)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geo_eval_ref.npz")


def _host():
    from gps_slam_amd import _build, _build_host, _lib
    _build.build()
    _lib.load_library()
    _build_host.build()
    import gps_slam_amd._host as h
    return h


def test_c_abi_exports_the_nn_entry_points_with_the_declared_signatures():
    from gps_slam_amd import _build, _lib
    raw = ctypes.CDLL(_build.build())
    i32, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    want = {"gps_nn_index_workspace_bytes": (i64, [i32]),
            "gps_nn_index_build": (i32, [i32, vp, vp, i64, vp]),
            "gps_nn_query_workspace_bytes": (i64, [i32]),
            "gps_nn_query": (i32, [i32, vp, i32, vp, vp, vp, vp, vp, i64, vp])}
    for name, sig in want.items():
        assert hasattr(raw, name), name
        assert _lib.PROTOTYPES[name] == sig, name
    lib = _lib.load_library()
    # size queries are host code: monotone, 16-byte multiples are not required but negative sizes are errors
    assert lib.gps_nn_index_workspace_bytes(-1) < 0 and lib.gps_nn_query_workspace_bytes(-1) < 0
    assert lib.gps_nn_index_workspace_bytes(1000) == lib.gps_knn_grid_workspace_bytes(1000)   # the same grid
    assert lib.gps_nn_query_workspace_bytes(0) >= 16 and lib.gps_nn_query_workspace_bytes(1000) >= 16 + 4000
    # argument checks come before any launch: R == 0 is an error, Q == 0 with a valid R a no-op
    assert lib.gps_nn_index_build(0, None, None, 0, None) == -1
    assert lib.gps_nn_query(0, None, 0, None, None, None, None, None, 0, None) == -1
    assert lib.gps_nn_query(5, None, 0, None, None, None, None, None, 0, None) == 0


def test_both_hosts_export_the_evaluation_surface_with_agreeing_signatures():
    h = _host()
    from gps_slam_amd import geom_eval
    from gps_slam_amd.slam_pipeline import SLAMPipeline
    from gps_slam_amd.tsdf_engine import TsdfEngine
    pairs = {"nearest_distances": "nearestDistances", "sample_surface": "sampleSurface", "eval_pcd": "evalPointClouds", "ate": "ate"}
    for py_name, cpp_name in pairs.items():
        assert callable(getattr(geom_eval, py_name)) and hasattr(h, cpp_name), (py_name, cpp_name)
    assert hasattr(TsdfEngine, "EvalMesh") and hasattr(h.ITMBasicEngine, "EvalMesh")
    for meth in ("evalGeometry", "evalTrajectory"):
        assert hasattr(SLAMPipeline, meth) and hasattr(h.SLAMPipeline, meth), meth
    # argument names and defaults: the C++ binding's docstring carries its signature
    sig = inspect.signature(geom_eval.eval_pcd)
    assert list(sig.parameters) == ["rec_points", "gt_points", "transform", "dist_thres", "sample_nums", "seed"]
    assert sig.parameters["sample_nums"].default == 1000000 and tuple(sig.parameters["dist_thres"].default) == (0.03,)
    doc = h.evalPointClouds.__doc__
    for name in sig.parameters:
        assert name in doc, name
    assert "1000000" in doc and "0.03" in doc
    assert list(inspect.signature(geom_eval.sample_surface).parameters) == ["triangles", "n", "seed", "uniforms"]
    for name in ("triangles", "n", "seed", "uniforms"):
        assert name in h.sampleSurface.__doc__
    for field in ("accuracy_cm", "completion_cm", "accuracy_ratio", "completion_ratio", "f1"):
        assert hasattr(h.GeomEvalResult, field), field
    for field in ("ate_mean_cm", "ate_rmse_cm"):
        assert hasattr(h.AteResult, field), field


def _triangles(rng, T):
    tri = rng.normal(size=(T, 3, 3)).astype(np.float32)
    tri *= rng.uniform(0.05, 3.0, size=(T, 1, 1)).astype(np.float32)   # very unequal areas
    tri[3] = tri[3, 0]                                                 # a degenerate triangle: zero area, never picked
    return tri


def _np_sample(tri, u):
    """numpy restatement of trimesh.sample.sample_surface for given uniforms u[n,3]"""
    t = tri.astype(np.float64)
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)
    cum = np.cumsum(area)
    face = np.searchsorted(cum, u[:, 0] * cum[-1])
    a, b = u[:, 1].copy(), u[:, 2].copy()
    flip = a + b > 1.0
    a[flip], b[flip] = 1.0 - a[flip], 1.0 - b[flip]
    return (t[face, 0] + a[:, None] * e1[face] + b[:, None] * e2[face]).astype(np.float32), face, area


@pytest.mark.parametrize("which", ["python", "cpp"])
def test_sample_surface_is_the_numpy_restatement_and_stays_inside_its_triangle(which):
    from gps_slam_amd import geom_eval
    rng = np.random.default_rng(5)
    tri = _triangles(rng, 37)
    n = 4001
    if which == "python":
        u = geom_eval.surface_uniforms(n, 11)
        pts, face = geom_eval.sample_surface(torch.as_tensor(tri), n, seed=11)
        pts_u, face_u = geom_eval.sample_surface(torch.as_tensor(tri), n, seed=99, uniforms=u)   # given uniforms win over the seed
    else:
        h = _host()
        u = h.surfaceUniforms(n, 11)
        pts, face = h.sampleSurface(torch.as_tensor(tri), n, 11)
        pts_u, face_u = h.sampleSurface(torch.as_tensor(tri), n, 99, u)
    assert torch.equal(u, geom_eval.surface_uniforms(n, 11))           # both hosts draw the same uniforms for a seed
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (n, 3) and face.dtype == torch.int64
    assert torch.equal(pts, pts_u) and torch.equal(face, face_u)       # the same uniforms give the same points
    want, want_face, area = _np_sample(tri, u.numpy())
    assert np.array_equal(face.numpy(), want_face)
    assert np.array_equal(pts.numpy(), want)
    assert 3 not in set(want_face.tolist())
    # area weighting: the share of samples per triangle follows its share of the area (4 sigma of a binomial)
    share = area / area.sum()
    got = np.bincount(want_face, minlength=len(tri)) / n
    assert np.all(np.abs(got - share) <= 4.0 * np.sqrt(share * (1 - share) / n) + 1.0 / n)
    # inside: barycentric coordinates of the float32 point, recomputed in float64, are >= 0 up to float32 rounding of the point
    t = tri.astype(np.float64)[want_face]
    e1, e2, d = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], pts.numpy().astype(np.float64) - t[:, 0]
    g11, g12, g22 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    det = g11 * g22 - g12 * g12
    a = ((d * e1).sum(1) * g22 - (d * e2).sum(1) * g12) / det
    b = ((d * e2).sum(1) * g11 - (d * e1).sum(1) * g12) / det
    tol = 1e-5   # float32 rounding of coordinates of magnitude <~ 10 against edges >= ~0.05 long, with slack for thin triangles
    assert a.min() >= -tol and b.min() >= -tol and (a + b).max() <= 1.0 + tol
    resid = d - a[:, None] * e1 - b[:, None] * e2                       # ... and the point lies in the triangle's plane
    assert np.abs(resid).max() <= 4e-6


@pytest.mark.parametrize("which", ["python", "cpp"])
def test_ate_matches_the_reference_alignment(which):
    from gps_slam_amd import geom_eval
    g = np.load(GOLD)
    est, gt = g["ate_est_c2w"], g["ate_gt_c2w"]
    if which == "python":
        r = geom_eval.ate(est, gt)
        mean_cm, rmse_cm, te, rot, trans = r["ate_mean_cm"], r["ate_rmse_cm"], r["trans_error"], r["rot"], r["trans"]
    else:
        r = _host().ate(torch.as_tensor(est), torch.as_tensor(gt))
        mean_cm, rmse_cm, te, rot, trans = r.ate_mean_cm, r.ate_rmse_cm, r.trans_error.numpy(), r.rot.numpy(), r.trans.numpy()
    want = float(g["ate_mean_cm"])
    assert abs(mean_cm - want) <= 1e-9 * want, (mean_cm, want)
    np.testing.assert_allclose(te, g["ate_trans_error"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(rot, g["ate_rot"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(trans, g["ate_trans"], rtol=0, atol=1e-12)
    # the true root mean square sits beside the mean the reference prints under that name, and is never below it
    want_rmse = float(np.sqrt(np.mean(g["ate_trans_error"] ** 2)) * 100.0)
    assert abs(rmse_cm - want_rmse) <= 1e-9 * want_rmse and rmse_cm > mean_cm
    # a rigidly moved copy of a trajectory has no error at all; float32 poses are accepted
    moved = gt.copy()
    moved[:, :3, 3] = gt[:, :3, 3] @ g["ate_rot"].T + np.array([3.0, -1.0, 0.5])
    z = geom_eval.ate(moved, gt) if which == "python" else None
    if z is not None:
        assert z["ate_mean_cm"] < 1e-10


@pytest.mark.parametrize("which", ["python", "cpp"])
def test_ate_rejects_mismatched_lengths_and_too_few_poses(which):
    from gps_slam_amd import geom_eval
    g = np.load(GOLD)
    est, gt = g["ate_est_c2w"], g["ate_gt_c2w"]
    if which == "python":
        call, err = (lambda a, b: geom_eval.ate(a, b)), ValueError
    else:
        h = _host()
        call, err = (lambda a, b: h.ate(torch.as_tensor(a), torch.as_tensor(b))), RuntimeError
    with pytest.raises(err):
        call(est[:-1], gt)
    with pytest.raises(err):
        call(est[:2], gt[:2])
    with pytest.raises(err):
        call(est[:, :3], gt[:, :3])
