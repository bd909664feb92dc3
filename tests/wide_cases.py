"""The wide-camera scene (scenes.wide_camera / wide_gaussians) with what the CPU oracle and the float64 formulation make of it,
computed once per size and shared by the oracle tests and the GPU parity tests.  Nothing here touches a GPU; callers must not
modify what they get."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from oracle import splat_ref as orc
from tests import scenes

N_WIDE, SEED_WIDE = 4000, 11
SIZES = [(96, 64), (50, 37)]


def torch_project(means, quats, scales, viewmat, K, W, H, eps2d=0.3):
    """Dense float64 restatement of the pinhole projection maths (for autograd)."""
    R, t = viewmat[:3, :3], viewmat[:3, 3]
    mc = means @ R.T + t
    q = quats / quats.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    Rq = torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = Rq * scales[:, None, :]
    cov = M @ M.transpose(1, 2)
    cov_c = R @ cov @ R.T
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    X, Y, Z = mc.unbind(1)
    tfx, tfy = 0.5 * W / fx, 0.5 * H / fy
    lxp, lxn = (W - cx) / fx + 0.3 * tfx, cx / fx + 0.3 * tfx
    lyp, lyn = (H - cy) / fy + 0.3 * tfy, cy / fy + 0.3 * tfy
    rz = 1 / Z
    tx = Z * torch.minimum(lxp, torch.maximum(-lxn, X * rz))
    ty = Z * torch.minimum(lyp, torch.maximum(-lyn, Y * rz))
    zero = torch.zeros_like(Z)
    J = torch.stack([fx * rz, zero, -fx * tx * rz * rz, zero, fy * rz, -fy * ty * rz * rz], 1).reshape(-1, 2, 3)
    c2 = J @ cov_c @ J.transpose(1, 2)
    c2 = c2 + eps2d * torch.eye(2, dtype=c2.dtype)
    det = c2[:, 0, 0] * c2[:, 1, 1] - c2[:, 0, 1] * c2[:, 1, 0]
    conic = torch.stack([c2[:, 1, 1] / det, -c2[:, 0, 1] / det, c2[:, 0, 0] / det], 1)
    m2 = torch.stack([fx * X * rz + cx, fy * Y * rz + cy], 1)
    b = 0.5 * (c2[:, 0, 0] + c2[:, 1, 1])
    radius = torch.ceil(3 * torch.sqrt(b + torch.sqrt(torch.clamp(b * b - det, min=0.01))))
    return m2, Z, conic, radius, det


@functools.lru_cache(maxsize=None)
def wide_case(W, H, seed=SEED_WIDE, sh_k=16):
    """N_WIDE Gaussians under the wide camera, the oracle's forward with default parameters, the float64 clamp classes -- and the
    assertion that every branch is populated (scenes.assert_wide_scene_reaches_every_branch)."""
    g = scenes.wide_gaussians(N_WIDE, W, H, seed, sh_k=sh_k)
    c2w, K = scenes.wide_camera(W, H)
    vm = scenes.pose_inv(c2w)
    r0, m0, d0, c0 = orc.proj_fwd(g["means"], g["quats"], g["scales"], vm, K, W, H)
    cls = scenes.wide_clamp_classes(g["means"], vm, K, W, H)
    scenes.assert_wide_scene_reaches_every_branch(cls, r0, big=(W, H) == (96, 64))
    clamped = cls["xp"] | cls["xn"] | cls["yp"] | cls["yn"]
    return SimpleNamespace(N=N_WIDE, W=W, H=H, g=g, c2w=c2w, K=K, vm=vm, cam_pos=c2w[:3, 3].astype(np.float32).copy(),
                           r0=r0, m0=m0, d0=d0, c0=c0, cls=cls, clamped=clamped)


def torch_project64(case, requires_grad=False):
    """torch_project in float64 on the case's float32 inputs -> (leaves, outputs)"""
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    leaves = [t(case.g["means"]), t(case.g["quats"]), t(case.g["scales"])]
    for x in leaves:
        x.requires_grad_(requires_grad)
    return leaves, torch_project(*leaves, t(case.vm), t(case.K), case.W, case.H)


def cull64(m2, z, radius, det, W, H, near=0.01, far=1e10, clip=0.0):
    """the projection's cull decisions (fully_fused_projection_fwd.cu:96-176) on float64 values -> [N] bool, True = culled"""
    with np.errstate(all="ignore"):
        return ((z < near) | (z > far) | ~(det > 0) | (radius <= clip) | (m2[:, 0] + radius <= 0) | (m2[:, 0] - radius >= W)
                | (m2[:, 1] + radius <= 0) | (m2[:, 1] - radius >= H))


@functools.lru_cache(maxsize=None)
def wide_bwd_case(W, H, seed=SEED_WIDE):
    """Seeded cotangents, the oracle's projection adjoint on its own forward state (r0, c0) and the float64 autograd adjoint of the
    same loss (rows the oracle keeps).  `cmp` = visible rows away from a clamp limit (the adjoint is discontinuous there);
    `budget` = per-row condition budgets of the three gradients; `e_c64`, `budget_c64` = the same on the float64 conics."""
    case = wide_case(W, H, seed)
    N, g = case.N, case.g
    rng = np.random.default_rng(1)
    v_m2 = rng.normal(size=(N, 2)).astype(np.float32)
    v_d = rng.normal(size=N).astype(np.float32)
    v_c = (rng.normal(size=(N, 3)) * 0.1).astype(np.float32)
    e = orc.proj_bwd(g["means"], g["quats"], g["scales"], case.vm, case.K, W, H, case.r0, case.c0, v_m2, v_d, v_c)
    leaves, (tm2, tz, tconic, _, _) = torch_project64(case, requires_grad=True)
    mask = torch.tensor(case.r0 > 0)
    loss = ((tm2 * torch.tensor(v_m2))[mask].sum() + (tz * torch.tensor(v_d))[mask].sum() + (tconic * torch.tensor(v_c))[mask].sum())
    loss.backward()
    ref64 = tuple(x.grad.numpy() for x in leaves)
    vis = case.r0 > 0
    # per-row budgets from the oracle adjoint's own sensitivity to 1-ulp jitter of its float inputs (scenes.condition_budget)
    fn = lambda mm, qq, ss, cc, x, y, z: orc.proj_bwd(mm, qq, ss, case.vm, case.K, W, H, case.r0, cc, x, y, z)
    budget = scenes.condition_budget(fn, (g["means"], g["quats"], g["scales"], case.c0, v_m2, v_d, v_c), e)
    # the adjoint alone against float64: fed the float64 conics rounded to float32, so that every input is within half an ulp of
    # what autograd differentiates (c0 carries the forward's own rounding, amplified by the 2x2 inverse: up to 1.6 budgets on
    # v_scales), with the budgets taken around those inputs
    c64 = np.where(vis[:, None], tconic.detach().numpy(), 0.0).astype(np.float32)
    e_c64 = orc.proj_bwd(g["means"], g["quats"], g["scales"], case.vm, case.K, W, H, case.r0, c64, v_m2, v_d, v_c)
    budget_c64 = scenes.condition_budget(fn, (g["means"], g["quats"], g["scales"], c64, v_m2, v_d, v_c), e_c64)
    return SimpleNamespace(case=case, v_m2=v_m2, v_d=v_d, v_c=v_c, e=e, ref64=ref64, vis=vis, cmp=vis & ~case.cls["on_limit"],
                           budget=budget, e_c64=e_c64, budget_c64=budget_c64)


def plane_case(near=0.5, far=3.0):
    """Identity camera, one small Gaussian on the optical axis per depth around the two cull planes
    -> (means, quats, scales, viewmat, K, W, H, near, far, expected visibility)"""
    W, H = 96, 64
    f = np.float32
    z = np.array([np.nextafter(f(near), f(0)), f(near), np.nextafter(f(near), f(1)), np.nextafter(f(far), f(0)), f(far),
                  np.nextafter(f(far), f(9)), f(-1), f(0)], np.float32)
    means = np.stack([np.zeros_like(z), np.zeros_like(z), z], 1)
    quats = np.tile(np.array([1, 0, 0, 0], np.float32), (z.shape[0], 1))
    scales = np.full((z.shape[0], 3), 0.02, np.float32)
    keep = np.array([False, True, True, True, True, False, False, False])
    return means, quats, scales, np.eye(4, dtype=np.float32), scenes.intrinsics(W, H), W, H, near, far, keep


RADIUS_CLIPS = (3.0, 7.0, 20.5)
