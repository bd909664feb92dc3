"""Generates tests/golden/image_metrics_ref.npz from the REFERENCE'S OWN PYTHON (imported from /root/reference in the build
container; it cannot travel, so its outputs are committed as data):

  * scripts/utils/image_utils.py: psnr and scripts/utils/loss_utils.py: ssim, applied the way scripts/metric_general.py:59-66
    applies them per view: to_tensor (uint8 -> float32, .div(255), [1,3,H,W]), both images multiplied by depth > 0 when there is
    a depth, then psnr and ssim.  (metric_general.py itself cannot be imported here: torchvision and the LPIPS weights are absent.)

Every case is stored as K stacked views: <case>_render, <case>_gt uint8 [K,H,W,3], <case>_depth float32 [K,H,W] where the case is
masked, and per view the reference's results on float32 inputs (<case>_psnr_f32, <case>_ssim_f32) and the same calls on float64
inputs (<case>_psnr_f64, <case>_ssim_f64).  Images are smooth (a product of sinusoids per channel plus noise of ~6 levels, so that
the windowed variance is small somewhere and C2 matters); the render is the ground truth plus noise of ~9 levels.

    a         11 x 5    smaller than the 11-tap window in one axis, than a tile in both
    b         32 x 32   exactly one tile
    c         33 x 65   one pixel over the tile edge on both axes
    d         45 x 70   no mask
    d_masked  45 x 70   the images of d under a depth with a 14 x 20 hole (zeros, a NaN, a negative value) that straddles x = 32
                        and y = 32, and with image row 0 masked
    e         K = 4 at 45 x 70: view 0 is d_masked; view 1 other content under another hole; view 2 render == gt (PSNR +inf,
              SSIM 1); view 3 a depth that is zero everywhere (both images become 0: MSE 0, SSIM exactly 1)

Run from the repo root:  python tests/golden/make_image_metrics_golden.py"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = "/root/reference/scripts/utils"


def _load(name):
    spec = importlib.util.spec_from_file_location("refpy_" + name, os.path.join(REF, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def smooth_pair(rng, H, W):
    """(render, gt) uint8 [H,W,3]"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    gt = np.empty((H, W, 3))
    for c in range(3):
        fy, fx = rng.uniform(0.03, 0.12, size=2)
        py, px = rng.uniform(0, 2 * np.pi, size=2)
        gt[..., c] = 128.0 + 100.0 * np.sin(fy * y + py) * np.sin(fx * x + px)
    gt += rng.normal(scale=6.0, size=gt.shape)
    gt8 = np.clip(np.rint(gt), 0, 255).astype(np.uint8)
    render8 = np.clip(np.rint(gt8 + rng.normal(scale=9.0, size=gt.shape)), 0, 255).astype(np.uint8)
    return render8, gt8


def positive_depth(rng, H, W):
    return rng.uniform(0.5, 4.0, size=(H, W)).astype(np.float32)


def reference_view(image_utils, loss_utils, render8, gt8, depth, dt):
    """metric_general.py:59-66 on one view"""
    to_tensor = lambda a: torch.from_numpy(a).permute(2, 0, 1).contiguous().to(dt).div(255).unsqueeze(0)[:, :3, :, :]
    render_img, gt_img = to_tensor(render8), to_tensor(gt8)
    if depth is not None:
        depth_img = torch.from_numpy(depth)[None, None]
        render_img = render_img * (depth_img > 0)
        gt_img = gt_img * (depth_img > 0)
    assert render_img.dtype == dt and gt_img.dtype == dt
    return float(image_utils.psnr(render_img, gt_img)), float(loss_utils.ssim(render_img, gt_img))


def main():
    loss_utils, image_utils = _load("loss_utils"), _load("image_utils")
    rng = np.random.default_rng(20261019)
    cases = {}   # name -> (render[K,H,W,3], gt, depth[K,H,W] or None)
    for name, (H, W) in (("a", (11, 5)), ("b", (32, 32)), ("c", (33, 65)), ("d", (45, 70))):
        r, g = smooth_pair(rng, H, W)
        cases[name] = (r[None], g[None], None)
    H, W = 45, 70
    d0 = positive_depth(rng, H, W)
    d0[25:39, 22:42] = 0.0          # 14 rows x 20 columns across y = 32 and x = 32
    d0[30, 30] = np.nan
    d0[31, 33] = -1.5
    d0[0, :] = 0.0
    cases["d_masked"] = (cases["d"][0], cases["d"][1], d0[None])
    r1, g1 = smooth_pair(rng, H, W)
    d1 = positive_depth(rng, H, W)
    d1[5:20, 50:70] = 0.0           # touches the right image edge
    _, g2 = smooth_pair(rng, H, W)
    r3, g3 = smooth_pair(rng, H, W)
    cases["e"] = (np.stack([cases["d"][0][0], r1, g2, r3]), np.stack([cases["d"][1][0], g1, g2, g3]),
                  np.stack([d0, d1, positive_depth(rng, H, W), np.zeros((H, W), np.float32)]))
    out = {}
    for name, (render, gt, depth) in cases.items():
        out[name + "_render"], out[name + "_gt"] = render, gt
        if depth is not None:
            out[name + "_depth"] = depth
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            res = [reference_view(image_utils, loss_utils, render[k], gt[k], None if depth is None else depth[k], dt) for k in range(len(render))]
            out["%s_psnr_%s" % (name, tag)] = np.array([p for p, _ in res], np.float64)
            out["%s_ssim_%s" % (name, tag)] = np.array([s for _, s in res], np.float64)
        print(name, render.shape, "psnr f64", out[name + "_psnr_f64"], "f32 - f64", out[name + "_psnr_f32"] - out[name + "_psnr_f64"],
              "ssim f64", out[name + "_ssim_f64"], "f32 - f64", out[name + "_ssim_f32"] - out[name + "_ssim_f64"])
    assert np.isposinf(out["e_psnr_f64"][2:]).all() and (out["e_ssim_f64"][2:] == 1.0).all()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_metrics_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
