"""Image-quality evaluation: the per-view and averaged PSNR and SSIM of the reference's scripts/metric.py (which run/eval.py calls)
and of its masked variant scripts/metric_general.py, on device tensors instead of image files.

    image_metrics   K views against their ground truth in one gps_image_metrics call (csrc/image_metrics.hip)

Mirror of host/image_eval.{hpp,cpp}: same arguments, same operations, same numbers.  The Python SLAMPipeline has no
renderEvalImgs, so it gets no evalImages either: render the views with the model and pass the tensors here.  LPIPS, the scripts'
third number, needs pretrained VGG and linear-head weights and stays outside the library.
"""
import ctypes as C

import torch

from ._lib import check, lib

IMAGE_U8, IMAGE_F32 = 0, 1   # GPS_IMAGE_U8 / GPS_IMAGE_F32


def image_metrics(render, gt, depth=None):
    """render, gt: [H,W,3] or [K,H,W,3] device tensors, both uint8 (what the reference measures: u8 / 255) or both float32;
    depth (optional): float32 [K,H,W] or [K,H,W,1] ([H,W] / [H,W,1] for one view) -- both images are multiplied by depth > 0
    (metric_general.py:62-64: masked pixels are zeroed, NOT excluded) -> dict(psnr, ssim, mse float64[K], sse_u8 int64[K] on the
    device, psnr_mean, ssim_mean floats).  psnr = 20 log10(1 / sqrt(mse)) in float64 (image_utils.py:19-21), +inf where mse == 0;
    the means are those metric.py:59-60 prints.  Runs on the current stream."""
    if not (torch.is_tensor(render) and torch.is_tensor(gt) and render.is_cuda and gt.is_cuda and render.device == gt.device):
        raise ValueError("image_metrics: render and gt must be tensors on the same device")
    if render.dtype not in (torch.uint8, torch.float32) or gt.dtype != render.dtype:
        raise ValueError("image_metrics: images must both be uint8 or both float32")
    if render.dim() not in (3, 4) or render.shape[-1] != 3 or render.shape != gt.shape:
        raise ValueError("image_metrics: images must be [H,W,3] or [K,H,W,3] of one shape, got %s and %s" % (tuple(render.shape), tuple(gt.shape)))
    lead = tuple(render.shape[:-1])
    r4 = (render.unsqueeze(0) if render.dim() == 3 else render).contiguous()
    g4 = (gt.unsqueeze(0) if gt.dim() == 3 else gt).contiguous()
    K, H, W = (int(v) for v in r4.shape[:3])
    if min(K, H, W) <= 0:
        raise ValueError("image_metrics: empty images %s" % (tuple(render.shape),))
    d = None
    if depth is not None:
        if not (torch.is_tensor(depth) and depth.is_cuda and depth.device == render.device and depth.dtype == torch.float32):
            raise ValueError("image_metrics: depth must be a float32 tensor on the images' device")
        if tuple(depth.shape) not in (lead, lead + (1,)):   # the images' shape without the channel axis, or with a channel axis of one
            raise ValueError("image_metrics: depth is %s for images %s" % (tuple(depth.shape), tuple(render.shape)))
        d = depth.reshape(K, H, W).contiguous()
    dev = r4.device
    mse = torch.empty(K, dtype=torch.float64, device=dev)
    ssim = torch.empty(K, dtype=torch.float64, device=dev)
    sse_u8 = torch.empty(K, dtype=torch.int64, device=dev)
    wb = int(lib.gps_image_metrics_workspace_bytes(K, H, W))
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    check(lib.gps_image_metrics(K, H, W, IMAGE_U8 if r4.dtype == torch.uint8 else IMAGE_F32, r4.data_ptr(), g4.data_ptr(),
                                d.data_ptr() if d is not None else None, ws.data_ptr(), wb, mse.data_ptr(), ssim.data_ptr(),
                                sse_u8.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "gps_image_metrics")
    psnr = 20.0 * torch.log10(torch.reciprocal(torch.sqrt(mse)))   # image_utils.py:21
    return dict(psnr=psnr, ssim=ssim, mse=mse, sse_u8=sse_u8, psnr_mean=float(psnr.mean()), ssim_mean=float(ssim.mean()))
