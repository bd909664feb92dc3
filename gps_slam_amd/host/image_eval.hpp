// Image-quality evaluation in the C++ host: the per-view and averaged PSNR and SSIM of the reference's scripts/metric.py (which
// run/eval.py calls) and of its masked variant scripts/metric_general.py, on device tensors instead of image files.  One call of
// gps_image_metrics evaluates all K views; PSNR and the two means are a handful of float64 ops on [K].
// gps_slam_amd/image_eval.py is the Python mirror: same operations, same numbers.  LPIPS (the scripts' third number) needs
// pretrained VGG and linear-head weights and stays outside.
#pragma once
#include "gps_host_common.hpp"

struct ImageMetrics {
    torch::Tensor psnr, ssim, mse;    // float64 [K], on the images' device
    torch::Tensor sse_u8;             // int64 [K]: exact sum of squared level differences (uint8 input; 0 for float32)
    double psnr_mean = 0, ssim_mean = 0;   // what metric.py:59-60 prints: the mean over the views (float64 here; +inf if a view is)
};

// render, gt: [H,W,3] or [K,H,W,3], both uint8 or both float32, device tensors; depth (optional): float32 [K,H,W] or [K,H,W,1]
// ([H,W] / [H,W,1] for a single view) -- both images are multiplied by depth > 0 (metric_general.py:62-64: masked pixels are
// zeroed, not excluded).  Runs on the current stream.
//   psnr = 20 log10(1 / sqrt(mse)) in float64 (scripts/utils/image_utils.py:19-21), +inf where mse == 0
// Shape, dtype or device mismatches throw.
ImageMetrics imageMetrics(const torch::Tensor& render, const torch::Tensor& gt, const torch::Tensor& depth = torch::Tensor());

struct ImageEvalResult {   // results.json / per_view.json of metric.py as data
    std::vector<int> cam_ids;           // Camera::id per view, in call order
    std::vector<double> psnr, ssim;     // per view
    double psnr_mean = 0, ssim_mean = 0;
    ImageMetrics metrics;               // the tensors behind them
};
