#include "image_eval.hpp"

using namespace gpsh;

ImageMetrics imageMetrics(const torch::Tensor& render_in, const torch::Tensor& gt_in, const torch::Tensor& depth_in) {
    TORCH_CHECK(render_in.defined() && gt_in.defined(), "imageMetrics: render and gt must be defined");
    TORCH_CHECK(render_in.is_cuda() && gt_in.is_cuda() && render_in.device() == gt_in.device(), "imageMetrics: render and gt must be on the same device");
    const auto dt = render_in.scalar_type();
    TORCH_CHECK(dt == torch::kUInt8 || dt == torch::kFloat32, "imageMetrics: images must be uint8 or float32");
    TORCH_CHECK(gt_in.scalar_type() == dt, "imageMetrics: render and gt must have the same dtype");
    TORCH_CHECK((render_in.dim() == 3 || render_in.dim() == 4) && render_in.size(-1) == 3, "imageMetrics: images must be [H,W,3] or [K,H,W,3]");
    TORCH_CHECK(render_in.sizes() == gt_in.sizes(), "imageMetrics: render is ", render_in.sizes(), ", gt is ", gt_in.sizes());
    auto render = (render_in.dim() == 3 ? render_in.unsqueeze(0) : render_in).contiguous();
    auto gt = (gt_in.dim() == 3 ? gt_in.unsqueeze(0) : gt_in).contiguous();
    const int64_t K = render.size(0), H = render.size(1), W = render.size(2);
    TORCH_CHECK(K > 0 && H > 0 && W > 0 && K <= INT32_MAX && H <= INT32_MAX && W <= INT32_MAX, "imageMetrics: empty or oversized images ", render.sizes());
    torch::Tensor depth;
    if (depth_in.defined()) {
        TORCH_CHECK(depth_in.is_cuda() && depth_in.device() == render.device() && depth_in.scalar_type() == torch::kFloat32,
                    "imageMetrics: depth must be a float32 tensor on the images' device");
        // the images' shape without the channel axis, or with a channel axis of one
        const auto lead = render_in.sizes().slice(0, render_in.dim() - 1);
        const auto ds = depth_in.sizes();
        TORCH_CHECK(ds == lead || (depth_in.dim() == render_in.dim() && ds.back() == 1 && ds.slice(0, ds.size() - 1) == lead),
                    "imageMetrics: depth is ", ds, " for images ", render_in.sizes());
        depth = depth_in.reshape({K, H, W}).contiguous();
    }
    const auto dev = render.device();
    const auto f64 = torch::TensorOptions().dtype(torch::kFloat64).device(dev);
    ImageMetrics out;
    out.mse = torch::empty({K}, f64);
    out.ssim = torch::empty({K}, f64);
    out.sse_u8 = torch::empty({K}, i64(dev));
    const int64_t wb = gps_image_metrics_workspace_bytes((int)K, (int)H, (int)W);
    auto ws = torch::empty({wb}, u8(dev));
    check(gps_image_metrics((int)K, (int)H, (int)W, dt == torch::kUInt8 ? GPS_IMAGE_U8 : GPS_IMAGE_F32, render.data_ptr(), gt.data_ptr(),
                            fptr(depth), ws.data_ptr(), wb, out.mse.data_ptr<double>(), out.ssim.data_ptr<double>(),
                            out.sse_u8.data_ptr<int64_t>(), current_stream()), "gps_image_metrics");
    out.psnr = 20.0 * torch::log10(torch::reciprocal(torch::sqrt(out.mse)));   // image_utils.py:21
    out.psnr_mean = out.psnr.mean().item<double>();
    out.ssim_mean = out.ssim.mean().item<double>();
    return out;
}
