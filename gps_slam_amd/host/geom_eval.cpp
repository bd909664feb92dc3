#include "geom_eval.hpp"

#include <cmath>

using namespace gpsh;

std::pair<torch::Tensor, torch::Tensor> nearestDistances(const torch::Tensor& query_in, const torch::Tensor& ref_in, torch::Tensor* stats_out) {
    for (const torch::Tensor* t : {&query_in, &ref_in})
        TORCH_CHECK(t->defined() && t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->dim() == 2 && t->size(1) == 3,
                    "nearestDistances: query and ref must be float32 device tensors [n,3]");
    auto query = query_in.contiguous(), ref = ref_in.contiguous();
    const int Q = (int)query.size(0), R = (int)ref.size(0);
    TORCH_CHECK(R > 0, "nearestDistances: the reference set is empty");
    const auto dev = query.device();
    auto dist2 = torch::empty({Q}, f32(dev));
    auto index = torch::empty({Q}, i32(dev));
    auto stats = torch::zeros({2}, i32(dev));
    const int64_t ib = gps_nn_index_workspace_bytes(R), qb = gps_nn_query_workspace_bytes(Q);
    auto iws = torch::empty({ib}, u8(dev)), qws = torch::empty({qb}, u8(dev));
    check(gps_nn_index_build(R, fptr(ref), iws.data_ptr(), ib, current_stream()), "gps_nn_index_build");
    check(gps_nn_query(R, iws.data_ptr(), Q, fptr(query), fptr(dist2), iptr(index), iptr(stats), qws.data_ptr(), qb, current_stream()),
          "gps_nn_query");
    if (stats_out) *stats_out = stats;
    return {torch::sqrt(dist2), index};
}

torch::Tensor surfaceUniforms(int64_t n, uint64_t seed) {
    auto gen = at::detail::createCPUGenerator(seed);
    return torch::rand({n, 3}, gen, torch::TensorOptions().dtype(torch::kFloat64));
}

std::pair<torch::Tensor, torch::Tensor> sampleSurface(const torch::Tensor& triangles, int64_t n, uint64_t seed, const torch::Tensor& uniforms) {
    TORCH_CHECK(triangles.defined() && triangles.dim() == 3 && triangles.size(0) > 0 && triangles.size(1) == 3 && triangles.size(2) == 3,
                "sampleSurface: triangles must be [T,3,3] with T > 0");
    auto tri = triangles.to(torch::kFloat64);
    auto u = (uniforms.defined() ? uniforms.to(torch::kFloat64) : surfaceUniforms(n, seed)).to(tri.device());
    auto p0 = tri.select(1, 0), e1 = tri.select(1, 1) - p0, e2 = tri.select(1, 2) - p0;
    auto c = [](const torch::Tensor& t, int k) { return t.select(1, k); };
    auto cx = c(e1, 1) * c(e2, 2) - c(e1, 2) * c(e2, 1);
    auto cy = c(e1, 2) * c(e2, 0) - c(e1, 0) * c(e2, 2);
    auto cz = c(e1, 0) * c(e2, 1) - c(e1, 1) * c(e2, 0);
    auto area = 0.5 * torch::sqrt(cx * cx + cy * cy + cz * cz);
    auto cum = torch::cumsum(area, 0);
    auto face = torch::searchsorted(cum, (c(u, 0) * cum[-1]).contiguous()).clamp_max(tri.size(0) - 1);
    auto a = c(u, 1), b = c(u, 2);
    auto flip = (a + b) > 1.0;
    auto a2 = torch::where(flip, 1.0 - a, a), b2 = torch::where(flip, 1.0 - b, b);
    auto pts = p0.index_select(0, face) + a2.unsqueeze(1) * e1.index_select(0, face) + b2.unsqueeze(1) * e2.index_select(0, face);
    return {pts.to(torch::kFloat32), face};
}

GeomEvalResult evalPointClouds(const torch::Tensor& rec_points, const torch::Tensor& gt_points, const torch::Tensor& transform,
                               const std::vector<double>& dist_thres, int64_t sample_nums, uint64_t seed) {
    TORCH_CHECK(rec_points.defined() && gt_points.defined() && rec_points.size(0) > 0 && gt_points.size(0) > 0, "evalPointClouds: empty point set");
    auto rec = rec_points;
    if (transform.defined()) {
        auto T = transform.to(rec.device(), torch::kFloat64).reshape({4, 4});
        rec = (rec.to(torch::kFloat64).matmul(T.slice(0, 0, 3).slice(1, 0, 3).t()) + T.slice(0, 0, 3).select(1, 3)).to(torch::kFloat32);
    }
    const int64_t P = rec.size(0);
    if (P > sample_nums) {   // (all P points otherwise: the reference's permutation of them changes no metric)
        auto gen = at::detail::createCPUGenerator(seed);
        auto pick = torch::randperm(P, gen, torch::TensorOptions().dtype(torch::kInt64)).slice(0, 0, sample_nums);
        rec = rec.index_select(0, pick.to(rec.device()));
    }
    rec = rec.contiguous();
    auto gt = gt_points.contiguous();
    auto d_acc = nearestDistances(rec, gt).first.to(torch::kFloat64);
    auto d_comp = nearestDistances(gt, rec).first.to(torch::kFloat64);
    GeomEvalResult out;
    out.accuracy_cm = d_acc.mean().item<double>() * 100.0;
    out.completion_cm = d_comp.mean().item<double>() * 100.0;
    out.dist_thres = dist_thres;
    out.n_rec = rec.size(0); out.n_gt = gt.size(0);
    for (double th : dist_thres) {
        const double p = 100.0 * (double)(d_acc < th).sum().item<int64_t>() / (double)d_acc.numel();
        const double r = 100.0 * (double)(d_comp < th).sum().item<int64_t>() / (double)d_comp.numel();
        out.accuracy_ratio.push_back(p);
        out.completion_ratio.push_back(r);
        out.f1.push_back(p + r > 0 ? 2.0 * p * r / (p + r) : 0.0);
    }
    return out;
}

AteResult ate(const torch::Tensor& est_c2w, const torch::Tensor& gt_c2w) {
    TORCH_CHECK(est_c2w.defined() && gt_c2w.defined() && est_c2w.dim() == 3 && gt_c2w.dim() == 3 && est_c2w.size(1) == 4 &&
                est_c2w.size(2) == 4 && gt_c2w.size(1) == 4 && gt_c2w.size(2) == 4, "ate: poses must be [n,4,4]");
    TORCH_CHECK(est_c2w.size(0) == gt_c2w.size(0), "ate: ", est_c2w.size(0), " estimated poses against ", gt_c2w.size(0), " ground-truth poses");
    TORCH_CHECK(est_c2w.size(0) >= 3, "ate: at least three poses are needed for a rigid alignment");
    const auto cpu64 = torch::TensorOptions().dtype(torch::kFloat64).device(torch::kCPU);
    // align(model = gt, data = est), [3,n]
    auto model = gt_c2w.to(cpu64).slice(1, 0, 3).select(2, 3).t().contiguous();
    auto data = est_c2w.to(cpu64).slice(1, 0, 3).select(2, 3).t().contiguous();
    auto mm = model.mean(1, true), dm = data.mean(1, true);
    auto W = (model - mm).matmul((data - dm).t());
    auto [U, d, Vh] = torch::linalg_svd(W.t(), true, c10::nullopt);
    (void)d;
    auto S = torch::eye(3, cpu64);
    if (torch::linalg_det(U).item<double>() * torch::linalg_det(Vh).item<double>() < 0) S[2][2] = -1.0;
    auto rot = U.matmul(S).matmul(Vh);
    auto trans = dm - rot.matmul(mm);
    auto err = rot.matmul(model) + trans - data;
    auto te = torch::sqrt((err * err).sum(0));
    AteResult out;
    out.ate_mean_cm = te.mean().item<double>() * 100.0;
    out.ate_rmse_cm = std::sqrt((te * te).mean().item<double>()) * 100.0;
    out.trans_error = te; out.rot = rot; out.trans = trans.select(1, 0).contiguous();
    return out;
}
