// Geometry and trajectory evaluation in the C++ host: the reference's scripts/geo_general.py (accuracy, completion, their ratios
// and F1 between a reconstructed and a ground-truth cloud) and scripts/ate_general.py (rigidly aligned trajectory error).
// The nearest-neighbour search is device work (gps_nn_index_build / gps_nn_query, exact); sampling and the means run once per
// evaluation and are plain libtorch ops.  gps_slam_amd/geom_eval.py is the Python mirror: same operations, same numbers.
#pragma once
#include <utility>
#include <vector>

#include "gps_host_common.hpp"

// For every row of query[Q,3] the distance to, and the index of, the nearest row of ref[R,3] (float32 device tensors), on the
// current stream -> {dist float32[Q], index int32[Q]}.  Exact; ties go to the lowest index; a non-finite query gets (+inf, -1).
// stats (optional): int32[2] device tensor = queries finished by the grid / by the brute force.
std::pair<torch::Tensor, torch::Tensor> nearestDistances(const torch::Tensor& query, const torch::Tensor& ref,
                                                         torch::Tensor* stats = nullptr);

// the [n,3] float64 uniforms sampleSurface draws for `seed`: column 0 picks the triangle, 1 and 2 the point in it
torch::Tensor surfaceUniforms(int64_t n, uint64_t seed);
// n area-weighted points on triangles[T,3,3] (trimesh.sample.sample_surface as eval_pcd uses it) -> {points float32[n,3],
// triangle index int64[n]} on the triangles' device.  The same uniforms give the same points.
std::pair<torch::Tensor, torch::Tensor> sampleSurface(const torch::Tensor& triangles, int64_t n, uint64_t seed = 0,
                                                      const torch::Tensor& uniforms = torch::Tensor());

struct GeomEvalResult {   // eval_pcd's result dictionary (geo_general.py:82-90)
    double accuracy_cm = 0, completion_cm = 0;                      // mean distances rec -> gt, gt -> rec (float64 means)
    std::vector<double> dist_thres, accuracy_ratio, completion_ratio, f1;   // per threshold, percent
    int64_t n_rec = 0, n_gt = 0;
};
// eval_pcd (geo_general.py:37-90) on two clouds: rec_points is transformed ([4,4], identity when undefined) and sub-sampled
// without replacement to min(P, sample_nums).
GeomEvalResult evalPointClouds(const torch::Tensor& rec_points, const torch::Tensor& gt_points,
                               const torch::Tensor& transform = torch::Tensor(), const std::vector<double>& dist_thres = {0.03},
                               int64_t sample_nums = 1000000, uint64_t seed = 0);

struct AteResult {
    double ate_mean_cm = 0;   // what the reference prints as "ATE RMSE": the MEAN of the per-frame errors
    double ate_rmse_cm = 0;   // their root mean square
    torch::Tensor trans_error, rot, trans;   // float64: [n] metres, [3,3], [3]
};
// ate_general.py: align(gt, est) on the translations of two [n,4,4] pose lists (float64 SVD on the host).  Mismatched lengths or
// fewer than three poses throw.
AteResult ate(const torch::Tensor& est_c2w, const torch::Tensor& gt_c2w);
