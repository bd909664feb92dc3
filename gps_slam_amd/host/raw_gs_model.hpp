// RawGaussianModel (include/raw_gs_model.h:16-258, src/raw_gs_model.cpp) and SLAMGaussianModel::addGaussians
// (slam/slam_gs_model.cpp:5-56) on the C-ABI.
//
// Two routes through one optimise iteration, same kernels underneath:
//   * the reference's call sequence  forward() -> computeLoss() -> loss.backward() -> optimizersStep() ->
//     optimizersZeroGrad()  works unchanged: in grad mode gesForward returns tensors whose grad_fn runs the fused
//     backward chain (raster bwd -> preprocess bwd) and leaves the gradients in the parameters' .grad();
//   * trainStep() is the same iteration as ONE C-ABI call (gps_splat_train_step: 10 launch sites, no host sync, no
//     autograd graph) -- what SLAMPipeline::localOptimize uses.
#pragma once
#include "config_fields.hpp"
#include "random_selector.hpp"
#include "raw_gs_param.hpp"

class RawGaussianModel {
public:
    RawGaussianModel() = default;
    ~RawGaussianModel() = default;

    void loadConfig(const gpsh::Config& config);  // MODEL section keys of configs/release/*/*.yaml
    // the reference's signature (raw_gs_model.h:24, N = YAML::Node; gpsh::Node of config_node.hpp reads the same files): the MODEL
    // node.  Keys the reference reads are required, this project's own are optional, and with gpsh::Node an unknown key throws
    // (config_fields.hpp).  The node is flattened and goes through loadConfig(const gpsh::Config&): one list of keys, configFields.
    template <class N> void loadConfig(const N& model_node);
    template <class V> void configFields(V& v, int64_t& capacity);
    template <class N> gpsh::Config flattenConfig(const N& model_node);   // every conversion and check of loadConfig(node), nothing assigned
    void updateSH(int curr_iter = -1);            // raw_gs_model.h:30-36

    // raw_gs_model.h:38-50.  -> {"rgb"[H,W,3], "depth"[H,W,1], "alpha"[H,W,1], "radiis"[N], "means2d"[N,2]}
    TensorDict forward(const Camera& cam, const torch::Tensor& ref_depth = torch::Tensor(),
                       const torch::Tensor& base_color = torch::Tensor());
    TensorDict gesForward(const Camera& cam, const torch::Tensor& ref_depth, const torch::Tensor& base_color);
    TensorDict rawForward(const Camera& cam);  // raw_gs_model.cpp:43-185 (render_method "raw")
    // raw_gs_model.cpp:369-417 with the weights every shipped config uses (L1 only; ssim / depth weights 0):
    // -> {"loss", "l1_loss"}
    TensorDict computeLoss(TensorDict& render_res, const Camera& cam, const gpsh::Config& weight_configs,
                           const torch::Tensor& mask = torch::Tensor());
    // raw_gs_model.h:52 with the PIPE.weight_configs node (ssim_weight, depth_weight: both required, as the reference reads them)
    template <class N> TensorDict computeLoss(TensorDict& render_res, const Camera& cam, const N& weight_configs,
                                              const torch::Tensor& mask = torch::Tensor());
    template <class V> static void lossWeightFields(V& v, float& ssim_weight, float& depth_weight) {
        v.f("ssim_weight", ssim_weight);
        v.f("depth_weight", depth_weight);
    }

    // raw_gs_model.h:68-83: the parameters as a libtorch archive / 3DGS PLY.  loadParamsTensor leaves a model forward() can render
    // at once: the rows go into the capacity loadConfig reserved (grown if the file holds more), the exposure table is the
    // file's, there are no optimisers (initOptimizers() starts training afresh).
    void saveParamsTensor(const std::string& filename) { opt_gs_params.saveTensor(filename); }
    void saveParamsPly(const std::string& filename) { opt_gs_params.savePly(filename); }
    void loadParamsTensor(const std::string& filename);

    // One optimise iteration as a single C-ABI call; the L1 loss accumulates in lossSum().
    // next_cam (optional): the camera of the NEXT trainStep() -- its preprocessing forward then runs in the tail of this step's
    // backward + Adam kernel (gps_splat_step::next_viewmat) and that next call skips its preprocessing launch, provided it comes
    // with exactly that camera and nothing else has used the model in between (any other launch on the step buffers disarms it).
    // weight_configs (optional; computeLoss's keys ssim_weight / depth_weight): with a non-zero weight the step carries those loss
    // terms as well (gps_splat_step::ssim_weight ..; cam.depth is used only when cam.has_depth); lossSum() then HOLDS the total
    // of this step and lossTerms() = {total, L1 mean, 1 - mean SSIM, depth L1}.  The empty config is the L1 step.  Not together
    // with an exposure row of the camera (the operator route forward -> computeLoss -> backward serves that combination).
    void trainStep(const Camera& cam, const torch::Tensor& ref_depth, const torch::Tensor& base_color,
                   const torch::Tensor& ref_depth_clamped = torch::Tensor(), const Camera* next_cam = nullptr,
                   const gpsh::Config& weight_configs = gpsh::Config());
    torch::Tensor lossSum() const { return B_.loss; }
    torch::Tensor lossTerms() const { return loss_terms_; }   // [4], undefined before the first step with loss terms

    // Allocate everything an iteration at this image size needs (intermediates, Adam state) now instead of lazily on the
    // first forward / initOptimizers -- keeps one-off hipMalloc + memset time out of the frame loop.
    void reserveWorkspace(int width, int height);
    // Capacity check of the binning buffers, meant for a point where the host synchronises anyway (once per keyframe:
    // SLAMPipeline::removeRedundantGs).  The kernels clamp n_isects / n_groups to the buffer capacities and raise a sticky
    // device flag where the reference would have allocated exact sizes (isect_tiles_no_depth.cu:238-262); this reads it back.
    // Overflow since the last check -> throws (Gaussians were dropped from a render / backward); more than half of a
    // capacity in use -> the buffers are doubled before the next iteration.  Returns {n_isects, n_groups} of the last launch.
    std::pair<int64_t, int64_t> checkBinningCapacity();
    // raw_gs_model.cpp:654-675.  max_iterations > 0: the means' rate decays to 0.01 x its start over that many schedulersStep()
    // calls (meansOptScheduler, gpsh::OptimScheduler); <= 0: constant rates
    void initOptimizers(int max_iterations = -1, float scene_scale = 1);
    // raw_gs_model.h:167-173: one step of the means' scheduler (nothing without one).  The next trainStep() / optimizersStep() is
    // handed the new rate the way the constant one is: lrs_[0] through the step struct / the Adam segment
    void schedulersStep() { means_scheduler_.step(lrs_[0]); }
    bool hasScheduler() const { return means_scheduler_.active; }
    double meansLr() const { return lrs_[0]; }
    int adamStep() const { return adam_step_; }
    void optimizersZeroGrad();
    void optimizersStep();
    void prunePoints(const torch::Tensor& deleteMask);  // raw_gs_model.cpp:635-644 (+ removeFromOptimizer)
    int64_t pruneKeep(const torch::Tensor& keepMask);   // prunePoints(~keepMask); returns the number of Gaussians kept
    void setParamsRequireGrad();

    // ---- densification (raw_gs_model.cpp:419-633), driven by SLAMPipeline::rawTrainCams ----
    // stepPostBackward: the reference's control flow.  While curr_iter < densify_end_iter: the statistics of updateDensifyGrad
    // from render_res["means2d"].grad() (retain_grad() before backward) and render_res["radiis"] in ONE launch
    // (gps_densify_accumulate); densifiyGs + cleared statistics when curr_iter % densify_interval == 0 && curr_iter >
    // densify_start_iter; the opacity reset when curr_iter % reset_opacity_interval == 0 -- at iteration 0 too (0 % k == 0), as
    // the reference has it: logits clamped to at most logit(2 prune_opacity_thres), the opacity moments zeroed, the step count kept.
    void stepPostBackward(TensorDict& render_res, const Camera& cam, float scene_scale, int curr_iter);
    void updateDensifyGrad(TensorDict& render_res, const Camera& cam);
    // clone / split / prune as ONE plan (gps_densify_plan), ONE stream synchronise for its five counts and ONE out-of-place pass
    // over parameters and Adam moments (gps_densify_apply) into the alternate buffers, which then become the model: see
    // include/gps_slam_hip.h for the layout (the reference's cat + order-preserving prune).  Grows every capacity-sized buffer
    // when the new count exceeds the capacity (the parameters' own policy: at least double, at least 2^19 rows); contents and the
    // step count survive.  split_samples [2 n_split, 3]: the normal draws (the reference: torch::randn); without them they come
    // from the generator of setDensifySeed(), or the default one.  Nothing happens while curr_iter % reset_opacity_interval <
    // pause_refine_after_reset (raw_gs_model.cpp:513).  Returns the counts {M, n_split, n_split_surviving, n_dup_surviving, n_keep}
    // (empty when paused or when the model is empty).
    std::vector<int64_t> densifiyGs(float scene_scale, int curr_iter, const c10::optional<torch::Tensor>& split_samples = c10::nullopt);
    void resetOpacities();
    void setDensifySeed(int64_t seed);   // a host generator for the split samples: the same on every device
    // the statistics as [:N] views {grad_sum, vis_count} (zero until something is accumulated); the caller may write them
    std::vector<torch::Tensor> densifyStats();
    torch::Tensor lastSplitSamples() const { return last_split_samples_; }   // the draws of the last densifiyGs that split (undefined: none yet)
    int densify_start_iter = 500, densify_end_iter = 6000, densify_interval = 100, reset_opacity_interval = 3000;
    float densify_grad_thres = 0.0002f, densify_large_thres = 0.01f, prune_opacity_thres = 0.005f;
    int pause_refine_after_reset = 0;    // raw_gs_model.h: a member, no key
    int64_t densify_events = 0;          // densifiyGs calls that changed the model
    // what stepPostBackward did, for callers that want to see the schedule: {curr_iter, M, n_split, n_split_surviving,
    // n_dup_surviving, n_keep} per densifiyGs it ran (paused calls: {curr_iter}), and the iterations of its opacity resets
    std::vector<std::vector<int64_t>> densify_log;
    std::vector<int> opacity_reset_log;

    RawGaussianParams& getGaussianParms() { return opt_gs_params; }
    int getMaxSH() const { return maxSH; }
    torch::Tensor getMeans() { return opt_gs_params.getMeans(); }
    torch::Tensor getScales() { return opt_gs_params.getScales(); }
    torch::Tensor getQuats() { return opt_gs_params.getQuats(); }
    torch::Tensor getFeaturesDc() { return opt_gs_params.getFeaturesDc(); }
    torch::Tensor getFeaturesRest() { return opt_gs_params.getFeaturesRest(); }
    torch::Tensor getOpacities() { return opt_gs_params.getOpacities(); }
    torch::Tensor getRealMeans() { return opt_gs_params.getRealMeans(); }
    torch::Tensor getRealScales() { return opt_gs_params.getRealScales(); }
    torch::Tensor getRealOpacities() { return opt_gs_params.getRealOpacities(); }
    int getGaussianNum() { return opt_gs_params.getGaussianNum(); }
    std::string getRenderMethod() const { return render_method; }
    std::vector<torch::Tensor> grads();  // gradients of the last iteration, reference parameter order
    // the autograd route's gradients (the parameter leaves' .grad() after backward(), before optimizersZeroGrad()); undefined
    // tensors where autograd has built no graph
    std::vector<torch::Tensor> leafGrads() {
        std::vector<torch::Tensor> out;
        for (auto& t : leaf_) out.push_back(t.grad());
        return out;
    }
    // Adam state as [:N] views: {exp_avg x 6, exp_avg_sq x 6} in reference parameter order (empty before initOptimizers).
    // UNDEFINED between initOptimizers() and the first step: initOptimizers does not zero the buffers -- step 1 of every route
    // (gps_splat_train_step in all three fuse modes, gps_adam_step) takes m = v = 0 without reading them and writes every live row
    // (tests: test_first_step_after_init_optimizers_does_not_read_the_moments, test_adam_step_one_writes_the_moments_without_
    // reading_them, tests/test_adam_libtorch_gpu.py with NaN-filled buffers).  A caller that steps only SOME tensors at step 1, or
    // starts an optimiser at adam_step != 1, must zero them itself.
    std::vector<torch::Tensor> adamState() {
        std::vector<torch::Tensor> out;
        if (!have_opt_) return out;
        applyPendingPrunes();
        const int64_t N = opt_gs_params.getGaussianNum();
        for (auto* vec : {&adam_m_, &adam_v_}) for (auto& t : *vec) out.push_back(t.slice(0, 0, N));
        return out;
    }

    // Per-frame exposure (use_exposure; raw_gs_model.cpp:331-346, :672): the table [F,3,4], its gradient of the last iteration
    // (zero outside the camera's row) and its Adam moments {exp_avg, exp_avg_sq} as [:F] views (empty before initOptimizers;
    // rows the optimiser has not stepped yet are undefined, as in adamState()).  The table has its own step count.
    torch::Tensor getExposure() { return opt_gs_params.getExposure(); }
    torch::Tensor exposureGrad();
    std::vector<torch::Tensor> exposureAdamState();
    int exposureStep() const { return exp_step_; }
    // the camera's row of the table, or -1: exposure off, or cam.id outside [0, F)
    int exposureRow(const Camera& cam) const {
        return use_exposure && cam.id >= 0 && cam.id < opt_gs_params.exposureRows() ? cam.id : -1;
    }

    static torch::Tensor clampRefDepth(const torch::Tensor& ref_depth);  // raw_gs_model.cpp:205-207

    RawGaussianParams opt_gs_params;
    torch::Device device = torch::kCUDA;

    // raw_gs_model.h:283-288 + MODEL section defaults (configs/release/replica/office0.yaml)
    int maxSH = 3, degreesToUse = 3, shDegreeInterval = 0;
    int max_gs_radii = 100, tile_size = 16;
    float eps2d = 0.3f, near_plane = 0.01f, far_plane = 1e10f, radius_clip = 0.0f, delta_depth = 0.1f;
    float maxInitScale = 0.01f, minInitScale = -1.0f, defaultOpacities = 0.5f;
    double means_lr = 1.6e-4, scales_lr = 5e-3, quats_lr = 1e-3, featuresDc_lr = 2.5e-3, featuresRest_lr = 5e-4,
           opacities_lr = 5e-2;
    int64_t isect_capacity = 0;  // 0 -> max(1M, 16 * capacity)
    int64_t binning_overflows = 0;  // how often checkBinningCapacity() found the sticky overflow flag raised (and grew the buffers)
    // trainStep: step featuresRest inside the backward kernel (its gradient never reaches HBM; grads()[4] is then stale).
    // The parameter update is bit-identical either way.
    bool fuse_sh_rest_adam = true;
    // trainStep's binning + backward rasterizer: superblock counting sort + column strips (gps_splat_step::v_rows .. set), or
    // the sorted-key binning + 32-pixel-group kernel of the operator-level entry points
    bool strip_backward = true;
    bool use_exposure = false;   // MODEL keys use_exposure / exposure_lr (configs/release/*/*.yaml:101-102)
    double exposure_lr = 0.003;
    std::string render_method = "ges";
    bool abs_grad = false;       // raw_gs_model.h:293
    // rawForward's rasterizer backward without float atomics (gps_raster_raw_bwd_ordered): the same inputs give the same bits, at
    // the price of a sort and a second pass.  SLAMPipeline::rawTrainCams switches it on: two runs with one seed end bit-identical
    bool ordered_raw_backward = false;
    torch::Tensor backgrounds;   // raw_gs_model.h:295 ([1,4] device tensor; undefined = none)

    // implementation detail, public for the autograd node
    struct Buffers {
        torch::Tensor radii, means2d, depths, conics, colors, opacities, records, tiles_per_gauss, flatten_ids,
            group_gs_ids, group_starts, tile_offsets, counts, workspace, render_colors, weight_sum, rgb, depth, loss,
            v_render_colors, v_render_alphas, v_means2d, v_conics, v_colors, v_opacities,
            v_rows, pix2, cls_ids, cls_counts;   // the strip backward's buffers (strip_backward)
    };
    gps_splat_step& stepStruct(int W, int H);
    void bindCamera(gps_splat_step& st, const Camera& cam, const torch::Tensor& ref_depth_clamped,
                    const torch::Tensor& base_color, const torch::Tensor& gt_rgb, bool consumes_prefetch = false);
    Buffers& buffers() { return B_; }
    // Every launch that overwrites the per-launch intermediates (radii, means2d, conics, colors, the tile / group tables, the
    // render) gets a new id.  The grad-mode forward stamps it into its autograd node; its backward reads those intermediates
    // and refuses to run if another launch has replaced them in between.
    int64_t launchId() const { return launch_id_; }
    int64_t nextLaunchId() { return ++launch_id_; }
    // the forward the last trainStep() ran ahead for its next_cam: camera arrays, Gaussian count, image size (viewmat == nullptr: none)
    struct PrefetchKey {
        uint64_t camera = 0;   // Camera::pack_serial() of the camera the forward was run for; 0 = nothing run ahead
        int64_t N = 0;
        int W = 0, H = 0;
        uint64_t version = 0;  // RawGaussianParams::version(): an add / prune between the two steps voids the forward run ahead
        int sh_degree = -1;    // the degree the colours were evaluated with: an updateSH() between the two steps voids it as well
        bool operator==(const PrefetchKey& o) const {
            return camera == o.camera && N == o.N && W == o.W && H == o.H && version == o.version && sh_degree == o.sh_degree;
        }
    };
    PrefetchKey prefetched_;

protected:
    Buffers B_;
    gps_splat_step step_{};
    int64_t step_cap_ = -1;
    int64_t launch_id_ = 0;
    int step_w_ = 0, step_h_ = 0;
    // Adam state: capacity-sized exp_avg / exp_avg_sq / grad buffers in reference parameter order + step count
    std::vector<torch::Tensor> adam_m_, adam_v_, adam_g_;
    double lrs_[RawGaussianParams::NUM] = {0, 0, 0, 0, 0, 0};
    gpsh::OptimScheduler means_scheduler_;
    int64_t adam_cap_ = -1;
    int adam_step_ = 0;
    bool have_opt_ = false;
    // exposure table: Adam state / gradient sized like the table's capacity buffer, the slab of per-workgroup d E partials, the
    // step count, and the autograd leaf of the grad-mode forward
    torch::Tensor exp_m_, exp_v_, exp_g_, exp_slab_, exp_leaf_;
    int exp_step_ = 0;
    int64_t exp_state_rows_ = 0;   // rows whose moments the optimiser has written (rows appended since start from zero)
    double exp_lr_ = 0;
    void exposureState();          // (re)size the table's optimiser buffers to the table's capacity
    torch::Tensor exposureSlab(int W, int H);
    torch::Tensor loss_terms_, loss_ws_;   // trainStep with loss terms: the four terms and gps_loss_terms' workspace
    std::vector<torch::Tensor> leaf_;  // parameter leaves handed to autograd by the last grad-mode forward
    std::vector<torch::Tensor> keep_;  // inputs of the last launch, kept alive until the next one
    struct PendingPrune { torch::Tensor keep; int64_t n_before; };
    std::vector<PendingPrune> pending_prunes_;  // prunePoints' Adam-state compactions not carried out yet
    void applyPendingPrunes();
    torch::Tensor grad_sum_, vis_count_;   // densification statistics, capacity sized (zero = cleared)
    torch::Tensor densify_host_counts_;    // pinned words gps_densify_plan reports its counts in
    c10::optional<at::Generator> densify_gen_;
    torch::Tensor last_split_samples_;
    void densifyStatBuffers();
    torch::Tensor host_count_;         // pinned word the mask compaction reports its count in (addGaussians)
    torch::Tensor host_subset_;        // pinned staging buffer of the sampled subset
};

class SLAMGaussianModel : public RawGaussianModel {
public:
    // slam_gs_model.cpp:5-56: sample new Gaussians where sample_mask is set.  frame_maps: "vertex_map", "normal_map".
    // Returns the number of Gaussians added.  `seed_gen` drives the random subset (host generator: n is host-known).
    int addGaussians(const Camera& cam, const TensorDict& frame_maps, const torch::Tensor& sample_mask,
                     float new_gs_sample_ratio, int frame_num, c10::optional<at::Generator> seed_gen = c10::nullopt);
};

// THE list of MODEL keys (src/raw_gs_model.cpp:11-40 of the reference + this project's own), for every route (config_fields.hpp)
template <class V>
void RawGaussianModel::configFields(V& v, int64_t& capacity) {
    v.s("render_method", render_method);
    v.i("sh_degree", maxSH);
    v.f("max_init_scale", maxInitScale);
    v.f("min_init_scale", minInitScale);
    v.i("sh_degree_interval", shDegreeInterval);
    v.f("default_opacities", defaultOpacities);
    // (the reference narrows the rates to float before AdamOptions widens them again; they have been doubles here from the start)
    v.d("means_lr", means_lr);
    v.d("scales_lr", scales_lr);
    v.d("quats_lr", quats_lr);
    v.d("featuresDc_lr", featuresDc_lr);
    v.d("featuresRest_lr", featuresRest_lr);
    v.d("exposure_lr", exposure_lr);
    v.b("use_exposure", use_exposure);
    v.d("opacities_lr", opacities_lr);
    v.i("max_gs_radii", max_gs_radii);
    v.f("delta_depth", delta_depth);
    // this project's
    v.i64("isect_capacity", isect_capacity, gpsh::kOptional);
    v.b("fuse_sh_rest_adam", fuse_sh_rest_adam, gpsh::kOptional);
    v.b("strip_backward", strip_backward, gpsh::kOptional);
    v.i64("capacity", capacity, gpsh::kOptional);
    // densification (stepPostBackward / densifiyGs read them from the node when they run, raw_gs_model.cpp:423-427, :505-510: a
    // file without them loads, so they are optional here)
    v.i("densify_start_iter", densify_start_iter, gpsh::kOptional);
    v.i("densify_end_iter", densify_end_iter, gpsh::kOptional);
    v.i("densify_interval", densify_interval, gpsh::kOptional);
    v.f("densify_grad_thres", densify_grad_thres, gpsh::kOptional);
    v.f("densify_large_thres", densify_large_thres, gpsh::kOptional);
    v.i("reset_opacity_interval", reset_opacity_interval, gpsh::kOptional);
    v.f("prune_opacity_thres", prune_opacity_thres, gpsh::kOptional);
    // in every shipped file, used by nothing: the scheduler's final rate is 0.01 x the start (raw_gs_model.cpp:673), and
    // densifiyGs reads split_screen_size into a local it never uses (:508)
    for (const char* k : {"means_lr_final", "split_screen_size"}) v.ignored(k);
}

template <class N>
gpsh::Config RawGaussianModel::flattenConfig(const N& model_node) {
    int64_t capacity = 0;
    return gpsh::flattenNode(model_node, "MODEL", [&](auto& v) { configFields(v, capacity); });
}

template <class N>
void RawGaussianModel::loadConfig(const N& model_node) { loadConfig(flattenConfig(model_node)); }

template <class N>
TensorDict RawGaussianModel::computeLoss(TensorDict& render_res, const Camera& cam, const N& weight_configs, const torch::Tensor& mask) {
    float ssim = 0.f, depth = 0.f;
    return computeLoss(render_res, cam, gpsh::flattenNode(weight_configs, "PIPE.weight_configs",
                                                          [&](auto& v) { lossWeightFields(v, ssim, depth); }), mask);
}
