// SLAMPipeline (slam/slam_pipeline.{h,cpp}): the per-frame loop that drives the hot path.
//
//    SLAMTrainCams      :52-173   per frame: TSDF ProcessFrame; every local_opt_interval frames:
//    localFrameRaycast  :417-448  runRaycastByCam for the <= 2 window frames
//    keyFrameRaycast    :528-561  + <= 7 random keyframes
//    initNewGaussians   :450-526  error-mask sampling -> addGaussians
//    localOptimize      :195-289  20 x (forward, L1, backward, 7 x Adam)
//    removeRedundantGs  :564-586  prune by scale / opacity
//
// All compute goes through the C-ABI (RawGaussianModel, TsdfEngine); this file is bookkeeping.  Random choices the
// reference seeds from std::random_device (dataset_reader.h:39) are seeded here so that runs are reproducible.
#pragma once
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>
#include <random>

#include "raw_gs_model.hpp"
#include "infinitam_tools.hpp"
#include "tsdf_engine.hpp"
#include "image_eval.hpp"

// dataset_reader.h:26-100 (uniform branch): draw without replacement, refill when exhausted
template <class T>
class RandomSelector {
public:
    RandomSelector(const std::vector<T>& items, std::mt19937_64& rng) : rng_(rng) {
        for (size_t i = 0; i < items.size(); i++) original_.push_back({(int)i, &items[i]});
        current_ = original_;
    }
    std::pair<int, const T*> getNext() {
        if (current_.empty()) current_ = original_;
        std::uniform_int_distribution<size_t> d(0, current_.size() - 1);
        const size_t i = d(rng_);
        auto v = current_[i];
        current_[i] = current_.back();
        current_.pop_back();
        return v;
    }

private:
    std::vector<std::pair<int, const T*>> original_, current_;
    std::mt19937_64& rng_;
};

// include/file_utils.h:35, src/file_utils.cpp:172-210: device memory in use, MiB (the reference asks NVML for `memory.used`; here
// hipMemGetInfo of the device: total - free, the same quantity -- every process's allocations on that GPU)
unsigned long long getGPUMemoryUsage(int gpu_id = 0);
torch::Tensor computeNormalMap(const torch::Tensor& vertex_map);  // src/tensor_math.cpp:278-300 -> gps_normal_map

struct ihipEvent_t;                     // (hipEvent_t's pointee: this header includes no HIP headers)
using RaycastEvent = ihipEvent_t*;

class SLAMPipeline {
public:
    // use_gt_pose: TSDF.use_gt_pose of the configs (true in every shipped one) -> engine->turnOffTracking(), as
    // createTsdfEngine does (InfiniTAM_tools.cpp:59-62); false keeps the depth tracker active
    SLAMPipeline(TsdfEngine* tsdf_engine, SLAMGaussianModel* model, uint64_t seed = 1234, bool use_gt_pose = true);
    // the reference's construction sequence (slam_trainer.cpp:26-33): SLAMPipeline pipe; pipe.setTsdfEngine(createTsdfEngine(
    // reader, config)); ... pipe.SLAMTrainCams(model, cams).  Frames then come from the CLIEngine's host-resident sequence
    // (per-frame upload inside the loop) instead of device tensors handed to processFrame.
    explicit SLAMPipeline(uint64_t seed = 1234);
    void setTsdfEngine(InfiniTAM::Engine::CLIEngine* tsdf_engine);  // slam_pipeline.h:22-29
    void detachTsdfEngine();   // flush + drop the pointers into the engine (CLIEngine::Shutdown calls it through beforeShutdown)
    void SLAMTrainCams(SLAMGaussianModel& model, std::vector<Camera>& cams);  // slam_pipeline.cpp:52-173
    void processFrame(int i, Camera& cam);  // one iteration of that loop: tsdf_engine->ProcessFrame() + the Gaussian block

    void loadConfig(const gpsh::Config& config);  // PIPELINE section keys
    // The reference's signature (slam_pipeline.cpp:175-193 + Pipeline::loadConfig, src/pipeline.cpp:5-36; N = YAML::Node or
    // gpsh::Node): the PIPE node with its nested weight_configs / vis_configs / keyframe_sample_configs / remove_configs / TSDF.
    // The output paths are workspace_dir + the file's strings, as the reference concatenates them; is_train creates the
    // directories the reference creates (each one emptied first, like its createDirectory(path, true); no TensorBoard logger).
    // enable_densify: true throws -- densification is out of scope.  One list of keys: configFields.
    template <class N> void loadConfig(const N& pipe_node, const std::string& workspace_dir, bool is_train);
    template <class V> void configFields(V& v);
    // the two halves of the node route: node -> flat Config (every conversion and check, nothing assigned), and the assignment
    template <class N> gpsh::Config flattenConfig(const N& pipe_node);
    void applyConfig(const gpsh::Config& flat, bool from_node);
    void createOutputDirs();   // what loadConfig(node, dir, true) creates

    // Pipeline::save (src/pipeline.cpp:38-54): nothing for an empty model; else model_path/cfg_args, point_cloud/point_cloud.ply,
    // model.pt and cameras.json (session.hpp: writeCfgArgs, writeCamerasJson) -- a directory 3DGS viewers load.  Returns the files.
    std::vector<std::string> save(SLAMGaussianModel& model, const std::vector<Camera>& cams);
    // DatasetReader::savePose (dataset_reader.cpp:405-418): one frame<id>.txt per camera with its c2w_slam (writePoseTxt)
    std::vector<std::string> savePoses(const std::string& dir, const std::vector<Camera>& cams);

    // body of the SLAMTrainCams frame loop (:69-132) for frame i
    void processFrame(int i, Camera& cam, const torch::Tensor& rgb_u8, const torch::Tensor& depth_mm_i16);
    void SLAMTrainCams(std::vector<Camera>& cams, const std::vector<torch::Tensor>& rgb_u8,
                       const std::vector<torch::Tensor>& depth_mm_i16);

    TensorDict runRaycastByCam(const Camera& cam, bool use_cam_depth = true);  // :362-415
    void updateFrameList();                                                    // :319-360
    void localFrameRaycast();
    void keyFrameRaycast();
    void initNewGaussians(TensorDict& raycast_maps);
    void localOptimize();
    void removeRedundantGs();

    // renderEvalImgs (slam_pipeline.cpp:588-695), the compute half: for every camera the free-view raycast with the stored pose
    // and, if the model is not empty, forward() under NoGradGuard.  Returns per camera the tensors the reference turns into
    // image files with OpenCV ("raycast_color", "raycast_depth" and, per requested name, "rgb" clamped to [0,1], "alpha",
    // "depth") plus "psnr" -- and the same images AS THE REFERENCE QUANTISES THEM for its files: "rgb_u8", "gt_u8",
    // "raycast_color_u8" ((t * 255.0).toType(kU8), cv_utils.cpp:57-76), "raycast_depth_u16" (millimetres, cv_utils.cpp:79-101)
    // and "psnr_u8" = scripts/metric.py's PSNR of the 8-bit render against the 8-bit ground truth.  The JPEG / PNG encoders
    // themselves are I/O outside this library.
    std::vector<TensorDict> renderEvalImgs(const std::vector<Camera>& cams, const std::vector<std::string>& names = {"rgb"});

    // The reference's image-quality numbers for those views (scripts/metric.py, run/eval.py; with depth_mask its masked variant
    // scripts/metric_general.py): flush(), every camera rendered exactly as renderEvalImgs renders it, "rgb_u8" and "gt_u8" stacked
    // and ONE imageMetrics call (image_eval.hpp) -> per-view PSNR and SSIM and their means, the content of results.json /
    // per_view.json as data (file writing and the JPEG encoder stay outside).  source "raycast_color" compares "raycast_color_u8"
    // instead: the TSDF-colour baseline (the comparison left commented out in metric.py:15).  depth_mask multiplies both images by
    // cam.depth > 0 and needs has_depth on every camera.  A camera without an image, an unknown source, or source "rgb" on an
    // empty model throw.
    ImageEvalResult evalImages(const std::vector<Camera>& cams, bool depth_mask = false, const std::string& source = "rgb");

    // Pipeline::gesTrainCams (src/pipeline.cpp:229-319): the pass over ALL of `cams` once the sequence is over -- ONE
    // initOptimizers(max_iterations, scene_scale) whose state lives for the whole call, the means' rate decaying to 0.01 x its
    // start, the SH degree growing by MODEL.sh_degree_interval.  Per iteration: the camera from a gpsh::RandomSelector seeded with
    // `seed` (or cams[selected_cam_idx]), drawn one iteration early so that the step can run the next camera's preprocessing
    // ahead; updateSH(curr_iter); the iteration body of localOptimize (optimizeOne: same routes for exposure rows and loss
    // weights); schedulersStep().  No prune, no new Gaussians.  flush() first; the engine's volume is read, never modified.
    // Base layers: the reference reads pre-rendered mesh images (mesh_rgb_path / mesh_depth_path); here each camera's come from
    // the attached engine's FINAL volume -- runRaycastByCam(cam, false)'s maps, batched, kept on the device (colour, depth,
    // clamped depth) -- or, second overload, from the caller as one {"depth_map", "color_map"} pair per camera (the reference's
    // file route; reading files stays outside).  If those layers plus the cameras' device images exceed refine_cache_mb the call
    // throws before anything is allocated.  curr_iter is a member, as in the reference: a second call continues (and returns at
    // once when curr_iter >= max_iterations).  Every log_iter iterations and at the last one lossSum() is read into refine_log
    // and checkBinningCapacity() runs: the loop's only host synchronisations.  max_iterations < 0: this->max_iterations;
    // seed < 0: refine_seed.  Returns the number of iterations run.
    int gesTrainCams(const std::vector<Camera>& cams, int max_iterations = -1, int64_t seed = -1);
    int gesTrainCams(const std::vector<Camera>& cams, const std::vector<TensorDict>& base_layers, int max_iterations = -1, int64_t seed = -1);
    int64_t refineCacheBytes(const std::vector<Camera>& cams) const;   // what gesTrainCams holds on the device for these cameras
    // Pipeline::rawTrainCams (src/pipeline.cpp:155-226), the classic 3DGS trainer over posed images: no TSDF layer, no engine.
    // render_method must be "raw".  ONE initOptimizers(max_iterations, scene_scale); per iteration the camera from the seeded
    // RandomSelector (or cams[selected_cam_idx]), updateSH, forward, computeLoss, backward, optimizersStep, optimizersZeroGrad,
    // with `densify` retain_grad() on means2d and stepPostBackward (RawGaussianModel: clone / split / prune / opacity reset, its
    // split samples from a generator of the same seed), schedulersStep.  The loss is read every log_iter iterations and at the
    // last one into refine_log.  The reference's switch is PIPE.enable_densify, which the SLAM configuration refuses: here it is
    // the argument.  curr_iter, max_iterations < 0, seed < 0: as gesTrainCams.  Returns the number of iterations run.
    int rawTrainCams(const std::vector<Camera>& cams, int max_iterations = -1, int64_t seed = -1, bool densify = false);
    int trainCams(const std::vector<Camera>& cams, const std::string& mode);   // "raw" | "ges" (src/pipeline.cpp trainCams)
    int curr_iter = 0;
    struct RefineLogEntry { int iter; float loss; };
    std::vector<RefineLogEntry> refine_log;
    // PIPE keys of this project (all optional): what runSession does between SLAMTrainCams and save
    int refine_iterations = 0;               // 0: no refinement
    std::string refine_cams = "keyframes";   // "keyframes": keyframe_cam_list + the live window; "all": every train camera
    int64_t refine_seed = 1234;              // (the constructor's seed unless the key is given)
    int64_t refine_cache_mb = 16384;
    bool refine_lr_decay = true;             // (no key) false: gesTrainCams builds its optimisers without the scheduler -- constant rates
    std::vector<Camera> refineKeyframeCams() const;   // the "keyframes" set (a window camera that is a keyframe too counts once)

    // slam_pipeline.h:32-49: mesh / engine state files under workspace_dir (empty names are skipped like the reference)
    std::string workspace_dir = ".", saved_mesh, saved_engine;
    void saveMesh() { if (!saved_mesh.empty()) main_engine->SaveSceneToMesh((workspace_dir + "/" + saved_mesh).c_str()); }
    void saveEngine() { if (!saved_engine.empty()) main_engine->SaveToFile(workspace_dir + "/" + saved_engine); }
    void loadEngine() { main_engine->LoadFromFile(workspace_dir + "/" + saved_engine); }

    // The reference's other two result numbers (scripts/geo_general.py, scripts/ate_general.py) on the run so far; both flush()
    // first and need an attached engine.  evalGeometry: TsdfEngine::EvalMesh.  evalTrajectory: ate() of the engine's stored
    // per-frame poses (camPoses) against gtC2wPoses; mismatched lengths or fewer than three frames throw.
    GeomEvalResult evalGeometry(const torch::Tensor& gt_points_or_triangles, const torch::Tensor& transform = torch::Tensor(),
                                const std::vector<double>& dist_thres = {0.03}, int64_t sample_nums = 1000000, uint64_t seed = 0);
    AteResult evalTrajectory();

    // Pipeline::loadConfig's session settings (src/pipeline.cpp:9-22).  The *_cfg strings are the file's ("/gs_model", "/log", "/val");
    // model_path / log_path / eval_path = workspace_dir + them.  max_iterations, selected_cam_idx and log_iter are gesTrainCams';
    // log_slam_state and enable_densify are stored only.
    bool eval_after_train = false, save_after_train = false, enable_densify = false, log_slam_state = false;
    int max_iterations = 10000, selected_cam_idx = -1, log_iter = 1000;
    std::string model_path_cfg = "/gs_model", log_path_cfg = "/log", eval_path_cfg = "/val";
    std::string model_path, log_path, eval_path, saved_images;
    float color_error_max = 0.1f, depth_error_max = 0.1f;   // vis_configs of the reference's image logging (stored only)
    void updatePaths() {
        model_path = workspace_dir + model_path_cfg; log_path = workspace_dir + log_path_cfg; eval_path = workspace_dir + eval_path_cfg;
    }

    torch::Device device = torch::kCUDA;
    std::string work_mode = "train";
    InfiniTAM::Engine::CLIEngine* tsdf_engine = nullptr;
    TsdfEngine* main_engine = nullptr;
    SLAMGaussianModel* model = nullptr;
    float voxel_size;

    int curr_frame_id = -1;
    int localframe_cam_window_length = 2, localframe_cam_window_interval = 5;
    int local_opt_iters = 20, local_opt_interval = 10;
    int keyframe_select_max = 7;
    Camera curr_cam;
    std::deque<Camera> localframe_cam_window;
    std::deque<TensorDict> localframe_raycast_window;
    std::vector<Camera> keyframe_cam_list;
    float keyframe_theta_thres = 30.0f, keyframe_trans_thres = 0.3f;
    // keyframe_sample_configs (slam_pipeline.cpp:130, 293-317, 538): "random" draws keyframe_select_max history keyframes per update;
    // "ours" -- as the reference ships it -- adds NO history views (keyFrameRaycast has a "random" branch only) and keeps a loss
    // record per keyframe: {loss, frame id of the check, mean raycast confidence, number of checks with loss > loss_thres}
    std::string sample_method = "random";
    float loss_thres = 0.0f;
    std::map<int, std::vector<float>> keyframe_loss_dict;
    void checkKeyFrameError();
    float new_gs_sample_ratio = 0.25f, color_error_thres = 0.05f;
    float depth_vis_max = 5.0f, depth_vis_min = 0.0f, alpha_vis_max = 5.0f;
    float large_scale_thres = 0.1f, small_scale_thres = 0.003f, low_opac_thres = 0.005f;
    float scene_scale = 1.1f * 3.0f;
    float ssim_weight = 0.0f, depth_weight = 0.0f;  // both 0 in every shipped config -> the fused L1 trainStep
    // a non-zero weight: false (default) -> the reference's sequence through autograd (forward, computeLoss, backward,
    // optimizersStep); true -> trainStep with the weights (gps_splat_step::ssim_weight ..: one C-ABI call, next_cam prefetch
    // allowed) for every camera without an exposure row
    bool fused_loss_terms = false;
    int64_t autograd_iters = 0;   // optimise iterations that went through the autograd route (forward -> computeLoss -> backward)

    // LOG_PIPELINE_TIME of the reference (slam_pipeline.cpp:54-67, 73-96, 141-167): host wall-clock totals of one SLAMTrainCams run in
    // milliseconds.  `per_frame` is the reference's "per frame fusion time" (ProcessFrame + pose + toGPU + updateFrameList); FPS =
    // frames / (slam_total / 1000); run/read_results.py:38-39 derives Fusion-FPS = 1000 / per_frame and Gaussian-FPS =
    // 1000 / (1000 / FPS - per_frame) from them.  slam_total here ends AFTER flush() and a device synchronise (the reference stops
    // its clock with kernels still in flight).  The per-stage totals are HOST time of the thread that runs the stage, comparable with
    // the reference's in the sequential schedule only.  Under overlap: streams-only books none of them (its host share of the frame
    // thread is `keyframe_step`); with the mapping thread localFrameRaycast / keyFrameRaycast are the ENQUEUE time of whoever builds
    // the views (frame thread with pipeline_raycasts, else the worker; one batch: all under localFrameRaycast), the other stages are
    // the worker's, and localOptimize includes its wait for the map stream.  per_frame, slam_total and gpu_memory_mb always mean
    // what the reference's mean.
    struct PipelineTimes {
        int frames = 0;
        double slam_total = 0, per_frame = 0, keyframe_step = 0, localFrameRaycast = 0, keyFrameRaycast = 0, initNewGaussians = 0,
               localOptimize = 0, removeGaussian = 0, checkError = 0;
        long long gpu_memory_mb = -1;    // getGPUMemoryUsage after emptyCache() at the end of the run (slam_pipeline.cpp:168-171)
        double max_frame_after_30 = 0;   // slowest processFrame call (host wall) from frame 30 on
        int max_frame_id = -1;
        double fps() const { return slam_total > 0 ? frames / (slam_total / 1000.0) : 0.0; }
        double fusion_fps() const { return per_frame > 0 ? 1000.0 / (per_frame / frames) : 0.0; }
        double gaussian_fps() const {
            const double rest = slam_total > 0 && frames > 0 ? (slam_total - per_frame) / frames : 0.0;
            return rest > 0 ? 1000.0 / rest : 0.0;
        }
    } times;
    bool log_pipeline_time = false;        // print the reference's "[PIPELINE AVG TIME]" line at the end of SLAMTrainCams
    double frame_report_ms = -1.0;         // debug aid: a processFrame call that took longer than this many ms of host time prints where it went
    std::vector<float> frame_ms;           // host wall of every processFrame call of the last SLAMTrainCams (filled when keep_frame_ms)
    std::vector<float> frame_wait_ms;      // ... of which: waiting for the map worker (previous update's completion / this update's raycasts)
    bool keep_frame_ms = false;

    // counters are bumped by the frame thread AND (mapping_thread) by the map worker: atomics
    struct Stats { std::atomic<int64_t> frames{0}, opt_iters{0}, raycasts{0}, added{0}, pruned{0}; } stats;

    // Tracking / mapping overlap.  The reference runs a keyframe's map update (raycasts, new Gaussians, 20 optimise iterations,
    // prune) to completion before it looks at the next frame.  Nothing in frames i+1 .. i+9 reads the Gaussian model, and the
    // model update reads the TSDF volume only through the free-view raycasts at its start -- so with overlap_mapping the
    // update runs on a second HIP stream while a high-priority stream tracks and fuses the following frames (the latency-bound
    // LM loop of the tracker fits into the shadow of the throughput-bound rasterizer kernels).  Ordering is kept with events:
    // map stream waits for frame i's fusion; frame i+1 may TRACK at once but waits for the raycasts before it fuses
    // (TsdfEngine::beforeNextFusion); the next keyframe waits for the previous update; without a mapping thread the prune
    // of update k runs at the start of update k+1 (or in flush()).
    // Results are those of the sequential schedule.  Off by default: with it on, processFrame() returns while the update is
    // still in flight and the model may only be read after flush() (SLAMTrainCams and the accessors below call it).
    bool overlap_mapping = false;
    // overlapped arrangements: the window's and the keyframes' free views of an update as ONE batch (the next frame's fusion waits
    // for all of them anyway: 0.68 instead of 0.23 + 0.54 ms) or as two (initNewGaussians then starts after the window's views
    // alone).  Measured: one batch is + 1 % on some boxes of the pool and - 5 % on others at 640x480 (the map update and the ten
    // frames it runs beside are equally long there, so which of the two waits for the other flips) and - 6 % at 1280x720: two.
    bool merge_keyframe_raycasts = false;
    bool views_reserved_ = false, raycast_pool_warm_ = false;
    bool async_raycasts = true;   // the update's free-view raycasts run beside its optimise iterations (same results)
    // which stream each chain gets (slam_pipeline.cpp: make_stream): 0 / 1 = torch's high- / normal-priority pool, 2 / 3 / 4 = a
    // stream of the pipeline's own at the lowest / highest / default priority
    // Round 5: ALL THREE are streams of the library's own now (one per priority for the life of the process: make_stream).  torch hands
    // its pool streams out round-robin and never destroys them, ROCm spreads the streams of one priority level over <= 4 hardware
    // queues by reference count -- so which chains ended up sharing a queue depended on how many scenes the PROCESS had built
    // before: the same 1,000-frame run gave 1,120 frames/s in a fresh process and 900 after six other scenes, a test process's
    // tenth scene ran its frames and its map update on ONE queue (540 instead of 850 frames/s, every period's fifth frame 6 ms
    // late); with own streams every measurement is history-free (bench.py: cfg1 1,070 -> 1,640 and cfgR 710 -> 820 frames/s when
    // they run after the whole-sequence leg).
    int frame_stream_kind = 3, map_stream_kind = 4, raycast_stream_kind = 2;
    // an optimise iteration's backward + Adam kernel also runs the NEXT iteration's preprocessing forward (the next camera is drawn
    // one iteration early: same draws, same order): one launch and one pass over the parameters less per iteration, same results
    bool prefetch_next_preprocess = true;
    // what gps_set_frame_chain_reserve gets while the schedules overlap (1: the strip backward leaves register room for a tracker wave
    // and the forward launches row-major; 0: off; other bits: experiment switches of the kernel library)
    int frame_chain_reserve = 1;
    // with mapping_thread + async_raycasts: the free views of update k + 1 are enqueued by the FRAME thread the moment keyframe k + 1 is
    // fused, whether or not the worker has finished update k (they read the volume, not the model; their results go into the job the
    // worker adopts when it gets there).  Before, the worker raycast at the start of its job: 0.6-0.8 ms at the head of a chain that
    // carries the period once the update is longer than its ten frames, and the next frame's fusion waited for the worker to get that far.
    bool pipeline_raycasts = true;
    // with overlap_mapping: run the map update on a worker thread of its own (tracking thread + mapping thread) instead of
    // interleaving its host work with the frames on the caller's thread
    bool mapping_thread = false;
    int pump_iters_first = 4, pump_iters_per_frame = 3;  // optimise iterations enqueued at the keyframe / per following frame
    void flush();
    // Test hook: with trace_frames every frame leaves, ENQUEUED on the stream the frame ran on (no host synchronisation, so the
    // schedule under test is undisturbed), a copy of the live raycast image and of the engine's counters, plus the pose the
    // frame was fused with (host values).  Read them after flush().
    bool trace_frames = false;
    std::vector<torch::Tensor> trace_live, trace_counters, trace_poses;
    ~SLAMPipeline();

    // One map update's view set: the cameras it optimises over (the local window first, then the history keyframes), each camera's
    // free-view raycast and the event behind that result (nullptr: the result is ordered by the stream itself).
    struct UpdateViews {
        std::vector<Camera> cams;
        std::vector<TensorDict> raycasts;
        std::vector<RaycastEvent> events;    // parallel to raycasts for the views the builder made; a view appended by hand has none
        size_t window_len = 0;               // length of the local window at the front (what checkKeyFrameError skips)
        int frame_id = 0;                    // frame number of the update the set belongs to (what checkKeyFrameError stamps with)
        RaycastEvent last_event = nullptr;   // the last batch's: one raycast stream, so it covers every result of the set
        RaycastEvent eventOf(size_t k) const { return k < events.size() ? events[k] : nullptr; }
    };

private:
    UpdateViews views_;   // the current update's

public:
    // slam_pipeline.h names of the current set (the drop-in surface): the same storage
    std::vector<Camera>& opt_cam_list = views_.cams;
    std::vector<TensorDict>& opt_raycast_list = views_.raycasts;

private:
    struct Streams;         // map + frame stream and the fixed events between them (defined in the .cpp: no HIP / c10 stream headers here)
    struct RaycastStream;   // the free views' stream, its "volume complete" event and the pooled per-batch events
    std::unique_ptr<Streams> streams_;      // created by the first overlapped frame
    std::unique_ptr<RaycastStream> rc_;     // created by the first asynchronous raycast
    void ensureStreams();
    RaycastStream& raycastStream();
    void requireEngine(const char* who) const;   // TORCH_CHECK: an engine is attached (not shut down / detached)

    void processFrameImpl(int i, Camera& cam, const torch::Tensor& rgb_u8, const torch::Tensor& depth_mm_i16);
    // one camera's free view on the current stream, un-batched (runRaycastByCam, renderEvalImgs)
    TensorDict raycastCam(const Camera& cam, const std::vector<ORUtils::SE3Pose>& poses);
    // one camera of renderEvalImgs / evalImages (the caller holds the NoGradGuard and has flushed)
    TensorDict renderEvalCam(const Camera& cam, const std::vector<std::string>& names);
    // the same for several cameras of one volume state in ONE batched free-view chain.  ev_out != nullptr: on the raycast stream, and
    // *ev_out is the one event behind all results (use_event: record THIS event instead of one of the update's pooled events)
    std::vector<TensorDict> raycastCams(const std::vector<const Camera*>& cams, const std::vector<ORUtils::SE3Pose>& poses,
                                        RaycastEvent* ev_out = nullptr, RaycastEvent use_event = nullptr);
    // where a view set is built from: the live lists (sequential / streams-only schedule, the frame thread's enqueue) or a job's
    // snapshot of them (the worker raycasts itself while the frame thread keeps appending to the originals)
    struct ViewSource {
        const std::deque<Camera>& window; const std::vector<Camera>& keyframes; const std::vector<ORUtils::SE3Pose>& poses; int frame_id;
    };
    ViewSource liveSource() const { return {localframe_cam_window, keyframe_cam_list, main_engine->camPoses, curr_frame_id}; }
    enum ViewParts { kWindowBatch = 1, kKeyframeBatch = 2, kTwoBatches = 3, kOneBatch = 7 };   // kOneBatch: window + keyframes share the launches
    struct RaycastMs { double window = 0, keyframes = 0; };   // host time of the two steps (one batch: all under `window`)
    // THE builder of a view set (see the .cpp for the rule the schedules' bit-equality rests on).  job_events: the {window, keyframe}
    // events of a job the frame thread enqueues; nullptr: pooled events (async_raycasts) or none
    RaycastMs buildViews(UpdateViews& out, const ViewSource& src, int parts, const RaycastEvent* job_events = nullptr);
    RaycastMs buildCurrentViews(const ViewSource& src, int parts);   // ... into views_ (+ localframe_raycast_window)
    void adoptViews(UpdateViews&& v);
    void bookRaycastMs(const RaycastMs& ms) { times.localFrameRaycast += ms.window; times.keyFrameRaycast += ms.keyframes; }

    void initNewGaussiansFor(TensorDict& raycast_maps, const Camera& cam);
    // The pieces of one update.  runUpdate is the whole stage sequence with the stage timers (sequential schedule, map worker); the
    // streams-only schedule opens an update with beginUpdate, pumps the iterations from later frames and defers finishUpdate.
    double beginUpdate(const Camera& cam);   // initNewGaussians + localOptimizeBegin; returns the host time between the two
    void finishUpdate();                     // prune + ("ours") loss records
    void runUpdate(const Camera& cam);
    void finishDeferredUpdate();             // streams-only: update k's finishUpdate, on the map stream, if it is still owed
    void keyframeStep();
    void keyframeStepOverlapped();
    void keyframeStepThreaded();
    void mapWorker(int device_index);
    void rethrowWorkerError();
    struct MapJob {
        Camera curr_cam;
        // pipeline_raycasts: the update's views, already enqueued by the frame thread (the worker adopts them instead of raycasting)
        bool views_ready = false;
        UpdateViews views;
        // otherwise: what the worker builds them from
        std::deque<Camera> window; std::vector<Camera> keyframes; std::vector<ORUtils::SE3Pose> poses; int frame_id = 0;
    };
    MapJob job_;
    // The threaded hand-over: start the worker if needed, wait until the previous update is done or has failed, rethrow its error,
    // let `fill` write job_, wake the worker.  waitWorkerIdle is the wait alone (flush()).
    template <class Fill> void postJob(Fill&& fill);
    void waitWorkerIdle(std::unique_lock<std::mutex>& lk);
    int job_parity_ = 0;                          // which of Streams::job's two event pairs the next enqueued job gets
    std::mt19937_64 rng_kf_;                      // the history keyframes' draw (its own generator: the frame thread draws while the worker's update draws cameras)
    std::mutex loss_mu_;                         // keyframe_loss_dict: written by updateFrameList (frame thread) and checkKeyFrameError (map thread)
    std::thread worker_;
    std::mutex mu_;
    std::condition_variable cv_;
    int64_t job_seq_ = 0, raycasts_seq_ = 0, done_seq_ = 0;
    bool stop_ = false;
    std::exception_ptr worker_error_;
    // host time the frame thread spent WAITING for the map worker inside the last processFrame call: for the previous update to finish
    // (hand-over at a keyframe) and for this update's raycasts to be enqueued (gate of the next frame's fusion)
    double gate_wait_ms_ = 0.0, handover_wait_ms_ = 0.0;
    std::atomic<double> job_post_ms_{0.0};        // (debug aid only: when the frame thread woke the mapping thread)
    void localOptimizeBegin();
    void optimizeIterations(int count);
    // One optimise iteration on `cam` over its base layers `rc` (depth_map, color_map, depth_map_clamped; ev: the event behind
    // them or nullptr): the fused trainStep, with the loss weights inside it (fused_loss_terms), or the reference's sequence
    // through autograd.  THE iteration body of localOptimize and of gesTrainCams.  next_cam: see RawGaussianModel::trainStep;
    // pass one only where canRunAhead().
    void optimizeOne(const Camera& cam, TensorDict& rc, RaycastEvent ev, const Camera* next_cam);
    int refineLoop(const std::vector<Camera>& cams, std::vector<TensorDict>& layers, int max_iterations, int64_t seed);   // gesTrainCams behind its base layers
    bool canRunAhead() const {
        const bool terms = ssim_weight > 0 || depth_weight > 0;
        return prefetch_next_preprocess && (!terms || fused_loss_terms);
    }
    void pumpMapping(int count);
    std::unique_ptr<RandomSelector<Camera>> opt_loader_;
    std::pair<int, const Camera*> opt_peek_{0, nullptr};   // the next iteration's camera, drawn one iteration early (optimizeIterations)
    bool opt_peek_valid_ = false;
    int opt_pending_ = 0;
    bool map_update_open_ = false;
    std::mt19937_64 rng_;
    at::Generator gen_;
    // A keyframe's free-view raycasts on a stream of their own, next to the optimise iterations (they only read the volume; the
    // rasterizer kernels fill the GPU their latency-bound tails leave idle): every result carries an event, and whoever reads
    // a result (initNewGaussians, an optimise iteration) makes its stream wait for it.
    void beginAsyncRaycasts();                    // call once per update, on the stream that is ordered after the volume
    void waitRaycast(RaycastEvent ev);            // current stream waits for one result (no-op for nullptr)
    void waitAllRaycasts() { waitRaycast(views_.last_event); }   // ... for all of the current update's
    bool map_in_flight_ = false, prune_pending_ = false;
};

// THE list of PIPE keys (slam_pipeline.cpp:175-193, src/pipeline.cpp:5-36 and the nested sections the reference reads where it uses
// them: :130, :308, :420-459, :538, :568-570, slam_pipeline.h:32-49), for every route (config_fields.hpp)
template <class V>
void SLAMPipeline::configFields(V& v) {
    v.i("max_iterations", max_iterations);
    v.i("selected_cam_idx", selected_cam_idx);
    v.b("enable_densify", enable_densify);
    v.b("eval_after_train", eval_after_train);
    v.b("save_after_train", save_after_train);
    v.i("log_iter", log_iter);
    v.s("model_path", model_path_cfg);
    v.s("log_path", log_path_cfg);
    v.s("eval_path", eval_path_cfg);
    v.f("new_gs_sample_ratio", new_gs_sample_ratio);
    v.i("keyframe_select_max", keyframe_select_max);
    v.i("localframe_cam_window_length", localframe_cam_window_length);
    v.i("localframe_cam_window_interval", localframe_cam_window_interval);
    v.i("local_opt_iters", local_opt_iters);
    v.i("local_opt_interval", local_opt_interval);
    v.f("color_error_thres", color_error_thres);
    v.f("keyframe_theta_thres", keyframe_theta_thres);
    v.f("keyframe_trans_thres", keyframe_trans_thres);
    v.b("log_slam_state", log_slam_state);
    {
        auto w = v.section("weight_configs");   // LOSS weights (office0.yaml:37-39)
        RawGaussianModel::lossWeightFields(w, ssim_weight, depth_weight);
    }
    {
        auto s = v.section("vis_configs");
        s.f("color_error_max", color_error_max);
        s.f("depth_error_max", depth_error_max);
        s.f("depth_vis_max", depth_vis_max);
        s.f("depth_vis_min", depth_vis_min);
        s.f("alpha_vis_max", alpha_vis_max);
    }
    {
        auto s = v.section("keyframe_sample_configs");
        s.s("sample_method", sample_method);
        s.f("loss_thres", loss_thres);
        s.ignored("weight_intervel");   // (in every shipped file, read by nothing)
        s.ignored("opt_thres");
    }
    {
        auto s = v.section("remove_configs");
        s.f("large_scale_thres", large_scale_thres);
        s.f("small_scale_thres", small_scale_thres);
        s.f("low_opac_thres", low_opac_thres);
    }
    {
        auto s = v.section("TSDF");
        s.s("saved_mesh", saved_mesh);
        s.s("saved_engine", saved_engine);
        s.s("saved_images", saved_images);
        for (const char* k : {"voxel_size", "trunc_dist", "viewFrustum_min", "viewFrustum_max", "load_images", "use_gt_pose",
                              "sdf_local_block_num", "sdf_bucket_num", "sdf_excess_list_size", "failure_mode",
                              "use_approximate_raycast", "use_bilateral_filter"})
            s.ignored(k);   // (createTsdfEngine's: TsdfConfig)
    }
    v.ignored("train_mode");     // (one of the two is in every shipped file; the render method is MODEL.render_method)
    v.ignored("train_method");
    // this project's.  The schedule switches are read from a node alone: the flat route never read them and still does not.
    // (The flat route does accept the session keys above -- model_path, eval_after_train, saved_mesh ... -- which it had no field
    // for before.)
    v.b("fused_loss_terms", fused_loss_terms, gpsh::kOptional);
    v.i("refine_iterations", refine_iterations, gpsh::kOptional);
    v.s("refine_cams", refine_cams, gpsh::kOptional);
    v.i64("refine_seed", refine_seed, gpsh::kOptional);
    v.i64("refine_cache_mb", refine_cache_mb, gpsh::kOptional);
    v.b("overlap_mapping", overlap_mapping, gpsh::kNodeOnly);
    v.b("mapping_thread", mapping_thread, gpsh::kNodeOnly);
    v.b("async_raycasts", async_raycasts, gpsh::kNodeOnly);
    v.b("pipeline_raycasts", pipeline_raycasts, gpsh::kNodeOnly);
    v.b("merge_keyframe_raycasts", merge_keyframe_raycasts, gpsh::kNodeOnly);
    v.b("prefetch_next_preprocess", prefetch_next_preprocess, gpsh::kNodeOnly);
    v.b("log_pipeline_time", log_pipeline_time, gpsh::kNodeOnly);
    // the flat route alone: what the nested files keep outside PIPE (READER.scene_scale x 1.1, the root's work_mode)
    v.f("scene_scale", scene_scale, gpsh::kFlatOnly);
    v.s("work_mode", work_mode, gpsh::kFlatOnly);
}

template <class N>
gpsh::Config SLAMPipeline::flattenConfig(const N& pipe_node) {
    gpsh::Config flat = gpsh::flattenNode(pipe_node, "PIPE", [&](auto& v) { configFields(v); });
    if (flat.get("enable_densify", 0.0) != 0.0)
        throw gpsh::ConfigError(gpsh::nodePath(pipe_node, "PIPE") + ".enable_densify: densification is not supported (set it to false)");
    const std::string which = flat.gets("refine_cams", "keyframes");
    if (which != "keyframes" && which != "all")
        throw gpsh::ConfigError(gpsh::nodePath(pipe_node, "PIPE") + ".refine_cams: 'keyframes' or 'all', got '" + which + "'");
    if (flat.get("refine_iterations", 0.0) < 0.0)
        throw gpsh::ConfigError(gpsh::nodePath(pipe_node, "PIPE") + ".refine_iterations: must not be negative");
    return flat;
}

template <class N>
void SLAMPipeline::loadConfig(const N& pipe_node, const std::string& workspace_dir_, bool is_train) {
    const gpsh::Config flat = flattenConfig(pipe_node);
    workspace_dir = workspace_dir_;
    applyConfig(flat, true);
    if (is_train) createOutputDirs();
}
