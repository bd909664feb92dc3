#include "slam_pipeline.hpp"

#include <atomic>

#include <chrono>
#include <cstdlib>
#include <deque>

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>
#include <hip/hip_runtime_api.h>

#include <cmath>

using namespace gpsh;

namespace {
inline void hip_ok(hipError_t e, const char* what) { TORCH_CHECK(e == hipSuccess, what, ": ", hipGetErrorString(e)); }
// an event that orders streams (no timing), owned
struct Event {
    hipEvent_t ev = nullptr;
    Event() { hip_ok(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate"); }
    ~Event() { (void)hipEventDestroy(ev); }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    operator hipEvent_t() const { return ev; }
};
// kind 0 / 1: torch's high- / normal-priority pool; 2 / 3 / 4: a stream of this library's own (hipStreamCreateWithPriority,
// non-blocking) at the lowest / highest / default priority, wrapped for the stream guards.  ONE stream per (device, kind) for the
// life of the process, shared by every pipeline: ROCm places a new stream on a hardware queue by what exists at that moment, and
// creating a stream costs ~10 ms of a blocked runtime -- creating the three once keeps the placement the same for every scene of
// a process and the cost out of all but the first.  Two pipelines alive at once share the streams: ordered, just not concurrent
// with each other.  (The 90 ms / 2.1 s holes in the first frames of round 5's early whole-sequence runs, first blamed on queue
// creation, were the container's CPU quota: LABBOOK section 14, dist_util.cap_host_threads.)
c10::hip::HIPStream make_stream(int kind) {
    const auto dev = c10::hip::current_device();
    if (kind == 0) return c10::hip::getStreamFromPool(/*isHighPriority=*/true, dev);
    if (kind == 1) return c10::hip::getStreamFromPool(/*isHighPriority=*/false, dev);
    static std::mutex mu;
    static std::map<std::pair<int, int>, hipStream_t> own;
    std::lock_guard<std::mutex> lock(mu);
    auto it = own.find({(int)dev, kind});
    if (it == own.end()) {
        int least = 0, greatest = 0;
        hip_ok(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
        hipStream_t st = nullptr;
        hip_ok(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, kind == 2 ? least : kind == 3 ? greatest : 0), "hipStreamCreateWithPriority");
        // first use now, not in somebody's frame: the queue behind the stream exists when this returns
        void* word = nullptr;
        hip_ok(hipMalloc(&word, 256), "hipMalloc");
        hip_ok(hipMemsetAsync(word, 0, 256, st), "hipMemsetAsync");
        hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
        (void)hipFree(word);
        it = own.emplace(std::make_pair((int)dev, kind), st).first;
    }
    return c10::hip::getStreamFromExternal(it->second, dev);
}
}  // namespace
using torch::indexing::Slice;

// The overlapped schedules' streams (see make_stream: handles on the process-wide streams) and the fixed events between them.
struct SLAMPipeline::Streams {
    c10::hip::HIPStream map, frame;
    Event frame_fused;   // "frame i is fused": what an update's raycasts wait for
    Event raycasts;      // "the update's raycasts have read the volume": the gate of the next frame's fusion
    Event map_done;      // streams-only schedule: the update's last iteration
    Event caller;        // the caller's stream at processFrame (inputs)
    Event job[2][2];     // {window batch, keyframe batch} per update parity, for the views the frame thread enqueues
    Streams(int map_kind, int frame_kind) : map(make_stream(map_kind)), frame(make_stream(frame_kind)) {}
    ~Streams() { (void)hipStreamSynchronize(map.stream()); (void)hipStreamSynchronize(frame.stream()); }
};

struct SLAMPipeline::RaycastStream {
    c10::hip::HIPStream s;
    Event begin;                // "the volume the raycasts read is complete" (recorded on the issuing stream)
    std::deque<Event> pool;     // one per raycast batch of the current update, reused by the next
    size_t next = 0;
    explicit RaycastStream(int kind) : s(make_stream(kind)) {}
    ~RaycastStream() { (void)hipStreamSynchronize(s.stream()); }
    hipEvent_t nextEvent() {
        if (next == pool.size()) pool.emplace_back();
        return pool[next++];
    }
};

unsigned long long getGPUMemoryUsage(int gpu_id) {
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess) return ~0ull;
    size_t free_b = 0, total_b = 0;
    const bool ok = hipSetDevice(gpu_id) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    (void)hipSetDevice(prev);
    return ok ? (unsigned long long)((total_b - free_b) / (1024 * 1024)) : ~0ull;
}

torch::Tensor computeNormalMap(const torch::Tensor& vertex_map_in) {
    auto vertex_map = vertex_map_in.contiguous();
    check_f32_dev(vertex_map, "vertex_map");
    const int H = (int)vertex_map.size(0), W = (int)vertex_map.size(1);
    auto out = torch::empty_like(vertex_map);
    check(gps_normal_map(W, H, fptr(vertex_map), fptr(out), current_stream()), "gps_normal_map");
    return out;
}

SLAMPipeline::SLAMPipeline(TsdfEngine* tsdf_engine, SLAMGaussianModel* model_, uint64_t seed, bool use_gt_pose)
    : main_engine(tsdf_engine), model(model_), rng_kf_(seed ^ 0x9E3779B97F4A7C15ull), rng_(seed), gen_(at::detail::createCPUGenerator(seed)) {
    refine_seed = (int64_t)(seed & 0x7fffffffffffffffull);
    if (use_gt_pose) main_engine->turnOffTracking();
    device = model->device;
    voxel_size = main_engine->getVoxelSize();
}

SLAMPipeline::SLAMPipeline(uint64_t seed) : rng_kf_(seed ^ 0x9E3779B97F4A7C15ull), rng_(seed), gen_(at::detail::createCPUGenerator(seed)) {
    refine_seed = (int64_t)(seed & 0x7fffffffffffffffull);
}

void SLAMPipeline::setTsdfEngine(InfiniTAM::Engine::CLIEngine* engine) {
    // an engine attached before must not call back into this pipeline (its Shutdown() would detach the new one)
    detachTsdfEngine();
    tsdf_engine = engine;
    auto* be = dynamic_cast<ITMLib::ITMBasicEngine<ITMVoxel, ITMVoxelIndex>*>(engine->getMainEngine());
    TORCH_CHECK(be != nullptr, "setTsdfEngine: the main engine must be an ITMBasicEngine<ITMVoxel, ITMVoxelIndex>");
    main_engine = be;
    voxel_size = be->getVoxelSize();
    // CLIEngine::Shutdown() frees the engine (ownsInputs): finish what is in flight and let go of it first
    engine->beforeShutdown = [this] { detachTsdfEngine(); };
}

void SLAMPipeline::detachTsdfEngine() {
    if (!tsdf_engine) return;
    try { flush(); } catch (...) {}   // (a worker error has been, or will be, reported by the call that hit it)
    (void)hipDeviceSynchronize();
    if (main_engine) main_engine->beforeNextFusion = nullptr;
    if (tsdf_engine->beforeShutdown) tsdf_engine->beforeShutdown = nullptr;
    main_engine = nullptr;
    tsdf_engine = nullptr;
}

void SLAMPipeline::requireEngine(const char* who) const {
    TORCH_CHECK(main_engine != nullptr, who, ": no TSDF engine is attached -- it was shut down (CLIEngine::Shutdown / detachTsdfEngine) or "
                "never set; attach one with setTsdfEngine()");
}

static inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// slam_pipeline.cpp:52-173 with its LOG_PIPELINE_TIME clock: `times` holds what the reference prints as "[PIPELINE AVG TIME]"
void SLAMPipeline::SLAMTrainCams(SLAMGaussianModel& model_, std::vector<Camera>& cams) {
    model = &model_;
    device = model->device;
    times = PipelineTimes();
    frame_ms.clear(); frame_wait_ms.clear();
    const double t0 = now_ms();
    for (size_t i = 0; i < cams.size(); i++) {
        const double tf = now_ms();
        processFrame((int)i, cams[i]);
        const double dt = now_ms() - tf;
        if (keep_frame_ms) { frame_ms.push_back((float)dt); frame_wait_ms.push_back((float)(gate_wait_ms_ + handover_wait_ms_)); }
        if (i >= 30 && dt > times.max_frame_after_30) { times.max_frame_after_30 = dt; times.max_frame_id = (int)i; }
    }
    flush();
    hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
    times.slam_total = now_ms() - t0;
    times.frames = (int)cams.size();
    if (times.frames == 0) return;   // (nothing to average: the reference would print NaN into time_log.txt)
    // slam_pipeline.cpp:168-171: emptyCache(), then the device memory in use (what run/read_results.py reads as "GPU memory usage")
    c10::hip::HIPCachingAllocator::emptyCache();
    times.gpu_memory_mb = (long long)getGPUMemoryUsage((int)c10::hip::current_device());
    if (!log_pipeline_time) return;
    char avg[512];
    snprintf(avg, sizeof avg, "[PIPELINE AVG TIME] GS num: %d, per frame fusion time: %f, localFrameRaycast time: %f, keyFrameRaycast time: %f, "
             "initNewGaussians time: %f, localOptimize time: %f, FPS: %f\n", model->getGaussianNum(), times.per_frame / times.frames,
             times.localFrameRaycast / times.frames, times.keyFrameRaycast / times.frames, times.initNewGaussians / times.frames,
             times.localOptimize / times.frames, times.fps());
    if (FILE* f = fopen((workspace_dir + "/time_log.txt").c_str(), "w")) {   // (the file run/read_results.py parses)
        fprintf(f, "%sGPU memory usage: %d MB\n", avg, (int)times.gpu_memory_mb);
        fclose(f);
    }
    printf("GPU memory usage: %d MB\n%s", (int)times.gpu_memory_mb, avg);
}

void SLAMPipeline::processFrame(int i, Camera& cam) {
    requireEngine("processFrame(i, cam)");
    TORCH_CHECK(tsdf_engine != nullptr && model != nullptr, "processFrame(i, cam): setTsdfEngine() and a model first");
    processFrame(i, cam, torch::Tensor(), torch::Tensor());
}

void SLAMPipeline::loadConfig(const Config& c) { applyConfig(c, false); }

void SLAMPipeline::applyConfig(const Config& c, bool from_node) {
    // every key, with the field it goes to: configFields (slam_pipeline.hpp); a key the Config lacks leaves its field as it is
    ConfigReader reader{c, from_node};
    configFields(reader);
    TORCH_CHECK(sample_method == "random" || sample_method == "ours", "sample_method: 'random' or 'ours', got '", sample_method, "'");
    TORCH_CHECK(refine_cams == "keyframes" || refine_cams == "all", "refine_cams: 'keyframes' or 'all', got '", refine_cams, "'");
    if (log_iter == -1) log_iter = max_iterations - 1;   // src/pipeline.cpp:17-18
    updatePaths();
}

// ------------------------------------------------------------------ raycast -> tensors (runRaycastByCam :362-415)
TensorDict SLAMPipeline::runRaycastByCam(const Camera& cam, bool use_cam_depth) {
    requireEngine("runRaycastByCam");
    TensorDict m = raycastCam(cam, main_engine->camPoses);
    if (use_cam_depth) {  // slam_pipeline.cpp:405-408: the sensor depth instead of the raycast's (no call site of the loop uses it)
        TORCH_CHECK(cam.depth.defined(), "runRaycastByCam(use_cam_depth = true): the camera has no depth image");
        m["depth_map"] = cam.depth.contiguous().to(device);
        m["depth_map_clamped"] = RawGaussianModel::clampRefDepth(m["depth_map"]);
    }
    return m;
}

// slam_pipeline.cpp:367-379: a camera of the sequence is rendered with the intrinsics the engine stored for its frame
// (camIntrincs[cam.id]), any other camera with its own fx / fy / cx / cy
static ITMLib::ITMIntrinsics intrinsicsOf(const Camera& cam, const TsdfEngine* eng) {
    if (cam.id >= 0 && cam.id < (int)eng->camIntrincs.size()) return eng->camIntrincs[cam.id];
    ITMLib::ITMIntrinsics in;
    in.SetFrom(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy);
    return in;
}

// the pose a camera is rendered with: the engine's own for a frame of the sequence, else the camera's c2w
static ORUtils::SE3Pose poseOf(const Camera& cam, const std::vector<ORUtils::SE3Pose>& poses) {
    if (cam.id >= 0 && cam.id < (int)poses.size()) return poses[cam.id];
    ORUtils::SE3Pose pose;
    auto c = cam.c2w.to(torch::kCPU, torch::kFloat32).contiguous();
    pose.SetInvM(c.data_ptr<float>());
    pose.Coerce();
    return pose;
}

// the five result tensors of one view, from `alloc(h, w, channels)`
template <class Alloc>
static TensorDict resultMaps(const Camera& cam, Alloc&& alloc) {
    TensorDict m;
    m["color_map"] = alloc(cam.height, cam.width, 3);
    m["vertex_map"] = alloc(cam.height, cam.width, 3);
    m["confidence_map"] = alloc(cam.height, cam.width, 1);
    m["depth_map"] = alloc(cam.height, cam.width, 1);
    m["depth_map_clamped"] = alloc(cam.height, cam.width, 1);
    return m;
}

TensorDict SLAMPipeline::raycastCam(const Camera& cam, const std::vector<ORUtils::SE3Pose>& poses) {
    requireEngine("raycast");
    TsdfEngine* eng = main_engine;
    ORUtils::SE3Pose pose = poseOf(cam, poses);
    const auto F = f32(device);
    TensorDict m = resultMaps(cam, [&](int64_t h, int64_t w, int64_t c) { return torch::empty({h, w, c}, F); });
    auto w2c = poseInv(cam.c2w.to(torch::kCPU, torch::kFloat32)).contiguous();  // poseInv(cam.c2w): dataset pose (:398)
    ITMLib::ITMIntrinsics intr = intrinsicsOf(cam, eng);
    eng->runRaycast(&pose, &intr);
    check(gps_raycast_to_maps(cam.width, cam.height, reinterpret_cast<const float*>(eng->GetFreeVertex()->GetData(MEMORYDEVICE_CUDA)),
                              reinterpret_cast<const uint8_t*>(eng->GetFreeImage()->GetData(MEMORYDEVICE_CUDA)),
                              eng->getVoxelSize(), w2c.data_ptr<float>(), fptr(m["color_map"]), fptr(m["vertex_map"]),
                              fptr(m["confidence_map"]), fptr(m["depth_map"]), fptr(m["depth_map_clamped"]),
                              current_stream()), "gps_raycast_to_maps");
    stats.raycasts++;
    return m;
}

SLAMPipeline::RaycastStream& SLAMPipeline::raycastStream() {
    if (!rc_) rc_.reset(new RaycastStream(raycast_stream_kind));
    return *rc_;
}

void SLAMPipeline::beginAsyncRaycasts() {
    if (rc_) rc_->next = 0;
    if (!async_raycasts) return;
    RaycastStream& rc = raycastStream();
    // the raycast stream starts behind everything the current stream holds (the fusion of the keyframe; the previous
    // update's last readers of the engine's free-view scratch)
    hip_ok(hipEventRecord(rc.begin, c10::hip::getCurrentHIPStream().stream()), "hipEventRecord");
    hip_ok(hipStreamWaitEvent(rc.s.stream(), rc.begin, 0), "hipStreamWaitEvent");
}

void SLAMPipeline::waitRaycast(RaycastEvent ev) {
    if (ev) hip_ok(hipStreamWaitEvent(c10::hip::getCurrentHIPStream().stream(), ev, 0), "hipStreamWaitEvent");
}

// ------------------------------------------------------------------ frame bookkeeping (updateFrameList :319-360)
void SLAMPipeline::updateFrameList() {
    if (curr_frame_id == 0) return;
    if (curr_frame_id % localframe_cam_window_interval == 0) {
        localframe_cam_window.push_back(curr_cam);
        if ((int)localframe_cam_window.size() == localframe_cam_window_length + 1) localframe_cam_window.pop_front();
    }
    bool is_key = false;
    if (keyframe_cam_list.empty()) {
        is_key = true;
    } else {
        const Camera& last = keyframe_cam_list.back();
        auto a = last.c2w_slam.to(torch::kCPU, torch::kFloat32).contiguous();
        auto b = curr_cam.c2w_slam.to(torch::kCPU, torch::kFloat32).contiguous();
        const float* A = a.data_ptr<float>();
        const float* B = b.data_ptr<float>();
        float tr = 0.f;  // trace(Rp^T Rc)
        for (int r = 0; r < 3; r++)
            for (int k = 0; k < 3; k++) tr += A[4 * k + r] * B[4 * k + r];
        const float cos_t = std::max(-1.0f, std::min(1.0f, (tr - 1.f) / 2.f));
        const float theta = std::acos(cos_t) * 180.0f / (float)M_PI;
        const float dx = A[3] - B[3], dy = A[7] - B[7], dz = A[11] - B[11];
        const float trans = std::sqrt(dx * dx + dy * dy + dz * dz);
        is_key = theta > keyframe_theta_thres || trans > keyframe_trans_thres;
    }
    if (is_key) {
        keyframe_cam_list.push_back(curr_cam);
        std::lock_guard<std::mutex> lk(loss_mu_);
        keyframe_loss_dict[curr_cam.id] = {0.1f, (float)curr_frame_id, 0.f, 0.f, 0.f};   // slam_pipeline.cpp:355
    }
}

void SLAMPipeline::localFrameRaycast() { buildCurrentViews(liveSource(), kWindowBatch); }
void SLAMPipeline::keyFrameRaycast() { buildCurrentViews(liveSource(), kKeyframeBatch); }
void SLAMPipeline::initNewGaussians(TensorDict& rm) { initNewGaussiansFor(rm, curr_cam); }

// runRaycastByCam for several cameras of ONE volume state: one batched free-view chain (TsdfEngine::runRaycastBatch) instead
// of one chain per camera, then each view's tensor glue.  Same tensors as raycastCam per camera; one event covers them all.
std::vector<TensorDict> SLAMPipeline::raycastCams(const std::vector<const Camera*>& cams,
                                                  const std::vector<ORUtils::SE3Pose>& poses, RaycastEvent* ev_out, RaycastEvent use_event) {
    std::vector<TensorDict> out;
    if (cams.empty()) return out;
    requireEngine("raycast");
    TsdfEngine* eng = main_engine;
    const auto F = f32(device);
    // Whose pool the result tensors come from.  They are WRITTEN on the raycast stream and READ on the consumer's (the stream
    // current here: the map stream, or the frames stream in the sequential schedule).  Allocated with the consumer's stream
    // current they would be a write-after-read hazard when the FRAME thread enqueues update k+1's views while the worker is still
    // running update k on the map stream: the caching allocator may hand out a block the worker freed a moment ago that queued
    // map-stream kernels still read, and the raycast stream only waits for the frame's fusion.  So: allocated with the RAYCAST
    // stream current (a block of that pool is only reused in that stream's order) and the consumer registered with recordStream,
    // so that a freed block waits for the consumer's queued work before the raycast stream gets it again; the consumer itself
    // waits on the batch events.  (Only the allocations run under the raycast stream's guard: the pose glue below must not
    // inherit it.)
    const c10::hip::HIPStream consumer = c10::hip::getCurrentHIPStream();
    auto result = [&](int64_t h, int64_t w, int64_t c) {
        c10::optional<c10::hip::HIPStreamGuard> alloc_on_rc;
        if (ev_out) alloc_on_rc.emplace(raycastStream().s);
        torch::Tensor t = torch::empty({h, w, c}, F);
        // (the allocator's own entry point: Tensor::record_stream wants a c10::Stream of the masquerading "cuda" device type)
        if (ev_out) c10::hip::HIPCachingAllocator::recordStream(t.storage().data_ptr(), consumer);
        return t;
    };
    if (!raycast_pool_warm_) {
        // The result tensors of an update (5 per view, ~11 MB per 640x480 view) are allocated on the consumer's stream and freed
        // when the next update replaces them, so in steady state the caching allocator hands the same blocks out again -- but
        // while the keyframe list is still filling every update has one view more than the last, i.e. a fresh hipMalloc under
        // the allocator's lock in the middle of an update (measured: the frame thread's own 3.7 MB image allocation then waited
        // 3-6 ms for that lock in about one run in six).  Take the full set once, up front, and give it back to the cache.
        // (two sets where the frame thread enqueues update k+1's views while update k's are still being read)
        std::vector<torch::Tensor> warm;
        const int64_t H = cams[0]->height, W = cams[0]->width;
        const int sets = mapping_thread && pipeline_raycasts && async_raycasts ? 2 : 1;
        for (int k = 0; k < sets * (localframe_cam_window_length + keyframe_select_max); k++) {
            warm.push_back(result(H, W, 3)); warm.push_back(result(H, W, 3));
            warm.push_back(result(H, W, 1)); warm.push_back(result(H, W, 1));
            warm.push_back(result(H, W, 1));
        }
        raycast_pool_warm_ = true;
    }
    std::vector<ORUtils::SE3Pose> view_poses(cams.size());
    std::vector<ITMLib::ITMIntrinsics> view_intr(cams.size());
    std::vector<torch::Tensor> w2c(cams.size());
    for (size_t k = 0; k < cams.size(); k++) {
        const Camera& cam = *cams[k];
        view_poses[k] = poseOf(cam, poses);
        view_intr[k] = intrinsicsOf(cam, eng);
        out.push_back(resultMaps(cam, result));
        w2c[k] = poseInv(cam.c2w.to(torch::kCPU, torch::kFloat32)).contiguous();  // poseInv(cam.c2w): dataset pose (:398)
    }
    c10::optional<c10::hip::HIPStreamGuard> on_rc;
    if (ev_out) on_rc.emplace(raycastStream().s);
    constexpr size_t kMaxBatch = 12;  // views per gps_tsdf_free_raycast_batch call; a later chunk reuses the render states in stream order
    for (size_t base = 0; base < cams.size(); base += kMaxBatch) {
        const size_t cnt = std::min(kMaxBatch, cams.size() - base);
        std::vector<TsdfEngine::ViewMaps> maps(cnt);
        for (size_t k = 0; k < cnt; k++) {
            TensorDict& m = out[base + k];
            maps[k] = {w2c[base + k].data_ptr<float>(), fptr(m["color_map"]), fptr(m["vertex_map"]), fptr(m["confidence_map"]),
                       fptr(m["depth_map"]), fptr(m["depth_map_clamped"])};
        }
        // (the tensor glue of every view -- gps_raycast_to_maps -- is written by the batch's last kernel)
        const std::vector<ITMLib::ITMIntrinsics> intr(view_intr.begin() + base, view_intr.begin() + base + cnt);
        eng->runRaycastBatch(std::vector<ORUtils::SE3Pose>(view_poses.begin() + base, view_poses.begin() + base + cnt), nullptr, &maps, &intr);
    }
    if (ev_out) {
        *ev_out = use_event ? use_event : raycastStream().nextEvent();
        hip_ok(hipEventRecord(*ev_out, c10::hip::getCurrentHIPStream().stream()), "hipEventRecord");
    }
    stats.raycasts += (int64_t)cams.size();
    return out;
}

// The view set of one map update: the local window's cameras, then (sample_method "random") up to keyframe_select_max history
// keyframes drawn without replacement, each with its free-view raycast -- localFrameRaycast + keyFrameRaycast (:417-448, :528-561).
// Every schedule builds its sets HERE, and the schedules give the same bits (test_overlapped_mapping_equals_sequential_schedule)
// because of one rule: ONE draw loop per update, from rng_kf_ and nothing else, whichever thread builds the set and however the
// views are batched.  rng_kf_ has no other user; the builds of successive updates never overlap (one frame thread, or one worker
// the frame thread waits for), so every schedule draws the same numbers in the same order.
SLAMPipeline::RaycastMs SLAMPipeline::buildViews(UpdateViews& out, const ViewSource& src, int parts, const RaycastEvent* job_events) {
    requireEngine("raycast");
    const bool one_batch = parts == kOneBatch, with_events = job_events || async_raycasts;
    std::vector<const Camera*> cams;   // the batch being collected
    auto raycastBatch = [&](RaycastEvent job_event) {
        RaycastEvent ev = nullptr;
        for (TensorDict& m : raycastCams(cams, src.poses, with_events ? &ev : nullptr, job_event)) {
            out.raycasts.push_back(std::move(m));
            out.events.push_back(ev);
        }
        if (ev) out.last_event = ev;
        cams.clear();
    };
    // (the set `out` held before is released between the two batches -- after the single one -- and not earlier: the keyframes'
    // batch then finds its blocks in the caching allocator again, and the steady-state footprint stays the warmed pool's)
    UpdateViews previous;
    const double t0 = now_ms();
    if (parts & kWindowBatch) {
        previous = std::move(out);
        out = UpdateViews();
        if (!job_events) beginAsyncRaycasts();   // (a job's raycast stream is ordered by the frame thread: keyframeStepThreaded)
        out.cams.assign(src.window.begin(), src.window.end());
        out.window_len = src.window.size();
        for (const Camera& cam : src.window) cams.push_back(&cam);
        if (!one_batch) raycastBatch(job_events ? job_events[0] : nullptr);
    }
    const double t1 = now_ms();
    if (parts & kKeyframeBatch) {
        if (!one_batch) previous = UpdateViews();
        if (parts == kKeyframeBatch) {   // the public two-step API: the window's views stay, history views of an earlier call go
            out.cams.erase(out.cams.begin() + out.window_len, out.cams.end());
            out.raycasts.erase(out.raycasts.begin() + out.window_len, out.raycasts.end());
            out.events.resize(out.window_len);
            if (async_raycasts && !rc_) beginAsyncRaycasts();   // (no localFrameRaycast() before it: order the raycast stream now)
        }
        out.frame_id = src.frame_id;
        const int n = sample_method == "random" ? std::min<int>(keyframe_select_max, (int)src.keyframes.size()) : 0;   // :538
        ::RandomSelector<Camera> sel(src.keyframes, rng_kf_);
        for (int k = 0; k < n; k++) {
            const Camera* cam = sel.getNext().second;
            out.cams.push_back(*cam);
            cams.push_back(cam);
        }
        raycastBatch(job_events ? job_events[1] : nullptr);
    }
    const double t2 = now_ms();
    return one_batch ? RaycastMs{t2 - t0, 0.0} : RaycastMs{t1 - t0, t2 - t1};
}

SLAMPipeline::RaycastMs SLAMPipeline::buildCurrentViews(const ViewSource& src, int parts) {
    if (parts & kWindowBatch) localframe_raycast_window.clear();   // (views_ alone holds the previous window's tensors: see buildViews)
    const RaycastMs ms = buildViews(views_, src, parts);
    if (parts & kWindowBatch) localframe_raycast_window.assign(views_.raycasts.begin(), views_.raycasts.begin() + views_.window_len);
    return ms;
}

void SLAMPipeline::adoptViews(UpdateViews&& v) {
    views_ = std::move(v);
    localframe_raycast_window.assign(views_.raycasts.begin(), views_.raycasts.begin() + views_.window_len);
}

// ------------------------------------------------------------------ initNewGaussians :450-526
void SLAMPipeline::initNewGaussiansFor(TensorDict& rm, const Camera& cam) {
    torch::NoGradGuard no_grad;
    if (views_.window_len > 0) waitRaycast(views_.eventOf(views_.window_len - 1));  // rm is the newest window camera's result
    const auto &depth = rm.at("depth_map"), &color = rm.at("color_map"), &vertex = rm.at("vertex_map");
    int frame_num = local_opt_interval;
    // valid = depth in (min, max) & vertex.sum(2) != 0;  mask = mean|src - image| > thres & valid [& alpha < max]: one launch
    // (gps_new_gaussian_mask) instead of the reference's ~12 tensor ops (:455-480)
    const int64_t H = cam.image.size(0), W = cam.image.size(1);
    auto image = cam.image.contiguous(), depth_c = depth.contiguous(), vertex_c = vertex.contiguous();
    auto mask = torch::empty({H, W, 1}, torch::TensorOptions().dtype(torch::kBool).device(depth.device()));
    torch::Tensor src = color.contiguous(), alpha;
    if (model->getGaussianNum() == 0) {
        frame_num += 1;
    } else {
        auto res = model->forward(cam, depth, color);
        src = res.at("rgb").contiguous();
        alpha = res.at("alpha").contiguous();
    }
    check(gps_new_gaussian_mask((int)W, (int)H, fptr(depth_c), fptr(src), fptr(image), fptr(vertex_c), fptr(alpha), depth_vis_min,
                                depth_vis_max, color_error_thres, alpha_vis_max, reinterpret_cast<uint8_t*>(mask.data_ptr<bool>()),
                                current_stream()), "gps_new_gaussian_mask");
    rm["normal_map"] = computeNormalMap(vertex);
    stats.added += model->addGaussians(cam, rm, mask, new_gs_sample_ratio, frame_num, gen_);
}

// ------------------------------------------------------------------ checkKeyFrameError :293-317
// The loss record of every history keyframe in the current optimise list (the entries behind the local window's).
void SLAMPipeline::checkKeyFrameError() {
    torch::NoGradGuard no_grad;
    Config wc;
    wc.num["ssim_weight"] = ssim_weight; wc.num["depth_weight"] = depth_weight;
    // The window length and frame number are those of the update the view set belongs to (recorded when it was built): with
    // overlapped / threaded mapping this check runs while the frame thread keeps pushing into localframe_cam_window and
    // advancing curr_frame_id, or one update late.  keyframe_loss_dict is shared with updateFrameList (frame thread): loss_mu_.
    for (size_t k = views_.window_len; k < views_.cams.size(); k++) {
        const Camera& cam = views_.cams[k];
        TensorDict& rc = views_.raycasts[k];
        waitRaycast(views_.eventOf(k));
        auto res = model->forward(cam, rc.at("depth_map"), rc.at("color_map"));
        auto loss = model->computeLoss(res, cam, wc, rc.at("depth_map") > 0);
        const float total = loss.at("total").item<float>();
        const float confidence_mean = rc.at("confidence_map").mean().item<float>();
        std::lock_guard<std::mutex> lk(loss_mu_);
        auto it = keyframe_loss_dict.find(cam.id);
        float opt_count = it != keyframe_loss_dict.end() && it->second.size() > 3 ? it->second[3] : 0.f;
        if (total > loss_thres) opt_count += 1.f;
        keyframe_loss_dict[cam.id] = {total, (float)views_.frame_id, confidence_mean, opt_count};
    }
}

// ------------------------------------------------------------------ localOptimize :195-289
void SLAMPipeline::localOptimize() {
    localOptimizeBegin();
    optimizeIterations(opt_pending_);
}

void SLAMPipeline::localOptimizeBegin() {
    opt_pending_ = 0;
    if (model->getGaussianNum() == 0) return;
    model->initOptimizers(-1, scene_scale);
    opt_loader_.reset(new ::RandomSelector<Camera>(views_.cams, rng_));
    opt_peek_valid_ = false;
    opt_pending_ = local_opt_iters;
}

// the next `count` iterations of the current localOptimize (cameras drawn in the same order as the all-at-once loop)
void SLAMPipeline::optimizeIterations(int count) {
    for (; count > 0 && opt_pending_ > 0; count--, opt_pending_--) {
        // the camera of THIS iteration was drawn one iteration early (same draws in the same order), so that the previous
        // iteration's backward kernel could run its preprocessing forward in its tail (RawGaussianModel::trainStep next_cam)
        auto pick = opt_peek_valid_ ? opt_peek_ : opt_loader_->getNext();
        opt_peek_valid_ = false;
        const Camera* next_cam = nullptr;
        if (canRunAhead() && opt_pending_ > 1) {
            opt_peek_ = opt_loader_->getNext();
            opt_peek_valid_ = true;
            next_cam = opt_peek_.second;
        }
        optimizeOne(*pick.second, views_.raycasts[pick.first], views_.eventOf(pick.first), next_cam);
    }
}

void SLAMPipeline::optimizeOne(const Camera& cam, TensorDict& rc, RaycastEvent ev, const Camera* next_cam) {
    waitRaycast(ev);
    const bool terms = ssim_weight > 0 || depth_weight > 0;
    // loss terms inside the fused step (fused_loss_terms), with or without an exposure row of the camera
    const bool fused_terms = terms && fused_loss_terms;
    Config wc;
    if (terms) { wc.num["ssim_weight"] = ssim_weight; wc.num["depth_weight"] = depth_weight; }
    if (fused_terms) {
        model->trainStep(cam, rc.at("depth_map"), rc.at("color_map"), rc.at("depth_map_clamped"), next_cam, wc);
    } else if (terms) {
        // losses beyond L1: the reference's own sequence (slam_pipeline.cpp:247-254) through the autograd route
        auto res = model->forward(cam, rc.at("depth_map"), rc.at("color_map"));
        auto loss = model->computeLoss(res, cam, wc);
        loss.at("total").backward();
        model->optimizersStep();
        model->optimizersZeroGrad();
        autograd_iters++;
    } else {
        model->trainStep(cam, rc.at("depth_map"), rc.at("color_map"), rc.at("depth_map_clamped"), next_cam);
    }
    stats.opt_iters++;
}

// ------------------------------------------------------------------ gesTrainCams (src/pipeline.cpp:229-319)
std::vector<Camera> SLAMPipeline::refineKeyframeCams() const {
    std::vector<Camera> out(keyframe_cam_list);
    for (const Camera& w : localframe_cam_window) {
        bool have = false;
        for (const Camera& k : out) have = have || k.id == w.id;
        if (!have) out.push_back(w);
    }
    return out;
}

int64_t SLAMPipeline::refineCacheBytes(const std::vector<Camera>& cams) const {
    int64_t bytes = 0;   // per pixel: colour 3 + depth 1 + clamped depth 1 floats of the base layers, 3 (+ 1 with a depth) of the camera's images
    for (const Camera& cam : cams) bytes += (int64_t)cam.width * cam.height * (3 + 1 + 1 + 3 + (cam.depth.defined() ? 1 : 0)) * (int64_t)sizeof(float);
    return bytes;
}

// cameras as the optimise iterations want them: copies whose image and pose pack are on the device
static std::vector<Camera> refineDeviceCams(const std::vector<Camera>& cams, const torch::Device& device) {
    std::vector<Camera> out(cams);
    for (Camera& c : out) {
        TORCH_CHECK(c.image.defined(), "gesTrainCams: camera ", c.id, " has no image");
        c.toGPU(device);   // (a camera of the pipeline's lists is there already and keeps its upload)
    }
    return out;
}

int SLAMPipeline::gesTrainCams(const std::vector<Camera>& cams, int max_iters, int64_t seed) {
    flush();
    requireEngine("gesTrainCams");
    TORCH_CHECK(!cams.empty(), "gesTrainCams: no cameras");
    const int64_t need = refineCacheBytes(cams);
    TORCH_CHECK(need <= refine_cache_mb * (int64_t(1) << 20), "gesTrainCams: the base layers and images of ", cams.size(), " cameras need ",
                (need + (1 << 20) - 1) >> 20, " MiB on the device, refine_cache_mb allows ", refine_cache_mb,
                " (fewer cameras -- refine_cams: keyframes -- or a larger refine_cache_mb)");
    std::vector<Camera> dev = refineDeviceCams(cams, device);
    // the base layers from the engine's final volume: runRaycastByCam(cam, false)'s maps, a batch of views at a time (the vertex and
    // confidence maps of a batch are released before the next one)
    std::vector<TensorDict> layers;
    {
        torch::NoGradGuard no_grad;
        constexpr size_t kBatch = 12;
        for (size_t base = 0; base < dev.size(); base += kBatch) {
            std::vector<const Camera*> batch;
            for (size_t k = base; k < std::min(dev.size(), base + kBatch); k++) batch.push_back(&dev[k]);
            for (TensorDict& m : raycastCams(batch, main_engine->camPoses)) {
                TensorDict keep;
                for (const char* name : {"color_map", "depth_map", "depth_map_clamped"}) keep[name] = m.at(name);
                layers.push_back(std::move(keep));
            }
        }
    }
    return refineLoop(dev, layers, max_iters, seed);
}

int SLAMPipeline::gesTrainCams(const std::vector<Camera>& cams, const std::vector<TensorDict>& base_layers, int max_iters, int64_t seed) {
    flush();
    TORCH_CHECK(!cams.empty(), "gesTrainCams: no cameras");
    TORCH_CHECK(base_layers.size() == cams.size(), "gesTrainCams: ", base_layers.size(), " base layers for ", cams.size(), " cameras");
    const int64_t need = refineCacheBytes(cams);
    TORCH_CHECK(need <= refine_cache_mb * (int64_t(1) << 20), "gesTrainCams: the base layers and images of ", cams.size(), " cameras need ",
                (need + (1 << 20) - 1) >> 20, " MiB on the device, refine_cache_mb allows ", refine_cache_mb,
                " (fewer cameras -- refine_cams: keyframes -- or a larger refine_cache_mb)");
    std::vector<Camera> dev = refineDeviceCams(cams, device);
    std::vector<TensorDict> layers;
    for (size_t k = 0; k < cams.size(); k++) {
        TensorDict keep;
        for (const auto& layer : {std::make_pair("color_map", 3), std::make_pair("depth_map", 1)}) {
            const char* name = layer.first;
            TORCH_CHECK(base_layers[k].count(name), "gesTrainCams: base layer ", k, " has no ", name);
            keep[name] = base_layers[k].at(name).to(device, torch::kFloat32).contiguous();
            TORCH_CHECK(keep[name].numel() == (int64_t)dev[k].width * dev[k].height * layer.second, "gesTrainCams: base layer ", k, ": ", name,
                        " does not have the camera's image size");
        }
        keep["depth_map_clamped"] = RawGaussianModel::clampRefDepth(keep["depth_map"]);
        layers.push_back(std::move(keep));
    }
    return refineLoop(dev, layers, max_iters, seed);
}

int SLAMPipeline::refineLoop(const std::vector<Camera>& cams, std::vector<TensorDict>& layers, int max_iters, int64_t seed) {
    TORCH_CHECK(model != nullptr, "gesTrainCams: no model (SLAMTrainCams / setModel first)");
    TORCH_CHECK(model->getRenderMethod() == "ges", "gesTrainCams: render_method must be 'ges', got '", model->getRenderMethod(), "'");   // :231
    if (max_iters < 0) max_iters = max_iterations;
    if (seed < 0) seed = refine_seed;
    TORCH_CHECK(selected_cam_idx >= -1 && selected_cam_idx < (int)cams.size(), "gesTrainCams: selected_cam_idx ", selected_cam_idx, " with ",
                cams.size(), " cameras");
    if (curr_iter >= max_iters || model->getGaussianNum() == 0) return 0;
    model->initOptimizers(refine_lr_decay ? max_iters : -1, scene_scale);   // ONE optimiser state for the whole call (:267)
    gpsh::RandomSelector<Camera> loader(cams, (uint64_t)seed);
    auto draw = [&]() -> size_t { return selected_cam_idx == -1 ? loader.getNext().originalIndex : (size_t)selected_cam_idx; };
    // the L1 route accumulates its loss in lossSum(): each log entry is the mean since the last one (with loss weights lossSum() holds
    // the last step's total and that is the entry)
    const bool terms = ssim_weight > 0 || depth_weight > 0;
    auto zeroLoss = [&] { if (model->lossSum().defined()) model->lossSum().zero_(); };
    zeroLoss();
    int since_log = 0;
    const int first = curr_iter;
    size_t next_idx = 0;
    bool have_next = false;
    for (; curr_iter < max_iters; curr_iter++) {
        const size_t idx = have_next ? next_idx : draw();
        have_next = false;
        const Camera* next_cam = nullptr;
        if (canRunAhead() && curr_iter + 1 < max_iters) {   // the next iteration's camera, one iteration early: the same draws in the same order
            next_idx = draw();
            have_next = true;
            next_cam = &cams[next_idx];
        }
        model->updateSH(curr_iter);   // (a step whose successor has another degree arms nothing the successor accepts: PrefetchKey)
        optimizeOne(cams[idx], layers[idx], nullptr, next_cam);
        model->schedulersStep();
        since_log++;
        const bool last = curr_iter + 1 == max_iters;
        if (last || (log_iter > 0 && (curr_iter + 1) % log_iter == 0)) {
            torch::Tensor sum = model->lossSum();
            const float value = sum.defined() ? sum.item<float>() : 0.f;   // (blocks: the loop's host synchronisation, with the check below)
            refine_log.push_back({curr_iter, terms ? value : value / (float)since_log});
            zeroLoss();
            since_log = 0;
            model->checkBinningCapacity();
        }
    }
    return curr_iter - first;
}

// ------------------------------------------------------------------ rawTrainCams (src/pipeline.cpp:155-226)
int SLAMPipeline::rawTrainCams(const std::vector<Camera>& cams, int max_iters, int64_t seed, bool densify) {
    flush();
    TORCH_CHECK(model != nullptr, "rawTrainCams: no model (setModel first)");
    TORCH_CHECK(model->getRenderMethod() == "raw", "rawTrainCams: render_method must be 'raw', got '", model->getRenderMethod(), "'");   // :157
    TORCH_CHECK(!cams.empty(), "rawTrainCams: no cameras");
    if (max_iters < 0) max_iters = max_iterations;
    if (seed < 0) seed = refine_seed;
    TORCH_CHECK(selected_cam_idx >= -1 && selected_cam_idx < (int)cams.size(), "rawTrainCams: selected_cam_idx ", selected_cam_idx, " with ",
                cams.size(), " cameras");
    if (curr_iter >= max_iters || model->getGaussianNum() == 0) return 0;
    std::vector<Camera> dev = refineDeviceCams(cams, device);
    model->initOptimizers(max_iters, scene_scale);   // ONE optimiser state for the whole call, with the means' scheduler (:176)
    model->setDensifySeed(seed);                     // the split samples: a second stream of the same seed
    // one seed, one result: the rasterizer's backward with a reduction of fixed order (the atomic one differs run to run in the last
    // bits, and the differences grow over thousands of iterations and densifications)
    struct Ordered {
        SLAMGaussianModel* m; bool was;
        explicit Ordered(SLAMGaussianModel* m) : m(m), was(m->ordered_raw_backward) { m->ordered_raw_backward = true; }
        ~Ordered() { m->ordered_raw_backward = was; }
    } ordered(model);
    gpsh::RandomSelector<Camera> loader(dev, (uint64_t)seed);
    Config wc;
    wc.num["ssim_weight"] = ssim_weight; wc.num["depth_weight"] = depth_weight;
    const int first = curr_iter;
    for (; curr_iter < max_iters; curr_iter++) {
        const size_t idx = selected_cam_idx == -1 ? loader.getNext().originalIndex : (size_t)selected_cam_idx;
        const Camera& cam = dev[idx];
        model->updateSH(curr_iter);
        TensorDict render_res = model->forward(cam);
        if (densify) render_res["means2d"].retain_grad();
        TensorDict loss = model->computeLoss(render_res, cam, wc);
        loss["total"].backward();
        model->optimizersStep();
        model->optimizersZeroGrad();
        if (densify) model->stepPostBackward(render_res, cam, scene_scale, curr_iter);
        model->schedulersStep();
        stats.opt_iters++;
        const bool last = curr_iter + 1 == max_iters;
        if (last || (log_iter > 0 && (curr_iter + 1) % log_iter == 0))   // (blocks: the loop's only read of the loss)
            refine_log.push_back({curr_iter, loss["total"].item<float>()});
        if (model->getGaussianNum() == 0) { curr_iter++; break; }   // everything pruned: nothing left to optimise
    }
    return curr_iter - first;
}

int SLAMPipeline::trainCams(const std::vector<Camera>& cams, const std::string& mode) {
    TORCH_CHECK(mode == "raw" || mode == "ges", "trainCams: mode 'raw' or 'ges', got '", mode, "'");
    TORCH_CHECK(model != nullptr, "trainCams: no model (setModel first)");
    TORCH_CHECK(model->getRenderMethod() == mode, "trainCams: render_method must be '", mode, "', got '", model->getRenderMethod(), "'");
    return mode == "raw" ? rawTrainCams(cams) : gesTrainCams(cams);
}

// ------------------------------------------------------------------ removeRedundantGs :564-586
void SLAMPipeline::removeRedundantGs() {
    torch::NoGradGuard no_grad;
    if (model->getGaussianNum() == 0) return;
    // delete = max real scale < small or > large, or real opacity < low (:566-575): one launch; the compaction of the keep
    // mask synchronises with the map stream once (the reference syncs 5 times here for its printf)
    const int64_t N = model->getGaussianNum();
    const auto dev = model->getMeans().device();
    auto del = torch::empty({N}, torch::TensorOptions().dtype(torch::kBool).device(dev));
    auto keep = torch::empty({N}, torch::TensorOptions().dtype(torch::kBool).device(dev));
    check(gps_prune_mask((int)N, fptr(model->getScales()), fptr(model->getOpacities()), small_scale_thres, large_scale_thres,
                         low_opac_thres, reinterpret_cast<uint8_t*>(del.data_ptr<bool>()),
                         reinterpret_cast<uint8_t*>(keep.data_ptr<bool>()), current_stream()), "gps_prune_mask");
    const int64_t kept = model->pruneKeep(keep);
    // the host is synchronised with the map stream right here: look at the capacity flags the kernels cannot raise as exceptions
    model->checkBinningCapacity();
    if (main_engine) main_engine->checkRenderingBlocks();
    stats.pruned += N - kept;
}

// ------------------------------------------------------------------ renderEvalImgs :588-695 (tensors instead of image files)
TensorDict SLAMPipeline::renderEvalCam(const Camera& cam, const std::vector<std::string>& names) {
    TensorDict r;
    TORCH_CHECK(cam.on_device(), "Camera::toGPU() must run before the camera is rendered");
    auto rc = runRaycastByCam(cam, false);
    r["raycast_color"] = rc.at("color_map");
    r["raycast_depth"] = rc.at("depth_map");
    // what the reference writes to disk, as it quantises it (cv_utils.cpp:57-76 tensorToImage: (t * 255.0).toType(kU8),
    // truncation; :79-101 tensorToDepth: convertTo(CV_16UC1, 1000) = saturate_cast<ushort>(round-half-even(d * 1000)))
    r["raycast_color_u8"] = (r["raycast_color"] * 255.0).toType(torch::kUInt8);
    r["raycast_depth_u16"] = torch::round(r["raycast_depth"] * 1000.0f).clamp(0.0, 65535.0).to(torch::kInt32);
    if (cam.image.defined()) r["gt_u8"] = (cam.image.to(device) * 255.0).toType(torch::kUInt8);
    if (model->getGaussianNum() > 0) {
        auto res = model->forward(cam, rc.at("depth_map"), rc.at("color_map"));
        for (const std::string& name : names) {
            if (name == "rgb") {
                r["rgb"] = torch::clamp(res.at("rgb"), 0, 1);
                r["rgb_u8"] = (r["rgb"] * 255.0).toType(torch::kUInt8);   // render/<frame>.color.jpg before the JPEG encoder
                if (cam.image.defined()) {
                    auto mse = torch::mean(torch::square(r["rgb"] - cam.image.to(device)));
                    r["psnr"] = -10.0 * torch::log10(mse);
                    // the number the reference reports: scripts/metric.py reads the 8-bit render / gt files back as
                    // u8 / 255 (to_tensor) and takes 20 log10(1 / sqrt(mse)) (scripts/utils/image_utils.py:19-21); the lossy
                    // JPEG encoder in between is I/O outside this library
                    auto a = r["rgb_u8"].to(torch::kFloat32) / 255.0f, b = r["gt_u8"].to(torch::kFloat32) / 255.0f;
                    r["psnr_u8"] = 20.0 * torch::log10(1.0 / torch::sqrt(torch::mean(torch::square(a - b))));
                }
            } else if (name == "alpha" || name == "depth") {
                r[name] = res.at(name).clone();
            }
        }
        if (r.count("rgb")) r["rgb"] = r["rgb"].clone();  // forward() returns views of buffers the next camera overwrites
    }
    return r;
}

std::vector<TensorDict> SLAMPipeline::renderEvalImgs(const std::vector<Camera>& cams, const std::vector<std::string>& names) {
    torch::NoGradGuard no_grad;
    flush();
    std::vector<TensorDict> out;
    for (const Camera& cam : cams) out.push_back(renderEvalCam(cam, names));
    return out;
}

// ------------------------------------------------------------------ image evaluation (image_eval.hpp): scripts/metric.py on tensors
ImageEvalResult SLAMPipeline::evalImages(const std::vector<Camera>& cams, bool depth_mask, const std::string& source) {
    torch::NoGradGuard no_grad;
    flush();
    TORCH_CHECK(source == "rgb" || source == "raycast_color", "evalImages: unknown source '", source, "' (rgb or raycast_color)");
    TORCH_CHECK(!cams.empty(), "evalImages: no cameras");
    const std::string key = source + "_u8";
    std::vector<torch::Tensor> renders, gts, depths;
    ImageEvalResult out;
    for (const Camera& cam : cams) {
        TORCH_CHECK(cam.image.defined(), "evalImages: camera ", cam.id, " has no image");
        if (depth_mask) TORCH_CHECK(cam.has_depth && cam.depth.defined(), "evalImages: depth_mask needs a depth, camera ", cam.id, " has none");
        TensorDict r = renderEvalCam(cam, {"rgb"});
        TORCH_CHECK(r.count(key), "evalImages: source '", source, "' needs a model with Gaussians");
        renders.push_back(r.at(key));
        gts.push_back(r.at("gt_u8"));
        if (depth_mask) depths.push_back(cam.depth.to(device, torch::kFloat32).reshape({cam.height, cam.width}));
        out.cam_ids.push_back(cam.id);
    }
    out.metrics = imageMetrics(torch::stack(renders), torch::stack(gts), depth_mask ? torch::stack(depths) : torch::Tensor());
    auto psnr = out.metrics.psnr.cpu(), ssim = out.metrics.ssim.cpu();
    out.psnr.assign(psnr.data_ptr<double>(), psnr.data_ptr<double>() + psnr.numel());
    out.ssim.assign(ssim.data_ptr<double>(), ssim.data_ptr<double>() + ssim.numel());
    out.psnr_mean = out.metrics.psnr_mean;
    out.ssim_mean = out.metrics.ssim_mean;
    return out;
}

// ------------------------------------------------------------------ geometry / trajectory evaluation (geom_eval.hpp)
GeomEvalResult SLAMPipeline::evalGeometry(const torch::Tensor& gt, const torch::Tensor& transform, const std::vector<double>& dist_thres,
                                          int64_t sample_nums, uint64_t seed) {
    flush();
    requireEngine("evalGeometry");
    return main_engine->EvalMesh(gt, transform, dist_thres, sample_nums, seed);
}

AteResult SLAMPipeline::evalTrajectory() {
    flush();
    requireEngine("evalTrajectory");
    const auto& est = main_engine->camPoses;
    const auto& gt = main_engine->gtC2wPoses;
    TORCH_CHECK(est.size() == gt.size(), "evalTrajectory: ", est.size(), " stored poses against ", gt.size(), " ground-truth poses");
    TORCH_CHECK(est.size() >= 3, "evalTrajectory: at least three frames are needed");
    const int64_t n = (int64_t)est.size();
    auto e = torch::empty({n, 4, 4}, torch::kFloat64), g = torch::empty({n, 4, 4}, torch::kFloat64);
    for (int64_t i = 0; i < n; i++) {
        const float* invM = est[i].GetInvM();   // ORUtils layout (column-major) -> row-major c2w
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) e[i][r][c] = (double)invM[4 * c + r];
        g[i] = gt[i].to(torch::kCPU, torch::kFloat64).reshape({4, 4});
    }
    return ate(e, g);
}

// ------------------------------------------------------------------ one SLAM frame (body of SLAMTrainCams :69-132)
void SLAMPipeline::processFrameImpl(int i, Camera& cam, const torch::Tensor& rgb_u8, const torch::Tensor& depth_mm_i16) {
    curr_frame_id = i;
    const double tt0 = now_ms();
    gate_wait_ms_ = handover_wait_ms_ = 0.0;
    // (with the tracker on the engine does not read them: kept for evalTrajectory)
    if ((!main_engine->trackingActive || cam.c2w.defined()) && (int)main_engine->gtC2wPoses.size() <= main_engine->framesSeen)
        main_engine->gtC2wPoses.push_back(cam.c2w);
    ITMTrackingState* ts;
    torch::Tensor frame_rgba;
    if (rgb_u8.defined()) {
        ts = main_engine->ProcessFrame(rgb_u8, depth_mm_i16);
    } else {
        // slam_pipeline.cpp:77-78: the CLIEngine owns the sequence (host memory) and uploads the frame
        TORCH_CHECK(tsdf_engine != nullptr && i == tsdf_engine->currentFrameNo, "frame ", i, " is not the CLIEngine's next frame");
        tsdf_engine->ProcessFrame();
        ts = main_engine->GetTrackingState();
        // (no float copy of the image kept for this camera: it is derived below, with the pose pack, from the uchar4 frame
        // UpdateView just put into HBM -- 3 of its 4 bytes per pixel instead of uploading 12 more as Camera::toGPU would)
        if (!cam.image.defined()) frame_rgba = main_engine->currentRgb();  // [H,W,4] u8, contiguous
    }
    if (trace_frames) {
        trace_live.push_back(main_engine->GetLiveVertex()->tensor().clone());
        trace_counters.push_back(main_engine->counters().clone());
        auto t = torch::empty({2, 16}, torch::kFloat32);
        const ORUtils::SE3Pose& p = main_engine->camPoses.back();
        for (int k = 0; k < 16; k++) { t[0][k] = p.GetM()[k]; t[1][k] = p.GetInvM()[k]; }
        trace_poses.push_back(t);
    }
    // est_pose = pose_d->GetInvM() (:81-82): ORUtils column-major -> row-major tensor
    auto est = torch::empty({4, 4}, torch::kFloat32);
    const float* invM = ts->pose_d->GetInvM();
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) est.data_ptr<float>()[4 * r + c] = invM[4 * c + r];
    cam.c2w_slam = est;
    if (!main_engine->lastFrameFused()) {
        // a frame the engine did not fuse (failure modes: tracking lost, or the frames right after a relocalisation) adds nothing
        // to the map: it is not offered as a keyframe and triggers no update.  Its camera still has the engine's pose.
        if (frame_rgba.defined()) tsdf_engine->markConsumed();
        stats.frames++;
        times.per_frame += now_ms() - tt0;
        return;
    }
    // `curr_cam = cams[i]; curr_cam.toGPU();` (:83-84): a COPY of the caller's camera goes to the device -- the caller's keeps the
    // pose and no device tensors, so a frame's 12-byte-per-pixel image lives exactly as long as the pipeline's lists hold it
    // (held by the caller's camera it stayed for the whole run: 3.7 MB per frame at 640x480, i.e. a fresh 20 MB hipMalloc by the
    // frame thread every fifth frame instead of the caching allocator handing the previous frame's block out again)
    curr_cam = cam;
    curr_cam.invalidate();
    const double tt1 = now_ms();
    curr_cam.toGPU(device, frame_rgba);
    const double tt2 = now_ms();
    if (frame_rgba.defined()) tsdf_engine->markConsumed();  // the staging slot's last reader is the conversion toGPU just enqueued
    updateFrameList();
    stats.frames++;
    const double tt_lists = now_ms();
    times.per_frame += tt_lists - tt0;   // the reference's perFrame_start .. perFrame_end (slam_pipeline.cpp:73-96)
    if (work_mode == "recon") return;
    if (i % local_opt_interval == 0 && i > 0) {
        if (!views_reserved_) {  // every free-view render state an update can need, once, before the first update
            main_engine->reserveViews(localframe_cam_window_length + keyframe_select_max);
            views_reserved_ = true;
        }
        if (overlap_mapping && mapping_thread) keyframeStepThreaded();
        else if (overlap_mapping) keyframeStepOverlapped();
        else keyframeStep();
        times.keyframe_step += now_ms() - tt_lists;
    }
    const double thr = frame_report_ms, tt3 = now_ms();
    if (thr >= 0.0 && tt3 - tt0 > thr)
        fprintf(stderr, "[pipe] frame %d: %.3f ms = engine %.3f (tracker %.3f, fusion enqueue %.3f, gate wait %.3f) + toGPU %.3f + lists / keyframe step %.3f (hand-over wait %.3f)\n",
                i, tt3 - tt0, tt1 - tt0, main_engine->trackDiag(14), main_engine->trackDiag(15), gate_wait_ms_, tt2 - tt1, tt3 - tt2, handover_wait_ms_);
}

// ------------------------------------------------------------------ tracking / mapping overlap (see slam_pipeline.hpp)

void SLAMPipeline::processFrame(int i, Camera& cam, const torch::Tensor& rgb_u8, const torch::Tensor& depth_mm_i16) {
    requireEngine("processFrame");
    // room for the tracker's evaluations beside the strip backward only while the two chains really run side by side (the strip
    // kernel alone is faster without the reserve: include/gps_slam_hip.h)
    gps_set_frame_chain_reserve(overlap_mapping ? frame_chain_reserve : 0);
    if (!overlap_mapping) { processFrameImpl(i, cam, rgb_u8, depth_mm_i16); return; }
    // overlap: frames run on a HIGH-priority stream of their own, so that the short, latency-bound tracker kernels are
    // dispatched ahead of the map stream's long rasterizer kernels; ordered after the caller's stream (inputs), and the
    // caller's stream is re-joined in flush()
    ensureStreams();
    const hipStream_t caller = c10::hip::getCurrentHIPStream().stream();
    c10::hip::HIPStream& fs = streams_->frame;
    if (caller != fs.stream()) {
        hip_ok(hipEventRecord(streams_->caller, caller), "hipEventRecord");
        hip_ok(hipStreamWaitEvent(fs.stream(), streams_->caller, 0), "hipStreamWaitEvent");
    }
    rethrowWorkerError();
    pumpMapping(pump_iters_per_frame);  // keep the map stream fed before this thread starts spinning on the tracker
    c10::hip::HIPStreamGuard guard(fs);
    processFrameImpl(i, cam, rgb_u8, depth_mm_i16);
}

void SLAMPipeline::ensureStreams() {
    if (!streams_) streams_.reset(new Streams(map_stream_kind, frame_stream_kind));
}

// ------------------------------------------------------------------ one map update (SLAMTrainCams :116-135)
double SLAMPipeline::beginUpdate(const Camera& cam) {
    initNewGaussiansFor(localframe_raycast_window.back(), cam);
    const double t = now_ms();
    localOptimizeBegin();
    return t;
}

void SLAMPipeline::finishUpdate() {
    removeRedundantGs();
    if (sample_method == "ours") checkKeyFrameError();   // slam_pipeline.cpp:130-131
}

// The stages behind the raycasts, start to finish on the current stream, with the reference's stage timers (host time on the
// calling thread: the map worker's are read by the frame thread only after flush()).
void SLAMPipeline::runUpdate(const Camera& cam) {
    const double s0 = now_ms();
    const double s1 = beginUpdate(cam);
    optimizeIterations(opt_pending_);
    const double s2 = now_ms();
    removeRedundantGs();
    const double s3 = now_ms();
    if (sample_method == "ours") checkKeyFrameError();   // slam_pipeline.cpp:130-131
    waitAllRaycasts();  // the next frame's fusion modifies the volume (results no iteration drew would still be in flight)
    times.initNewGaussians += s1 - s0; times.localOptimize += s2 - s1; times.removeGaussian += s3 - s2; times.checkError += now_ms() - s3;
}

void SLAMPipeline::keyframeStep() {
    // two batches: initNewGaussians only needs the window's views and starts while the keyframes' views render
    bookRaycastMs(buildCurrentViews(liveSource(), kTwoBatches));
    runUpdate(curr_cam);
}

// ------------------------------------------------------------------ tracking / mapping overlap (see slam_pipeline.hpp)
void SLAMPipeline::finishDeferredUpdate() {
    if (!prune_pending_) return;
    c10::hip::HIPStreamGuard guard(streams_->map);
    finishUpdate();
    prune_pending_ = false;
}

void SLAMPipeline::keyframeStepOverlapped() {
    ensureStreams();
    const hipStream_t frames = c10::hip::getCurrentHIPStream().stream();
    c10::hip::HIPStream& ms = streams_->map;
    // the previous update must be complete before its view set is replaced (host wait: B is idle afterwards)
    pumpMapping(opt_pending_);
    if (map_in_flight_) { hip_ok(hipEventSynchronize(streams_->map_done), "hipEventSynchronize"); map_in_flight_ = false; }
    hip_ok(hipEventRecord(streams_->frame_fused, frames), "hipEventRecord");
    hip_ok(hipStreamWaitEvent(ms.stream(), streams_->frame_fused, 0), "hipStreamWaitEvent");  // raycasts see frame i's volume
    {
        c10::hip::HIPStreamGuard guard(ms);
        finishDeferredUpdate();   // update k's prune (and loss records), before update k+1 reads the model and replaces the views
        buildCurrentViews(liveSource(), merge_keyframe_raycasts ? kOneBatch : kTwoBatches);
        if (async_raycasts) waitAllRaycasts();  // (this arrangement keeps its single map stream: the gate below covers them)
        hip_ok(hipEventRecord(streams_->raycasts, ms.stream()), "hipEventRecord");
        beginUpdate(curr_cam);
        map_update_open_ = true;
    }
    // a few iterations now, the rest a few at a time from the following processFrame calls: enqueueing all 20 at once keeps the
    // host (and with it the frame stream) busy for ~1 ms while the map stream only needs to stay ahead of the GPU
    pumpMapping(pump_iters_first);
    // the next frame's fusion must not modify the volume (or reuse the engine's free-view scratch) before the raycasts read it;
    // its tracking may overlap them: the wait sits in the engine's before-fusion hook
    main_engine->beforeNextFusion = [this] {
        hip_ok(hipStreamWaitEvent(c10::hip::getCurrentHIPStream().stream(), streams_->raycasts, 0), "hipStreamWaitEvent");
    };
}

// ------------------------------------------------------------------ mapping thread
// The classic SLAM split: this (the caller's) thread tracks and fuses, a worker thread owns the Gaussian model and runs each
// keyframe's map update start to finish on the map stream -- its host-side waits (mask counts in addGaussians / prune, 240
// kernel launches) no longer stall the frame stream at all.  Hand-over at keyframe i: wait for update i-10, record "frame i
// fused", snapshot the camera lists / poses the update reads (the frame thread keeps appending to the originals), wake the
// worker; the next frame's fusion waits until the update's raycasts have read the volume.
void SLAMPipeline::waitWorkerIdle(std::unique_lock<std::mutex>& lk) {
    cv_.wait(lk, [&] { return done_seq_ == job_seq_ || worker_error_; });
}

template <class Fill>
void SLAMPipeline::postJob(Fill&& fill) {
    std::unique_lock<std::mutex> lk(mu_);
    if (!worker_.joinable()) worker_ = std::thread([this, dev = (int)c10::hip::current_device()] { mapWorker(dev); });
    const double tw0 = now_ms();
    waitWorkerIdle(lk);
    handover_wait_ms_ = now_ms() - tw0;
    if (worker_error_) { lk.unlock(); rethrowWorkerError(); }
    fill(job_);   // (job_ is the frame thread's until job_seq_ moves)
    job_seq_++;
    job_post_ms_ = now_ms();
    cv_.notify_all();
}

void SLAMPipeline::keyframeStepThreaded() {
    ensureStreams();
    const hipStream_t frames = c10::hip::getCurrentHIPStream().stream();
    if (pipeline_raycasts && async_raycasts) {
        // This keyframe's free views, now, whether or not the worker has finished the previous update: the raycast stream starts
        // behind frame i's fusion, the map stream is the results' consumer (raycastCams), the worker adopts the set when it gets here.
        const hipStream_t rcs = raycastStream().s.stream();
        hip_ok(hipEventRecord(streams_->frame_fused, frames), "hipEventRecord");
        hip_ok(hipStreamWaitEvent(rcs, streams_->frame_fused, 0), "hipStreamWaitEvent");
        UpdateViews views;
        {
            c10::hip::HIPStreamGuard as_consumer(streams_->map);
            const Event* evs = streams_->job[job_parity_];
            job_parity_ ^= 1;
            const RaycastEvent job_events[2] = {evs[0], evs[1]};
            bookRaycastMs(buildViews(views, liveSource(), kTwoBatches, job_events));
        }
        hip_ok(hipEventRecord(streams_->raycasts, rcs), "hipEventRecord");
        postJob([&](MapJob& job) {
            job.curr_cam = curr_cam;
            job.views = std::move(views);
            job.views_ready = true;
        });
    } else {
        postJob([&](MapJob& job) {
            hip_ok(hipEventRecord(streams_->frame_fused, frames), "hipEventRecord");
            job.curr_cam = curr_cam;
            job.views_ready = false;
            job.window = localframe_cam_window;
            job.keyframes = keyframe_cam_list;
            job.poses = main_engine->camPoses;
            job.frame_id = curr_frame_id;
        });
    }
    // The next frame's fusion must not modify the volume (or reuse the engine's free-view scratch) before the update's raycasts
    // have read it -- but its TRACKING may run meanwhile: the wait is deferred to the engine's before-fusion hook of the next
    // ProcessFrame.  Two gates:
    if (pipeline_raycasts && async_raycasts) {
        // the raycasts are enqueued and their event recorded (above): a stream-side wait, no host wait
        main_engine->beforeNextFusion = [this] {
            hip_ok(hipStreamWaitEvent(c10::hip::getCurrentHIPStream().stream(), streams_->raycasts, 0), "hipStreamWaitEvent");
        };
    } else {
        // the WORKER enqueues them: first a host wait for it to have recorded the event (raycasts_seq_), then the stream-side wait
        main_engine->beforeNextFusion = [this, want = job_seq_] {
            {
                const double tw1 = now_ms();
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return raycasts_seq_ >= want || worker_error_; });
                gate_wait_ms_ = now_ms() - tw1;
            }
            rethrowWorkerError();
            hip_ok(hipStreamWaitEvent(c10::hip::getCurrentHIPStream().stream(), streams_->raycasts, 0), "hipStreamWaitEvent");
        };
    }
}

void SLAMPipeline::mapWorker(int device_index) {
    try {
        c10::hip::set_device((c10::DeviceIndex)device_index);
        c10::hip::HIPStream& ms = streams_->map;
        c10::hip::HIPStreamGuard guard(ms);
        int64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || job_seq_ > seen; });
                if (stop_) return;
                seen = job_seq_;
            }
            const double t_woke = now_ms();
            // job_ is stable until done_seq_ catches up (the frame thread waits for that before it writes the next one)
            hip_ok(hipStreamWaitEvent(ms.stream(), streams_->frame_fused, 0), "hipStreamWaitEvent");  // raycasts see frame i's volume
            if (job_.views_ready) {   // the frame thread has enqueued this update's views (and the gate event) already: adopt them
                adoptViews(std::move(job_.views));
            } else {
                const ViewSource snapshot{job_.window, job_.keyframes, job_.poses, job_.frame_id};
                bookRaycastMs(buildCurrentViews(snapshot, merge_keyframe_raycasts ? kOneBatch : kTwoBatches));
                // the gate of the next frame's fusion: the last raycast (on the raycast stream when they run beside the iterations)
                hip_ok(hipEventRecord(streams_->raycasts, async_raycasts && rc_ ? rc_->s.stream() : ms.stream()), "hipEventRecord");
            }
            { std::lock_guard<std::mutex> lk(mu_); raycasts_seq_ = seen; }
            cv_.notify_all();
            if (frame_report_ms >= 0.0 && now_ms() - job_post_ms_ > 1.0)
                fprintf(stderr, "[pipe] update %lld: raycasts enqueued %.3f ms after the hand-over (woke after %.3f)\n", (long long)seen,
                        now_ms() - job_post_ms_, t_woke - job_post_ms_);
            runUpdate(job_.curr_cam);
            // the wait for the map stream is the iterations' GPU time the enqueues ran ahead of: booked under localOptimize, which it
            // mostly is
            const double s0 = now_ms();
            hip_ok(hipStreamSynchronize(ms.stream()), "hipStreamSynchronize");
            times.localOptimize += now_ms() - s0;
            { std::lock_guard<std::mutex> lk(mu_); done_seq_ = seen; }
            cv_.notify_all();
        }
    } catch (...) {
        std::lock_guard<std::mutex> lk(mu_);
        worker_error_ = std::current_exception();
        cv_.notify_all();
    }
}

void SLAMPipeline::rethrowWorkerError() {
    std::exception_ptr e;
    { std::lock_guard<std::mutex> lk(mu_); e = worker_error_; worker_error_ = nullptr; }
    if (e) std::rethrow_exception(e);
}

// enqueue up to `count` pending optimise iterations on the map stream; closing the update records its completion event
void SLAMPipeline::pumpMapping(int count) {
    if (!map_update_open_) return;
    c10::hip::HIPStream& ms = streams_->map;
    c10::hip::HIPStreamGuard guard(ms);
    optimizeIterations(count);
    if (opt_pending_ == 0) {
        hip_ok(hipEventRecord(streams_->map_done, ms.stream()), "hipEventRecord");
        map_update_open_ = false;
        map_in_flight_ = true;
        prune_pending_ = true;
    }
}

void SLAMPipeline::flush() {
    if (main_engine) main_engine->beforeNextFusion = nullptr;  // no further frame: everything is joined below anyway (no engine: detached)
    if (worker_.joinable()) {
        { std::unique_lock<std::mutex> lk(mu_); waitWorkerIdle(lk); }
        rethrowWorkerError();
    }
    pumpMapping(opt_pending_);
    if (streams_) hip_ok(hipStreamSynchronize(streams_->frame.stream()), "hipStreamSynchronize");
    if (map_in_flight_) { hip_ok(hipEventSynchronize(streams_->map_done), "hipEventSynchronize"); map_in_flight_ = false; }
    if (prune_pending_) {
        finishDeferredUpdate();
        hip_ok(hipStreamSynchronize(streams_->map.stream()), "hipStreamSynchronize");
    }
}

SLAMPipeline::~SLAMPipeline() {
    if (tsdf_engine) {   // the engine outlives this pipeline: its hooks must not call into a dead object
        if (main_engine) main_engine->beforeNextFusion = nullptr;
        tsdf_engine->beforeShutdown = nullptr;
    }
    if (worker_.joinable()) {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        worker_.join();
    }
    // (each synchronises its streams, then destroys its events; the streams themselves belong to the process: make_stream)
    streams_.reset();
    rc_.reset();
}

void SLAMPipeline::SLAMTrainCams(std::vector<Camera>& cams, const std::vector<torch::Tensor>& rgb_u8,
                                 const std::vector<torch::Tensor>& depth_mm_i16) {
    for (size_t i = 0; i < cams.size(); i++) processFrame((int)i, cams[i], rgb_u8[i], depth_mm_i16[i]);
    flush();
}
