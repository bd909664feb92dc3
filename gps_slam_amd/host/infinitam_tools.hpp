// The TsdfFusion facade slam_trainer.cpp:26-29 and slam_pipeline.{h,cpp} program against:
//
//   ITMLib::ITMMainEngine / ITMLib::ITMBasicEngine<TVoxel, TIndex>   ITMLib/Core/ITMMainEngine.h, ITMBasicEngine.h:54-92
//   InfiniTAM::Engine::CLIEngine                                      slam/TsdfFusion/CLIEngine.{h,cpp}
//   createTsdfEngine(const DatasetReader&, config)                    slam/InfiniTAM_tools.{h,cpp}
//
// with the reference's names, constructor / method signatures and member names, over TsdfEngine (tsdf_engine.hpp) and the
// C-ABI.  What differs, and why: `config` is gpsh::Config instead of YAML::Node and DatasetReader is the plain struct below
// instead of the OpenCV/yaml-cpp reader of include/dataset_reader.h (I/O, out of scope); CLIEngine keeps the whole sequence in
// PINNED host memory and, knowing the next frame, uploads it on a copy stream while the current one is processed (the
// reference's UpdateView is a blocking cudaMemcpy per frame, ITMViewBuilder_CUDA.cu:61-62) -- every frame's 6 bytes per
// pixel still cross PCIe inside the frame loop.
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "config_fields.hpp"
#include "raw_gs_param.hpp"
#include "tsdf_engine.hpp"

namespace ITMLib {

// ITMLib/Core/ITMMainEngine.h:39-88 (the members GPS-SLAM calls)
class ITMMainEngine : public ITMMainEngineTypes {   // (GetImageType, InfiniTAM_IMAGE_*: tsdf_engine.hpp)
public:
    virtual ~ITMMainEngine() {}
    virtual void GetImage(ITMUChar4Image* out, GetImageType getImageType, ORUtils::SE3Pose* pose = NULL,
                          ITMIntrinsics* intrinsics = NULL) = 0;
    virtual ITMTrackingState* GetTrackingState(void) = 0;
    virtual ITMTrackingState::TrackingResult ProcessFrame(ITMUChar4Image* rgbImage, ITMShortImage* rawDepthImage,
                                                          ITMIMUMeasurement* imuMeasurement = NULL) = 0;
    virtual void SaveSceneToMesh(const char* fileName) = 0;
    virtual void SaveToFile(const std::string& saveOutputDirectory) = 0;
    virtual void LoadFromFile(const std::string& saveInputDirectory) = 0;
    virtual Vector2i GetImageSize(void) const = 0;
    virtual void turnOnTracking() = 0;
    virtual void turnOffTracking() = 0;
};

// ITMLib/Core/ITMBasicEngine.h:21-115.  TVoxel / TIndex select the storage layouts; the one combination GPS-SLAM
// instantiates (ITMVoxel_s_rgb + ITMVoxelBlockHash, ITMLibDefines.h:18-25) is what the kernels implement.
template <typename TVoxel, typename TIndex>
class ITMBasicEngine : public ITMMainEngine, public TsdfEngine {
    static_assert(std::is_same<TVoxel, ITMVoxel_s_rgb>::value && std::is_same<TIndex, ITMVoxelBlockHash>::value,
                  "the gfx950 kernels implement ITMVoxel_s_rgb voxels in an ITMVoxelBlockHash index");

public:
    // ITMBasicEngine.h:104: imgSize_d = (-1,-1) means "same as rgb"
    ITMBasicEngine(const ITMLibSettings* settings, const ITMRGBDCalib& calib, Vector2i imgSize_rgb,
                   Vector2i imgSize_d = Vector2i(-1, -1))
        : TsdfEngine(imgSize_d.x == -1 ? imgSize_rgb.x : imgSize_d.x, imgSize_d.x == -1 ? imgSize_rgb.y : imgSize_d.y,
                     calib.intrinsics_d.projectionParamsSimple.fx, calib.intrinsics_d.projectionParamsSimple.fy,
                     calib.intrinsics_d.projectionParamsSimple.px, calib.intrinsics_d.projectionParamsSimple.py,
                     settings->sceneParams.voxelSize, settings->sceneParams.mu, settings->sceneParams.viewFrustum_min,
                     settings->sceneParams.viewFrustum_max, settings->noTotalEntries_blocks, settings->noBuckets,
                     settings->excessListSize) {
        intrinsics_d = calib.intrinsics_d;
        // one camera with the standard calibration (what createTsdfEngine passes): the engine as it always ran.  Anything else --
        // another colour size, colour intrinsics or pose, a disparity calibration -- is the full ITMRGBDCalib (setCalibration)
        const bool sameSize = imgSize_d.x == -1 || (imgSize_d.x == imgSize_rgb.x && imgSize_d.y == imgSize_rgb.y);
        const ITMExtrinsics identity;
        const bool oneCamera = sameSize && std::memcmp(calib.trafo_rgb_to_depth.calib.m, identity.calib.m, 64) == 0 &&
                               std::memcmp(&calib.intrinsics_rgb.projectionParamsSimple.all, &calib.intrinsics_d.projectionParamsSimple.all, 16) == 0;
        if (!oneCamera || !calib.disparityCalib.isStandard()) {
            ITMRGBDCalib c = calib;
            c.intrinsics_rgb.imgSize = imgSize_rgb;
            c.intrinsics_d.imgSize = GetImageSize();
            setCalibration(c);
        }
    }

    ITMTrackingState* GetTrackingState(void) override { return TsdfEngine::GetTrackingState(); }
    ITMTrackingState::TrackingResult ProcessFrame(ITMUChar4Image* rgbImage, ITMShortImage* rawDepthImage,
                                                  ITMIMUMeasurement* imuMeasurement = NULL) override {
        TORCH_CHECK(imuMeasurement == NULL, "IMU measurements are not used by GPS-SLAM");
        return TsdfEngine::ProcessFrame(rgbImage, rawDepthImage)->trackerResult;
    }
    using TsdfEngine::ProcessFrame;  // + the tensor overload for frames that already live in HBM
    void SaveSceneToMesh(const char* fileName) override { (void)TsdfEngine::SaveSceneToMesh(fileName); }
    void SaveToFile(const std::string& d) override { TsdfEngine::SaveToFile(d); }
    void LoadFromFile(const std::string& d) override { TsdfEngine::LoadFromFile(d); }
    Vector2i GetImageSize(void) const override { return Vector2i(state().width, state().height); }
    void GetImage(ITMUChar4Image* out, ITMMainEngine::GetImageType getImageType, ORUtils::SE3Pose* pose = NULL,
                  ITMIntrinsics* intrinsics = NULL) override {
        TsdfEngine::GetImage(out, getImageType, pose, intrinsics);
    }
    void turnOnTracking() override { TsdfEngine::turnOnTracking(); }
    void turnOffTracking() override { TsdfEngine::turnOffTracking(); }
};

}  // namespace ITMLib

namespace InfiniTAM {
namespace Engine {

// slam/TsdfFusion/CLIEngine.h:14-66: process-wide singleton that owns the input sequence and feeds it to the main engine
class CLIEngine {
    static CLIEngine* instance;
    std::vector<ITMUChar4Image*> rgb_images;
    std::vector<ITMShortImage*> depth_images;
    ITMLib::ITMMainEngine* mainEngine = nullptr;

public:
    static CLIEngine* Instance(void) {
        if (instance == NULL) instance = new CLIEngine();
        return instance;
    }
    float processedTime = 0.f;
    int currentFrameNo = 0;  // (private in the reference; slam_pipeline.cpp:77 asserts on it, which only compiles under NDEBUG)

    void Initialise(std::vector<ITMUChar4Image*> rgb_images, std::vector<ITMShortImage*> depth_images,
                    ITMLib::ITMMainEngine* mainEngine);
    void Shutdown();
    void Run();
    bool ProcessFrame();
    // call on the stream of the LAST reader of the frame ProcessFrame() just consumed (e.g. after deriving the camera's float
    // image from currentRgb()): the staging slot is not overwritten by a later upload before that reader has run
    void markConsumed();
    Vector2i GetDepthSize() { return depth_images[0]->noDims; }
    Vector2i GetRGBSize() { return rgb_images[0]->noDims; }
    ITMLib::ITMMainEngine* getMainEngine() { return mainEngine; }

    // Upload pipelining (see the file comment).  prefetch = false reproduces the reference's schedule: the frame's upload is
    // enqueued on the frame's own stream right before its kernels.
    bool prefetch = true;
    int64_t uploadedBytes = 0;
    // called first thing by Shutdown(): a SLAMPipeline attached with setTsdfEngine() flushes its map worker and drops its raw
    // pointers into this engine (and the engine's beforeNextFusion hook that captures the pipeline) before the engine is freed
    // (round-5 advisor finding: bench.Scene.close() shuts the engine down while the pipeline is still alive)
    std::function<void()> beforeShutdown;
    bool ownsInputs = false;   // Shutdown() deletes the images and the engine (set by createTsdfEngine, which allocated them)

private:
    void upload(int frame);  // pinned host images of `frame` -> staging slot frame % 3, on the copy stream
    struct Staging;
    std::shared_ptr<Staging> staging_;
};

}  // namespace Engine
}  // namespace InfiniTAM

// include/dataset_reader.h:111-169, 171-230: what createTsdfEngine reads from the reader -- image size, pinhole intrinsics
// and the training cameras (image float [H,W,3] in [0,1], depth float [H,W,1] metres, c2w [4,4]), on the host.  createTsdfEngine also
// takes the image as uint8 [H,W,3] and the depth as (u)int16 millimetres -- what the dataset's files hold -- with the same bytes out
struct DatasetReader {
    int width = 0, height = 0;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
    float scene_scale = 1.1f * 3.0f;   // dataset_reader.cpp:231: 1.1 x READER.scene_scale (what slam_trainer.cpp:39 hands the pipeline)
    float depth_scale = 1000.0f;       // READER.depth_scale: raw depth units per metre (for whoever fills train_vec from files)
    std::vector<Camera> train_vec;

    // The READER node (dataset_reader.cpp:217-231, :342; N = YAML::Node or gpsh::Node): intrinsics, image_shape, scene_scale,
    // depth_scale.  downscale_factor other than 1 throws (resizing images is reader I/O: DESIGN.md section 8); the paths and the
    // frame range are for whoever reads the files -- filling train_vec stays the caller's job.
    template <class N> void loadConfig(const N& reader_node);
};

// PIPE.TSDF as createTsdfEngine reads it (InfiniTAM_tools.cpp:48-62) + the table sizes this project made runtime parameters
// (-1: ITMLibSettings' defaults)
struct TsdfConfig {
    float voxel_size = 0.005f, trunc_dist = 0.02f, viewFrustum_min = 0.2f, viewFrustum_max = 10.0f;
    bool use_gt_pose = true;
    int sdf_local_block_num = -1, sdf_bucket_num = -1, sdf_excess_list_size = -1;
    std::string failure_mode = "ignore";   // ignore | stop_integration | relocalise (ITMLibSettings::behaviourOnFailure)
    bool use_approximate_raycast = false;  // ITMLibSettings::useApproximateRaycast
    bool use_bilateral_filter = false;     // ITMLibSettings::useBilateralFilter
    template <class V> void configFields(V& v) {   // THE list of createTsdfEngine's keys (config_fields.hpp)
        v.f("voxel_size", voxel_size);
        v.f("trunc_dist", trunc_dist);
        v.f("viewFrustum_min", viewFrustum_min);
        v.f("viewFrustum_max", viewFrustum_max);
        v.b("use_gt_pose", use_gt_pose);
        v.i("sdf_local_block_num", sdf_local_block_num, gpsh::kOptional);
        v.i("sdf_bucket_num", sdf_bucket_num, gpsh::kOptional);
        v.i("sdf_excess_list_size", sdf_excess_list_size, gpsh::kOptional);
        v.s("failure_mode", failure_mode, gpsh::kOptional);
        v.b("use_approximate_raycast", use_approximate_raycast, gpsh::kOptional);
        v.b("use_bilateral_filter", use_bilateral_filter, gpsh::kOptional);
        for (const char* k : {"load_images", "saved_mesh", "saved_engine", "saved_images"}) v.ignored(k);   // (the pipeline's: SLAMPipeline::loadConfig)
    }
};

// slam/InfiniTAM_tools.cpp:3-67.  config keys: voxel_size, trunc_dist, viewFrustum_min, viewFrustum_max, use_gt_pose (0/1).
// Image conversion as the reference: rgb = (image * 255).toType(uint8), alpha 255 (cv_utils.cpp:57-76, 221-246);
// depth = round-half-even(depth * 1000) saturated to uint16, stored in shorts (cv_utils.cpp:79-101, 248-268).
InfiniTAM::Engine::CLIEngine* createTsdfEngine(const DatasetReader& data_reader, const gpsh::Config& config);
// the reference's signature: the PIPE.TSDF node (N = YAML::Node or gpsh::Node).  Its five keys are required; a missing one throws
// before an image is converted.
template <class N>
InfiniTAM::Engine::CLIEngine* createTsdfEngine(const DatasetReader& data_reader, const N& tsdf_node) {
    TsdfConfig t;
    return createTsdfEngine(data_reader, gpsh::flattenNode(tsdf_node, "PIPE.TSDF", [&](auto& v) { t.configFields(v); }));
}

// THE list of READER keys (dataset_reader.cpp:217-231, :342) that DatasetReader::loadConfig reads, and those it leaves to whoever
// reads the files
struct ReaderConfig {
    std::vector<float> intrinsics;
    std::vector<int> image_shape;
    float downscale_factor = 1.0f, scene_scale = 1.0f, depth_scale = 1000.0f;
    template <class V> void configFields(V& v) {
        v.fv("intrinsics", intrinsics);
        v.iv("image_shape", image_shape);
        v.f("downscale_factor", downscale_factor);
        v.f("scene_scale", scene_scale);
        v.f("depth_scale", depth_scale);
        for (const char* k : {"input_dir", "image_path", "pose_path", "depth_path", "pcd_name", "start_frame", "end_frame", "frame_step",
                              "test_split_interval"})
            v.ignored(k);
    }
};

template <class N>
void DatasetReader::loadConfig(const N& reader_node) {
    const std::string path = gpsh::nodePath(reader_node, "READER");
    ReaderConfig r;
    gpsh::rejectUnknownKeys(reader_node, [&](auto& v) { r.configFields(v); });
    gpsh::NodeAssigner<N> assign{reader_node, path};
    r.configFields(assign);
    if (r.intrinsics.size() < 4) throw gpsh::ConfigError(path + ".intrinsics: four numbers are needed (fx, fy, cx, cy)");
    if (r.image_shape.size() < 2) throw gpsh::ConfigError(path + ".image_shape: two numbers are needed (width, height)");
    if (r.downscale_factor != 1.0f) throw gpsh::ConfigError(path + ".downscale_factor: only 1 is supported (images are not resized here)");
    fx = r.intrinsics[0]; fy = r.intrinsics[1]; cx = r.intrinsics[2]; cy = r.intrinsics[3];
    width = r.image_shape[0]; height = r.image_shape[1];
    scene_scale = 1.1f * r.scene_scale;
    depth_scale = r.depth_scale;
}
