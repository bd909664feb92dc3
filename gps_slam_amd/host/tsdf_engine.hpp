// The TSDF engine surface SLAMPipeline drives (slam/slam_pipeline.cpp:69-83, 362-415; slam/InfiniTAM_tools.cpp:3-67;
// ITMLib/Core/ITMBasicEngine.{h,tpp}) on the C-ABI, in two layers:
//
//   TsdfEngine                                 the engine proper: owns the device buffers (through libtorch, where the reference
//                                              uses ORUtils::MemoryBlock), fills gps_tsdf_state once, afterwards only passes
//                                              pointers; tensor-based ProcessFrame for callers whose frames are already in HBM
//   ITMLib::ITMBasicEngine<TVoxel, TIndex>     the reference's class template over it (infinitam_tools.hpp): same constructor,
//     : ITMLib::ITMMainEngine, TsdfEngine      ProcessFrame(ITMUChar4Image*, ITMShortImage*, ITMIMUMeasurement*), runRaycast(
//                                              SE3Pose*, ITMIntrinsics*), camPoses / camIntrincs / gtC2wPoses, so that code
//                                              written against ITMBasicEngine.h:54-92 (slam_pipeline.cpp's dynamic_casts) reads as is
//   InfiniTAM::Engine::CLIEngine, createTsdfEngine    infinitam_tools.hpp
//
// Method and member names follow the reference: ProcessFrame, runRaycast, GetFreeImage, GetFreeVertex, getVoxelSize,
// GetTrackingState()->pose_d->GetInvM(), camPoses, camIntrincs, gtC2wPoses, turnOffTracking, SaveToFile, LoadFromFile,
// SaveSceneToMesh.
#pragma once
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <memory>
#include <functional>
#include <mutex>

#include <map>

#include "gps_host_common.hpp"
#include "geom_eval.hpp"
#include "relocaliser.hpp"

enum MemoryDeviceType { MEMORYDEVICE_CPU, MEMORYDEVICE_CUDA };

namespace ORUtils {

template <class T> struct Vector2 {  // ORUtils/Vector.h (the two fields the engine surface uses)
    T x, y;
    Vector2() : x(0), y(0) {}
    Vector2(T x_, T y_) : x(x_), y(y_) {}
    T width() const { return x; }
    T height() const { return y; }
};

// ORUtils/SE3Pose.h as used here: SetInvM(c2w) + Coerce() -> GetM / GetInvM (ORUtils column-major float[16])
class SE3Pose {
public:
    SE3Pose() { for (int i = 0; i < 16; i++) M_[i] = invM_[i] = (i % 5 == 0) ? 1.f : 0.f; }
    void SetInvM(const float* c2w_row_major) { gpsh::check(gps_pose_from_c2w(c2w_row_major, M_, invM_), "gps_pose_from_c2w"); }
    void SetBoth(const float* M, const float* invM) { for (int i = 0; i < 16; i++) { M_[i] = M[i]; invM_[i] = invM[i]; } }
    void Coerce() {}  // done by gps_pose_from_c2w
    const float* GetM() const { return M_; }
    const float* GetInvM() const { return invM_; }

private:
    float M_[16], invM_[16];
};

// ORUtils/Image.h + MemoryBlock.h as the pipeline uses them: an image with a host copy (pinned, so that UpdateView's
// CPU->device transfer can be asynchronous), a device copy, or both; GetData(MEMORYDEVICE_CUDA) is a pointer
// torch::from_blob can wrap (src/cv_utils.cpp:324-336).  Storage is torch tensors.
template <class T>
class Image {
public:
    Vector2<int> noDims;
    Image(int w, int h, torch::Tensor device_storage) : noDims(w, h), dev_(device_storage) {}
    // ORUtils::Image(noDims, allocate_CPU, allocate_CUDA) (Image.h:27-33)
    Image(Vector2<int> dims, bool allocate_CPU, bool allocate_CUDA, torch::Device device = torch::kCUDA) : noDims(dims) {
        const int64_t bytes = (int64_t)dims.x * dims.y * (int64_t)sizeof(T);
        // (empty + memset, not torch::zeros: the fill of a megabyte is a parallel region of torch's intra-op pool -- one thread per
        // core the machine SHOWS, each spinning for a while afterwards; two such regions per frame of a sequence exhaust a
        // container's CPU quota and the kernel then freezes every thread of the process, the tracking thread included, until the
        // end of the 100 ms accounting period: LABBOOK section 14, tools/probe/early_stall.py)
        if (allocate_CPU) {
            host_ = torch::empty({bytes}, torch::TensorOptions().dtype(torch::kUInt8).pinned_memory(true));
            std::memset(host_.data_ptr(), 0, (size_t)bytes);
        }
        if (allocate_CUDA) dev_ = torch::zeros({bytes}, torch::TensorOptions().dtype(torch::kUInt8).device(device));
    }
    T* GetData(MemoryDeviceType t) const {
        const torch::Tensor& s = t == MEMORYDEVICE_CUDA ? dev_ : host_;
        TORCH_CHECK(s.defined(), "Image: no ", t == MEMORYDEVICE_CUDA ? "device" : "host", " copy allocated");
        return reinterpret_cast<T*>(s.data_ptr());
    }
    bool isAllocated_CPU() const { return host_.defined(); }
    bool isAllocated_CUDA() const { return dev_.defined(); }
    size_t dataSize() const { return (size_t)noDims.x * noDims.y; }
    const torch::Tensor& tensor() const { return dev_; }         // device storage
    const torch::Tensor& host_tensor() const { return host_; }   // pinned host storage (raw bytes)

private:
    torch::Tensor dev_, host_;
};

}  // namespace ORUtils

struct Vector4u { unsigned char x, y, z, w; };
struct Vector4f { float x, y, z, w; };
typedef ORUtils::Vector2<int> Vector2i;
typedef ORUtils::Image<Vector4u> ITMUChar4Image;
typedef ORUtils::Image<Vector4f> ITMFloat4Image;
typedef ORUtils::Image<short> ITMShortImage;

// ITMLib/Objects/Tracking/ITMTrackingState.h:20-27, 38
struct ITMTrackingState {
    enum TrackingResult { TRACKING_GOOD = 2, TRACKING_POOR = 1, TRACKING_FAILED = 0 };
    ORUtils::SE3Pose* pose_d;
    TrackingResult trackerResult = TRACKING_GOOD;
};

namespace ITMLib {

// ITMLib/Objects/Camera/ITMIntrinsics.h:17-63
class ITMIntrinsics {
public:
    struct ProjectionParamsSimple { Vector4f all; float fx, fy, px, py; } projectionParamsSimple;
    Vector2i imgSize;
    void SetFrom(int width, int height, float fx, float fy, float cx, float cy) {
        imgSize = Vector2i(width, height);
        projectionParamsSimple.fx = fx; projectionParamsSimple.fy = fy; projectionParamsSimple.px = cx; projectionParamsSimple.py = cy;
        projectionParamsSimple.all = Vector4f{fx, fy, cx, cy};
    }
    ITMIntrinsics() { SetFrom(640, 480, 580.f, 580.f, 320.f, 240.f); }  // ITMIntrinsics.cpp:11-15
};

struct Vector2f { float x, y; };
struct Matrix4f { float m[16]; };   // ORUtils layout m[col * 4 + row]

// ITMLib/Objects/Camera/ITMDisparityCalib.h: raw values -> depth, 8 b fx / (a - d) (Kinect) or a d + b (affine)
class ITMDisparityCalib {
public:
    enum TrafoType { TRAFO_KINECT, TRAFO_AFFINE };   // == gps_depth_calib_type
    ITMDisparityCalib() { SetStandard(); }
    const Vector2f& GetParams() const { return params; }
    TrafoType GetType() const { return type; }
    void SetFrom(float a, float b, TrafoType _type) {   // "both zero" is the standard calibration (:55-64)
        if (a != 0.0f || b != 0.0f) { params.x = a; params.y = b; type = _type; }
        else SetStandard();
    }
    void SetStandard() { SetFrom(1.0f / 1000.0f, 0.0f, TRAFO_AFFINE); }   // millimetres
    bool isStandard() const { return type == TRAFO_AFFINE && params.x == 1.0f / 1000.0f && params.y == 0.0f; }

private:
    TrafoType type;
    Vector2f params;
};

// ITMLib/Objects/Camera/ITMExtrinsics.h: calib takes points of the colour camera to the depth camera; calib_inv as :28-40 build it
// (the transpose of the rotation, and -(R^T t) as three subtractions from 0, in float)
class ITMExtrinsics {
public:
    Matrix4f calib, calib_inv;
    void SetFrom(const Matrix4f& src) {
        calib = src;
        for (int i = 0; i < 16; i++) calib_inv.m[i] = (i % 5 == 0) ? 1.0f : 0.0f;
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) calib_inv.m[r + 4 * c] = calib.m[c + 4 * r];
        for (int r = 0; r < 3; ++r) {
            volatile float dest = 0.0f;   // (volatile: no fused multiply-subtract, whatever the host compiler's flags)
            for (int c = 0; c < 3; ++c) { volatile float p = calib.m[c + 4 * r] * calib.m[c + 4 * 3]; dest = dest - p; }
            calib_inv.m[r + 4 * 3] = dest;
        }
    }
    ITMExtrinsics() {
        Matrix4f m;
        for (int i = 0; i < 16; i++) m.m[i] = (i % 5 == 0) ? 1.0f : 0.0f;
        SetFrom(m);
    }
};

// ITMLib/Objects/Camera/ITMRGBDCalib.h
class ITMRGBDCalib {
public:
    ITMIntrinsics intrinsics_rgb, intrinsics_d;
    ITMExtrinsics trafo_rgb_to_depth;
    ITMDisparityCalib disparityCalib;
};

// ITMLib/Objects/Camera/ITMCalibIO.cpp: the four-part calib.txt (colour intrinsics, depth intrinsics, extrinsics, disparity
// calibration), read and written in the reference's text format
inline bool readIntrinsics(std::istream& src, ITMIntrinsics& dest) {
    int width, height;
    float f[2], c[2];
    src >> width >> height >> f[0] >> f[1] >> c[0] >> c[1];
    if (src.fail()) return false;
    dest.SetFrom(width, height, f[0], f[1], c[0], c[1]);
    return true;
}
inline bool readExtrinsics(std::istream& src, ITMExtrinsics& dest) {
    Matrix4f m;
    for (int r = 0; r < 3; r++) src >> m.m[r] >> m.m[4 + r] >> m.m[8 + r] >> m.m[12 + r];
    m.m[3] = m.m[7] = m.m[11] = 0.0f; m.m[15] = 1.0f;
    if (src.fail()) return false;
    dest.SetFrom(m);
    return true;
}
inline bool readDisparityCalib(std::istream& src, ITMDisparityCalib& dest) {
    std::string word;
    src >> word;
    if (src.fail()) return false;
    ITMDisparityCalib::TrafoType type = ITMDisparityCalib::TRAFO_KINECT;
    float a, b;
    if (word == "kinect") src >> a;
    else if (word == "affine") { type = ITMDisparityCalib::TRAFO_AFFINE; src >> a; }
    else {
        std::stringstream wordstream(word);
        wordstream >> a;
        if (wordstream.fail()) return false;
    }
    src >> b;
    if (src.fail()) return false;
    dest.SetFrom(a, b, type);   // (both zero: the standard calibration)
    return true;
}
inline bool readRGBDCalib(std::istream& src, ITMRGBDCalib& dest) {
    return readIntrinsics(src, dest.intrinsics_rgb) && readIntrinsics(src, dest.intrinsics_d) &&
           readExtrinsics(src, dest.trafo_rgb_to_depth) && readDisparityCalib(src, dest.disparityCalib);
}
inline bool readRGBDCalib(const char* fileName, ITMRGBDCalib& dest) {
    std::ifstream f(fileName);
    return readRGBDCalib(f, dest);
}
inline void writeIntrinsics(std::ostream& dest, const ITMIntrinsics& src) {
    dest << src.imgSize.x << ' ' << src.imgSize.y << '\n';
    dest << src.projectionParamsSimple.fx << ' ' << src.projectionParamsSimple.fy << '\n';
    dest << src.projectionParamsSimple.px << ' ' << src.projectionParamsSimple.py << '\n';
}
inline void writeExtrinsics(std::ostream& dest, const ITMExtrinsics& src) {
    const float* m = src.calib.m;
    for (int r = 0; r < 3; r++) dest << m[r] << ' ' << m[4 + r] << ' ' << m[8 + r] << ' ' << m[12 + r] << '\n';
}
inline void writeDisparityCalib(std::ostream& dest, const ITMDisparityCalib& src) {
    if (src.GetType() == ITMDisparityCalib::TRAFO_AFFINE) dest << "affine ";
    dest << src.GetParams().x << ' ' << src.GetParams().y << '\n';
}
inline void writeRGBDCalib(std::ostream& dest, const ITMRGBDCalib& src) {
    writeIntrinsics(dest, src.intrinsics_rgb);
    dest << '\n';
    writeIntrinsics(dest, src.intrinsics_d);
    dest << '\n';
    writeExtrinsics(dest, src.trafo_rgb_to_depth);
    dest << '\n';
    writeDisparityCalib(dest, src.disparityCalib);
}
inline void writeRGBDCalib(const char* fileName, const ITMRGBDCalib& src) {
    std::ofstream f(fileName);
    writeRGBDCalib(f, src);
}

// ITMLib/Utils/ITMSceneParams.h + ITMLibSettings.{h,cpp} (the fields createTsdfEngine sets, reference defaults :10)
struct ITMSceneParams { float voxelSize = 0.005f, mu = 0.02f, viewFrustum_min = 0.2f, viewFrustum_max = 3.0f; int maxW = 100; };
class ITMLibSettings {
public:
    ITMSceneParams sceneParams;
    // hash table / voxel block array capacities (ITMVoxelBlockHash.h:18-22; runtime parameters here)
    int noTotalEntries_blocks = 0x40000, noBuckets = 0x100000, excessListSize = 0x20000;
    // ITMLibSettings.h:24-29; the default is the reference's (ITMLibSettings.cpp:42)
    enum FailureMode { FAILUREMODE_RELOCALISE, FAILUREMODE_IGNORE, FAILUREMODE_STOP_INTEGRATION };
    FailureMode behaviourOnFailure = FAILUREMODE_IGNORE;
    // ITMLibSettings.h:45; the default is the reference's (ITMLibSettings.cpp:36).  TSDF.use_approximate_raycast of the configs.
    bool useApproximateRaycast = false;
    // ITMLibSettings.h:47; the default is the reference's (ITMLibSettings.cpp:39).  TSDF.use_bilateral_filter of the configs.
    bool useBilateralFilter = false;
    // TSDF.failure_mode of the configs: ignore | stop_integration | relocalise (anything else throws)
    static FailureMode failureModeFromString(const std::string& name) {
        if (name == "ignore") return FAILUREMODE_IGNORE;
        if (name == "stop_integration") return FAILUREMODE_STOP_INTEGRATION;
        if (name == "relocalise") return FAILUREMODE_RELOCALISE;
        throw std::invalid_argument("failure_mode: '" + name + "' is not one of ignore, stop_integration, relocalise");
    }
};

// What ITMBasicEngine::ProcessFrame does with a tracking verdict (ITMBasicEngine.tpp:286-366), as one pure function.
//   trackerVerdict       trackingState->trackerResult of the frame's TrackCamera
//   addedKeyframe        the relocaliser harvested this frame (known without asking it whenever it matters: a frame is only
//                        offered for harvesting when its verdict is GOOD, and only relocalised when it is FAILED)
//   relocalised          false: the evaluation after the frame's first TrackCamera.  true: the evaluation after the second
//                        TrackCamera of a frame that relocalised (:329-331) -- the relocaliser stage is over, count is the 10 it set
// -> result              the verdict the engine acts on and returns (:286-300)
//    useRelocaliser      the frame goes through Relocaliser::ProcessFrame (:304-314), with `harvest` as harvestKeyframes
//    relocalise          restart from the nearest keyframe's pose: rebuild the visible list, raycast, track again (:317-332), then
//                        evaluate again with relocalised = true
//    fuse                ITMDenseMapper::ProcessFrame (:338-347)
//    refreshAndRaycast   UpdateVisibleList when the frame did not fuse, then Prepare (:349-364); false: the old pose comes back (:366)
//    relocalisationCount the counter afterwards
struct FailureDecision {
    ITMTrackingState::TrackingResult result;
    bool useRelocaliser, harvest, relocalise, fuse, refreshAndRaycast;
    int relocalisationCount;
};
inline FailureDecision decideOnTrackingResult(ITMLibSettings::FailureMode mode, ITMTrackingState::TrackingResult trackerVerdict,
                                              bool addedKeyframe, int relocalisationCount, bool trackingInitialised, bool fusionActive,
                                              bool relocalised = false) {
    FailureDecision d{ITMTrackingState::TRACKING_GOOD, false, false, false, false, false, relocalisationCount};
    if (mode == ITMLibSettings::FAILUREMODE_RELOCALISE) d.result = trackerVerdict;
    else if (mode == ITMLibSettings::FAILUREMODE_STOP_INTEGRATION)
        d.result = trackerVerdict != ITMTrackingState::TRACKING_FAILED ? trackerVerdict : ITMTrackingState::TRACKING_POOR;
    if (mode == ITMLibSettings::FAILUREMODE_RELOCALISE && !relocalised) {
        if (d.result == ITMTrackingState::TRACKING_GOOD && d.relocalisationCount > 0) d.relocalisationCount--;
        d.useRelocaliser = true;
        d.harvest = d.result == ITMTrackingState::TRACKING_GOOD && d.relocalisationCount == 0;
        if (!addedKeyframe && d.result == ITMTrackingState::TRACKING_FAILED) {
            d.relocalise = true;
            d.relocalisationCount = 10;
            return d;   // the tail is decided by the second TrackCamera's verdict
        }
    }
    d.fuse = (d.result == ITMTrackingState::TRACKING_GOOD || !trackingInitialised) && fusionActive && d.relocalisationCount == 0;
    d.refreshAndRaycast = d.result == ITMTrackingState::TRACKING_GOOD || d.result == ITMTrackingState::TRACKING_POOR;
    return d;
}

// ITMLib/Core/ITMMainEngine.h:50-63: the images GetImage can be asked for (ITMMainEngine derives from this, so that
// ITMMainEngine::GetImageType and ITMMainEngine::InfiniTAM_IMAGE_* read as in the reference)
struct ITMMainEngineTypes {
    enum GetImageType {
        InfiniTAM_IMAGE_ORIGINAL_RGB,
        InfiniTAM_IMAGE_ORIGINAL_DEPTH,
        InfiniTAM_IMAGE_SCENERAYCAST,
        InfiniTAM_IMAGE_COLOUR_FROM_VOLUME,
        InfiniTAM_IMAGE_COLOUR_FROM_NORMAL,
        InfiniTAM_IMAGE_COLOUR_FROM_CONFIDENCE,
        InfiniTAM_IMAGE_FREECAMERA_SHADED,
        InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME,
        InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL,
        InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_CONFIDENCE,
        InfiniTAM_IMAGE_UNKNOWN
    };
};

// What ITMBasicEngine::GetImage does for an image type (ITMBasicEngine.tpp:400-497), as one pure function of the type, the age of
// the point cloud and the relocalisation countdown.
//   renderType   the RenderImage pass (gps_render_type), -1: none
//   rays         the ray image that pass reads: the last full cast (age_pointCloud <= 0), the forward projection (otherwise), or a
//                fresh cast of the free view that leaves the visible list alone
//   out          where the caller's image comes from.  OUT_KF_RAYCAST: the live types while relocalisationCount != 0 -- the live
//                image is rendered all the same, and the caller gets kfRaycast, which this reference never writes (all zeros).
//                OUT_CLEARED: InfiniTAM_IMAGE_UNKNOWN, the cleared image
struct GetImageDecision {
    enum RaySource { RAYS_NONE, RAYS_LIVE_RAYCAST, RAYS_FORWARD_PROJECTION, RAYS_FREE_RAYCAST };
    enum OutSource { OUT_CLEARED, OUT_RGB, OUT_DEPTH_COLOUR, OUT_LIVE_RENDER, OUT_KF_RAYCAST, OUT_FREE_RENDER };
    int renderType;
    RaySource rays;
    OutSource out;
};
inline GetImageDecision decideOnGetImage(ITMMainEngineTypes::GetImageType type, int age_pointCloud, int relocalisationCount) {
    typedef ITMMainEngineTypes T;
    GetImageDecision d{-1, GetImageDecision::RAYS_NONE, GetImageDecision::OUT_CLEARED};
    switch (type) {
    case T::InfiniTAM_IMAGE_ORIGINAL_RGB: d.out = GetImageDecision::OUT_RGB; break;
    case T::InfiniTAM_IMAGE_ORIGINAL_DEPTH: d.out = GetImageDecision::OUT_DEPTH_COLOUR; break;
    case T::InfiniTAM_IMAGE_SCENERAYCAST:
    case T::InfiniTAM_IMAGE_COLOUR_FROM_VOLUME:
    case T::InfiniTAM_IMAGE_COLOUR_FROM_NORMAL:
    case T::InfiniTAM_IMAGE_COLOUR_FROM_CONFIDENCE:
        d.rays = age_pointCloud <= 0 ? GetImageDecision::RAYS_LIVE_RAYCAST : GetImageDecision::RAYS_FORWARD_PROJECTION;
        d.renderType = type == T::InfiniTAM_IMAGE_COLOUR_FROM_CONFIDENCE ? GPS_RENDER_COLOUR_FROM_CONFIDENCE
                       : type == T::InfiniTAM_IMAGE_COLOUR_FROM_NORMAL   ? GPS_RENDER_COLOUR_FROM_NORMAL
                       : type == T::InfiniTAM_IMAGE_COLOUR_FROM_VOLUME   ? GPS_RENDER_COLOUR_FROM_VOLUME
                                                                         : GPS_RENDER_SHADED_GREYSCALE_IMAGENORMALS;
        d.out = relocalisationCount != 0 ? GetImageDecision::OUT_KF_RAYCAST : GetImageDecision::OUT_LIVE_RENDER;
        break;
    case T::InfiniTAM_IMAGE_FREECAMERA_SHADED:
    case T::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME:
    case T::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL:
    case T::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_CONFIDENCE:
        d.rays = GetImageDecision::RAYS_FREE_RAYCAST;
        d.renderType = type == T::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME       ? GPS_RENDER_COLOUR_FROM_VOLUME
                       : type == T::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL     ? GPS_RENDER_COLOUR_FROM_NORMAL
                       : type == T::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_CONFIDENCE ? GPS_RENDER_COLOUR_FROM_CONFIDENCE
                                                                                      : GPS_RENDER_SHADED_GREYSCALE;
        d.out = GetImageDecision::OUT_FREE_RENDER;
        break;
    default: break;
    }
    return d;
}

// The verdict itself.  The reference's comes from an SVM over four tracker statistics whose weights are constants of its source
// (ITMExtendedTracker::UpdatePoseQuality); they are not shipped here.  In their place: thresholds on the residual score the tracker
// already reports -- two of the SVM's four inputs: the residual score (trackDiag(10): the root of the mean robust residual, the
// space threshold standing in for every outlier; larger is worse) and the inlier share (trackDiag(8) / n_valid_max: inliers of the
// last accepted evaluation over the valid depth pixels; smaller is worse).  A POOR pair and a FAILED pair; either member of a
// pair trips it.  Off by default so that the verdict stays GOOD, and no default values: nobody has measured where they sit.
struct PoseQualityThresholds {
    bool enabled = false;
    float poorScore = 0.0f, poorInlierShare = 0.0f;       // score > poorScore or share < poorInlierShare: POOR
    float failedScore = 0.0f, failedInlierShare = 0.0f;   // score > failedScore or share < failedInlierShare: FAILED
};
inline ITMTrackingState::TrackingResult poseQualityVerdict(const PoseQualityThresholds& t, float score, float inlierShare) {
    if (!t.enabled) return ITMTrackingState::TRACKING_GOOD;
    if (score > t.failedScore || inlierShare < t.failedInlierShare) return ITMTrackingState::TRACKING_FAILED;
    if (score > t.poorScore || inlierShare < t.poorInlierShare) return ITMTrackingState::TRACKING_POOR;
    return ITMTrackingState::TRACKING_GOOD;
}

class ITMIMUMeasurement;

}  // namespace ITMLib

struct ITMVoxel_s_rgb {};        // ITMLib/Objects/Scene/ITMVoxelTypes.h:41-69 (layout: gps_voxel)
struct ITMVoxelBlockHash {};     // ITMLib/Objects/Scene/ITMVoxelBlockHash.h (layout: gps_hash_entry)
typedef ITMVoxel_s_rgb ITMVoxel;            // ITMLib/ITMLibDefines.h:18
typedef ITMVoxelBlockHash ITMVoxelIndex;    // ITMLib/ITMLibDefines.h:25

class TsdfEngine {
public:
    // capacities: ITMLib/Objects/Scene/ITMVoxelBlockHash.h:18-22
    TsdfEngine(int width, int height, float fx, float fy, float cx, float cy, float voxel_size = 0.005f,
                   float mu = 0.02f, float view_frustum_min = 0.2f, float view_frustum_max = 10.0f,
                   int n_blocks = 0x40000, int n_buckets = 0x100000, int n_excess = 0x20000,
                   torch::Device device = torch::kCUDA);
    virtual ~TsdfEngine() = default;   // (ITMBasicEngine<> is handed out and deleted through this class)

    void resetAll();
    // ITMBasicEngine::ProcessFrame with tracking off: pose := gtC2wPoses[framesProcessed] (ITMBasicEngine.tpp:260-385).
    // rgb uint8[H,W,4] (uchar4) and depth int16[H,W] (mm) device tensors are read in place.
    ITMTrackingState* ProcessFrame(const torch::Tensor& rgb_u8, const torch::Tensor& depth_mm_i16);
    // ITMBasicEngine::runRaycast(pose, intrinsics) (ITMBasicEngine.tpp:501-526): free-view FindVisibleBlocks +
    // CreateExpectedDepths + RenderImage into the free-view render state.  intrinsics == NULL: the depth camera's.
    // pose == NULL && intrinsics == NULL: the re-render of the live view (:503-518) in colour from the volume, from the last
    // full cast while it is current (age_pointCloud <= 0), from the forward projection afterwards -> GetLiveImage().
    void runRaycast(ORUtils::SE3Pose* pose = nullptr, ITMLib::ITMIntrinsics* intrinsics = nullptr);
    // ITMViewBuilder::UpdateView (ViewBuilding/CUDA/ITMViewBuilder_CUDA.cu:32-91) + ProcessFrame: images with a host copy only
    // are uploaded (asynchronously, pinned -> the engine's staging buffers) on the current stream first; images with a device
    // copy are read in place.
    ITMTrackingState* ProcessFrame(ITMUChar4Image* rgbImage, ITMShortImage* rawDepthImage);
    // runRaycast for several poses at once (gps_tsdf_free_raycast_batch): every launch of the free-view chain covers all
    // views, each view renders into a render state of its own (kept by the engine, created on first use) -- view k's images
    // are GetFreeImage(k) / GetFreeVertex(k).  Same images as runRaycast(pose k) would leave in GetFreeImage() / GetFreeVertex().
    // `maps` (optional, one per pose): the runRaycastByCam tensor glue of the view (gps_raycast_to_maps), written by the batch.
    struct ViewMaps { const float* w2c_row_major; float *color_map, *vertex_map, *confidence_map, *depth_map, *depth_map_clamped; };
    void runRaycastBatch(const std::vector<ORUtils::SE3Pose>& poses, ITMLib::ITMIntrinsics* intrinsics = nullptr,
                         const std::vector<ViewMaps>* maps = nullptr,
                         const std::vector<ITMLib::ITMIntrinsics>* per_view_intrinsics = nullptr);
    // creates the render states of views 0 .. n-1 now (runRaycastBatch otherwise creates them on first use: ~20 MB of device
    // allocations per view in the middle of a keyframe update)
    void reserveViews(int n);
    ITMUChar4Image* GetFreeImage(int view) { return views_.at(view)->image_p.get(); }
    ITMFloat4Image* GetFreeVertex(int view) { return views_.at(view)->vertex_p.get(); }
    ITMUChar4Image* GetFreeImage() { return &free_image_; }
    ITMFloat4Image* GetFreeVertex() { return &free_vertex_; }
    ITMFloat4Image* GetLiveVertex() { return &live_vertex_; }
    // ---- approximate raycast (ITMLibSettings::useApproximateRaycast; gps_tsdf_prepare): while the camera stays within
    // sqrt(0.0005) m of the last full cast and that cast is at most 5 frames old, Prepare forward-projects it into the new pose
    // and casts rays for the empty pixels only; the tracker keeps aligning against the ICP maps of the full cast.
    void setUseApproximateRaycast(bool on) { useApproximateRaycast = on; }
    bool usesApproximateRaycast() const { return useApproximateRaycast; }
    // ---- bilateral depth filter (ITMLibSettings::useBilateralFilter; gps_tsdf_convert_filter_depth): UpdateView runs five passes
    // of the 5x5 depth-adaptive filter behind the conversion, so tracking, allocation, integration, the relocaliser and GetImage's
    // original-depth view all see the filtered image (its two outer rows and columns are 0: invalid).  Off: today's launches.
    void setUseBilateralFilter(bool on) { useBilateralFilter = on; }
    bool usesBilateralFilter() const { return useBilateralFilter; }
    bool hasFilterScratch() const { return filter_scratch_.defined(); }   // (allocated by the option's first frame only)
    // ---- full RGB-D calibration (ITMRGBDCalib): a colour camera of its own size, intrinsics and pose, and a disparity calibration
    // of either type.  Call before the first frame.  Frames then carry a colour image of calib.intrinsics_rgb's size, which the
    // engine copies into a buffer of its own; the raw image goes through the calibrated conversion; the integration projects into
    // the colour camera (gps_tsdf_frame_map_rgb); GetImage(ORIGINAL_RGB) answers at the colour size.  Never called: one camera,
    // millimetres, the launches this engine always issued.
    void setCalibration(const ITMLib::ITMRGBDCalib& calib);
    bool hasCalibration() const { return has_cam_; }
    const ITMLib::ITMRGBDCalib& calibration() const { return calib_; }
    Vector2i GetRGBImageSize() const { return has_cam_ ? Vector2i(cam_.width, cam_.height) : Vector2i(state_.width, state_.height); }
    // the last frame's colour image registered to the depth camera (gps_tsdf_register_colour; OURS, not the reference's):
    // uint8 [H, W, 4] at the depth size, alpha 255 where a colour was found, 0 0 0 0 elsewhere; no occlusion test
    torch::Tensor registeredColour();
    int agePointCloud() const { return track_state_.age_point_cloud; }
    torch::Tensor GetForwardProjection() const;   // renderState->forwardProjection, float [H,W,4] (undefined before the first use)
    torch::Tensor GetLiveImage() const { return live_colour_; }   // uchar4 [H,W,4] of the last runRaycast(NULL, NULL)
    // (noFwdProjMissingPoints, the list) of the last forward render: blocking read-back, tests / statistics only
    std::pair<int, torch::Tensor> forwardMissingPoints() const;
    // ---- ITMBasicEngine::GetImage (ITMBasicEngine.tpp:394-498; decideOnGetImage above).  Before the first frame (view == NULL)
    // `out` is left untouched.  The live types render the last full cast while it is current and the forward projection afterwards
    // into the live render image (GetLiveImage()); SCENERAYCAST shades from the ray image's own normals, the others from the
    // volume.  While relocalisationCount != 0 they answer kfRaycast -- which the reference never writes (addKeyframeIdx is never
    // assigned): a cleared image.  The free-camera types run FindVisibleBlocks + CreateExpectedDepths + a cast that leaves the
    // visible list alone into the free-view render state (GetFreeImage()) at `pose` / `intrinsics` (NULL: the depth camera's;
    // the image size is the depth image's).  out must have the engine's image size; a host copy is filled and the stream
    // synchronised (the reference's GetImage is synchronous), a device copy is filled in stream order.
    typedef ITMLib::ITMMainEngineTypes::GetImageType GetImageType;
    void GetImage(ITMUChar4Image* out, GetImageType getImageType, ORUtils::SE3Pose* pose = NULL, ITMLib::ITMIntrinsics* intrinsics = NULL);
    // the same on the device: uint8 [H, W, 4], a tensor of its own, written on the current stream; no synchronisation.
    // Undefined before the first frame.
    torch::Tensor getImageTensor(GetImageType getImageType, ORUtils::SE3Pose* pose = NULL, ITMLib::ITMIntrinsics* intrinsics = NULL);
    float getVoxelSize() const { return state_.voxel_size; }
    ITMTrackingState* GetTrackingState() { return &tracking_state_; }

    // ITMBasicEngine::SaveSceneToMesh (ITMBasicEngine.tpp:105-117): MeshScene (gps_tsdf_mesh_scene, triangles in the CPU
    // engine's deterministic order) + ITMMesh::WritePLY (ITMMesh.h:39-106).  Returns noTotalTriangles.
    int64_t SaveSceneToMesh(const char* fileName, int64_t maxTriangles = (int64_t)1 << 24);
    // {triangles float[maxTriangles,7,3] (p0 p1 p2 c0 c1 c2 clr), counts int64[2]} on the device, no host sync
    std::pair<torch::Tensor, torch::Tensor> MeshScene(int64_t maxTriangles = (int64_t)1 << 24);
    // Geometric evaluation of the mesh (scripts/geo_general.py on the PLY SaveSceneToMesh writes): MeshScene(), then
    // evalPointClouds of the cloud the reference's script reads from that PLY -- all 3 * noTotalTriangles vertices, duplicates
    // included -- against ground-truth points [n,3], or against sample_nums points sampled from ground-truth triangles [T,3,3].
    // Host-synchronous.
    GeomEvalResult EvalMesh(const torch::Tensor& gt_points_or_triangles, const torch::Tensor& transform = torch::Tensor(),
                            const std::vector<double>& dist_thres = {0.03}, int64_t sample_nums = 1000000, uint64_t seed = 0,
                            int64_t maxTriangles = (int64_t)1 << 24);
    // ITMBasicEngine::SaveToFile / LoadFromFile (ITMBasicEngine.tpp:119-171): <dir>Scene/{voxel.dat, alloc.dat, vba.txt,
    // hash.dat, excess.dat, last.txt} in the reference's MemoryBlockPersister format (size_t count + raw elements)
    void SaveToFile(const std::string& saveOutputDirectory);
    void LoadFromFile(const std::string& saveInputDirectory);
    // MAX_RENDERING_BLOCKS (262144) exceeded in some CreateExpectedDepths since the last check?  The reference drops the excess
    // blocks silently (ITMVisualisationEngine_CUDA.tcu:150-163); here the kernel raises counters[GPS_TSDF_OVERFLOW] and this
    // (blocking) read-back turns it into one warning on stderr per engine.  Returns the flag.
    bool checkRenderingBlocks();
    const gps_tsdf_state& state() const { return state_; }
    torch::Tensor currentRgb() const { return frame_inputs_.empty() ? torch::Tensor() : frame_inputs_[0]; }  // view->rgb, [H,W,4] u8
    torch::Tensor counters() const { return counters_; }

    // ITMBasicEngine::turnOffTracking (ITMBasicEngine.tpp:532; createTsdfEngine calls it when use_gt_pose is true,
    // InfiniTAM_tools.cpp:59-62): poses then come from gtC2wPoses.  With tracking active (the reference's default) the
    // depth-only ExtendedTracker of ITMLibSettings.cpp:54-57 estimates them (gps_tsdf_process_frame_tracked).
    void turnOffTracking() { trackingActive = false; }

    // ---- failure modes (ITMBasicEngine.tpp:286-366).  IGNORE, the default, is the path above, launch for launch: no relocaliser
    // is created and verdicts, forced or not, are not looked at.  Otherwise a frame is frame_track, the verdict,
    // decideOnTrackingResult, and what that says: the relocaliser (on the float depth image already in HBM; its answer is read
    // back only on a frame that relocalises), fusion or the visible-list refresh without allocation, the raycast -- or, on
    // FAILED, the old pose and the previous raycast.  framesProcessed then counts fused frames, as the reference's does; the
    // frame index (gtC2wPoses, the staging slot, forced verdicts) is framesSeen.
    void setFailureMode(ITMLib::ITMLibSettings::FailureMode m) { behaviourOnFailure = m; }
    ITMLib::ITMLibSettings::FailureMode failureMode() const { return behaviourOnFailure; }
    void setPoseQualityThresholds(const ITMLib::PoseQualityThresholds& t) { pose_quality_ = t; }
    // the counterpart of the reference's ITMForceFailTracker: the verdict of the frame-th ProcessFrame call (0-based, since
    // construction / resetAll) is `result`, whatever the tracker says
    void forceTrackerResult(int frame, ITMTrackingState::TrackingResult result) { forced_results_[frame] = result; }
    void clearForcedTrackerResults() { forced_results_.clear(); }
    int relocalisationCount = 0;
    int framesSeen = 0;              // ProcessFrame calls since construction / resetAll
    int lastRelocalisedTo = -1;      // keyframe id the last relocalisation restarted from
    bool trackingInitialised = false, fusionActive = true;
    bool lastFrameFused() const { return last_frame_fused_; }
    FernRelocLib::Relocaliser<float>* relocaliser() { return relocaliser_.get(); }
    // the relocalisation step on its own (ITMBasicEngine.tpp:325-329): the pose becomes (M, invM), the visible list is rebuilt
    // and the live raycast rendered there, and the tracker refines the pose against the depth image last converted
    void relocaliseFromPose(const float* M, const float* invM);
    void convertDepth(const torch::Tensor& depth_mm_i16);   // view building's depth conversion alone (ITMViewBuilder: mm -> metres)
    // the tracker's argument line through the BAR (default, when the device memory is host-visible) or in the pinned mailbox
    void setBarArgLine(bool on) { bar_arg_line = on; track_state_.dev_arg_line = on ? track_arg_line_.get() : nullptr; }
    bool usesBarArgLine() const { return track_state_.dev_arg_line != nullptr; }
    // how many of the poses the LM loop would evaluate after a REJECTION ride along with every evaluation (0..2; BAR line only;
    // gps_track_state.mailbox_bytes).  Same poses, fewer round trips; the switch exists for A/B measurements and the equality test.
    void setPosesRidingAlong(int n) {
        poses_riding_along = n < 0 ? 0 : n > kMaxRidingAlong ? kMaxRidingAlong : n;
        track_state_.mailbox_bytes = mailboxBytes();
    }
    // the evaluation's workgroups store their rows of partial sums straight into the pinned mailbox and the tracking thread adds
    // them (default), or a summing workgroup on the device does and only the totals travel (round 4); same poses, bit for bit
    void setHostSummedRows(bool on) { host_summed_rows = on; track_state_.mailbox_bytes = mailboxBytes(); }
    bool hostSummedRows() const { return host_summed_rows; }
    int32_t mailboxBytes() const {
        return (1 + poses_riding_along) * (GPS_TRACK_MAILBOX_BLOCK_BYTES + (host_summed_rows ? GPS_TRACK_MAILBOX_ROWS_BYTES : 0));
    }
    int posesRidingAlong() const { return poses_riding_along; }
    // of the last tracked frame: {poses that rode along with evaluations, poses the loop consumed}
    float trackDiag(int k) const { return k >= 0 && k < 16 ? track_state_.diag[k] : 0.0f; }
    std::pair<int, int> ridingAlongStats() const { return {(int)track_state_.diag[12], (int)track_state_.diag[13]}; }
    // since construction / resetAll: {tracked frames, evaluations the LM loop consumed, poses that rode along, of those consumed}
    std::vector<int64_t> trackerTotals() const { return {tracked_frames_, evals_total_, rode_total_, used_total_}; }
    void turnOnTracking(const char* levels = "rrbb", int numIterC = 20, int numIterF = 50, float outlierSpaceC = 0.1f,
                        float outlierSpaceF = 0.004f, float minstep = 1e-4f, float tukeyCutOff = 8.0f, int framesToSkip = 20,
                        int framesToWeight = 50);
    const gps_track_state& trackState() const { return track_state_; }
    // gps_track_poll_profile of this engine's tracker scratch (blocking; measurement only): {ticks waiting for the host's
    // argument line, ticks evaluating, evaluations, launches retired unused}, cumulative, 100 MHz ticks
    std::vector<int64_t> trackPollProfile() const {
        uint32_t out[4] = {0, 0, 0, 0};
        if (track_scratch_.defined())
            gpsh::check(gps_track_poll_profile(track_scratch_.data_ptr(), state_.width, state_.height, out, gpsh::current_stream()),
                        "gps_track_poll_profile");
        return {out[0], out[1], out[2], out[3]};
    }

    // One-shot hook for the next ProcessFrame: called on the calling thread after the frame's tracking and before its fusion
    // (gps_tsdf_process_frame_tracked_gated); with given poses it runs right before the fusion kernels are enqueued.
    std::function<void()> beforeNextFusion;

    std::vector<ORUtils::SE3Pose> camPoses;       // pose used for every processed frame (ITMBasicEngine.tpp:382)
    std::vector<ITMLib::ITMIntrinsics> camIntrincs;  // ... and its intrinsics (ITMBasicEngine.tpp:383)
    ITMLib::ITMIntrinsics intrinsics_d;            // view->calib.intrinsics_d
    std::vector<torch::Tensor> gtC2wPoses;         // dataset poses, [4,4] float CPU tensors (push before ProcessFrame)
    bool trackingActive = true;
    bool warned_rendering_blocks_ = false;
    int framesProcessed = 0;

private:
    gps_tsdf_state state_{};
    // state_.rgb / frame_inputs_ change per frame (frame thread) while a mapping worker may snapshot state_ for a free-view
    // raycast: the snapshot and the per-frame update take this lock (device-side ordering is the caller's events)
    mutable std::mutex state_mu_;
    torch::Device device_;
    torch::Tensor vba_, vba_alloc_list_, hash_, excess_list_, counters_, alloc_prio_, scan_scratch_, visible_type_,
        visible_ids_, depth_, minmax_, raycast_, icp_points_, icp_normals_, fv_visible_ids_, fv_minmax_, fv_raycast_,
        fv_colour_;
    struct FreeView {  // one ITMRenderState_VH worth of buffers + scratch + counters (gps_tsdf_view)
        torch::Tensor visible_ids, minmax, raycast, colour, scratch, counters;
        std::unique_ptr<ITMUChar4Image> image_p;
        std::unique_ptr<ITMFloat4Image> vertex_p;
    };
    std::vector<std::unique_ptr<FreeView>> views_;
    void ensureView(int k, const gps_tsdf_state& s);
    torch::Tensor view_table_;
    std::vector<torch::Tensor> frame_inputs_;
    torch::Tensor stage_rgb_[2], stage_depth_[2];  // UpdateView staging (host-resident input images), alternating per frame
    gps_track_config track_cfg_{};
    gps_track_state track_state_{};
    torch::Tensor track_scratch_, track_mailbox_;
    // the tracker's argument line in host-writable device memory (gps_track_arg_line_alloc; null without a large BAR).  The
    // switch exists for A/B measurements and for the tests that cover both hand-over paths.
    std::shared_ptr<void> track_arg_line_;
    bool bar_arg_line = true, host_summed_rows = true;
    static constexpr int kMaxRidingAlong = 3;
    int64_t tracked_frames_ = 0, evals_total_ = 0, rode_total_ = 0, used_total_ = 0;
    int poses_riding_along = 1;   // (0 / 1 / 2 measured on the 640x480 loop: 973 / 993 / 980 frames/s sequential, 1,316 / 1,324 / 1,306 overlap)
    ITMLib::ITMLibSettings::FailureMode behaviourOnFailure = ITMLib::ITMLibSettings::FAILUREMODE_IGNORE;
    ITMLib::PoseQualityThresholds pose_quality_;
    std::map<int, ITMTrackingState::TrackingResult> forced_results_;
    std::unique_ptr<FernRelocLib::Relocaliser<float>> relocaliser_;
    bool last_frame_fused_ = true;
    bool useApproximateRaycast = false;
    bool useBilateralFilter = false;
    torch::Tensor filter_scratch_;
    void filterDepth(const torch::Tensor& depth_mm_i16);   // UpdateView with the filter: conversion + five passes into state_.depth
    // the calibration: the colour camera (its image pointer names rgb_c_), the depth calibration when it is not the standard one
    ITMLib::ITMRGBDCalib calib_;
    bool has_cam_ = false, has_depth_calib_ = false;
    gps_colour_camera cam_{};
    gps_depth_calib depth_calib_{};
    torch::Tensor rgb_c_;
    // UpdateView's depth half ahead of the frame's entry points (the filter and / or a calibration: depth_mm NULL afterwards)
    bool convertsAhead() const { return useBilateralFilter || has_cam_; }
    void convertAhead(const torch::Tensor& raw_i16);
    // gps_tsdf_frame_map_fwd, with the colour camera when there is one (NULL: exactly that call)
    int mapHalf(gps_track_state* ts, int fuse, int reset_visible, gps_stream st) {
        return gps_tsdf_frame_map_rgb(&state_, ts, fuse, reset_visible, forwardBlock(), useApproximateRaycast ? 1 : 0, has_cam_ ? &cam_ : nullptr, st);
    }
    torch::Tensor fwd_block_, live_colour_;
    torch::Tensor kf_raycast_, depth_colour_, depth_colour_scratch_;   // GetImage: kfRaycast (never written), DepthToUchar4's image and limits
    torch::Tensor getImageSource(GetImageType type, ORUtils::SE3Pose* pose, ITMLib::ITMIntrinsics* intrinsics);
    void* forwardBlock();   // the forward-render block when the option is on (allocated on first use), else NULL
    ITMTrackingState::TrackingResult verdictOfLastTrack() const;
    void ensureRelocaliser();
    ITMTrackingState* processFrameWithFailureModes(const torch::Tensor& depth_mm_i16);
    ORUtils::SE3Pose pose_d_;
    ITMTrackingState tracking_state_{&pose_d_};
    ITMUChar4Image free_image_;
    ITMFloat4Image free_vertex_, live_vertex_;
};

// Colour registered to the depth camera, without an engine (gps_tsdf_register_colour; OURS, not the reference's): depth_f float
// [Hd, Wd] device tensor in metres (<= 0: invalid), intrinsics_d = (fx, fy, cx, cy) of the depth camera, the calibration's colour
// camera and extrinsics, rgb uint8 [Hc, Wc, 4] device tensor -> uint8 [Hd, Wd, 4], alpha 255 where a colour was found, 0 0 0 0
// elsewhere.  One launch on the current stream, no host read, no occlusion test.
torch::Tensor registerColour(const torch::Tensor& depth_f, const std::vector<float>& intrinsics_d, const ITMLib::ITMRGBDCalib& calib,
                             const torch::Tensor& rgb_u8);
