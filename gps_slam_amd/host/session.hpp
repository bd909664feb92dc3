// slam_trainer.cpp:26-75 of the reference as library calls: construct from the config file's nodes, train, save the model, the
// engine, the mesh and the poses, render for evaluation -- and, in work_mode eval, reload both halves in a fresh process and
// render.  Reading images from disk, the JPEG / PNG encoders and TensorBoard stay outside: the reader comes
// in filled, the renders go out as tensors.
#pragma once
#include <string>
#include <vector>

#include "slam_pipeline.hpp"

// ---- the small files of Pipeline::save / DatasetReader::savePose, on host tensors (no device needed)
// saveCfgArgs (src/file_utils.cpp:162-169): the one line 3DGS viewers read the SH degree from
std::string cfgArgsLine(int maxSH);
void writeCfgArgs(const std::string& file_name, int maxSH);
// saveCameras (src/dataset_reader.cpp:420-460) in nlohmann's layout: one compact array, per camera the keys in alphabetical order
// (fx, fy, height, id, img_name, position, rotation, width), id = the index, position / rotation from c2w_slam, floats widened to
// double and printed with the fewest digits that read back to the same value ("600.0", "0.10000000149011612"), nlohmann's choice
// between plain and exponent notation and its short string escapes.  Not its output byte for byte in every case: Grisu2 is now
// and then one digit longer than the shortest, and a name that is not UTF-8 is written as it is where nlohmann throws.
std::string camerasJson(const std::vector<Camera>& cams);
void writeCamerasJson(const std::string& file_name, const std::vector<Camera>& cams);
// saveTensorTXT (src/file_utils.cpp:224-257): a 4x4 float tensor, four lines of four numbers, fixed notation, six decimals
std::string poseTxt(const torch::Tensor& c2w);
void writePoseTxt(const std::string& file_name, const torch::Tensor& c2w);
torch::Tensor readPoseTxt(const std::string& file_name);   // -> float32 [4,4] (host)
// Camera::getFrameID (src/dataset_reader.cpp:134-160): what stands between "frame" and ".jpg" in the image's name; a camera without
// such a name gets its id (its index `fallback_index` if it has none) as six digits, like the reference's idToFilename
std::string frameIdOf(const Camera& cam, size_t fallback_index);

// src/file_utils.cpp:97-160.  createDirectory(path, true) EMPTIES an existing directory, as the reference's does (a filesystem
// root, an empty path, and the current directory or one above it (".", "..") are refused).  createWorkSpace: the file's
// workspace_dir, emptied, with a copy of the file in it; returns it (a config file inside its own workspace_dir is refused: it
// would be removed before the copy).
bool createDirectory(const std::string& path, bool overwrite = false);
std::string createWorkSpace(const std::string& config_filename);

struct SessionResult {
    std::string work_mode, workspace_dir;
    std::vector<TensorDict> renders;   // renderEvalImgs(train_vec, {"rgb"}): eval_after_train / work_mode eval; else empty
    ImageEvalResult image_eval;        // evalImages over the same cameras (empty without Gaussians or without camera images)
    bool has_image_eval = false;
    int keyframe_count = 0;
    int gaussian_num = 0;
    // PIPE.refine_iterations > 0: gesTrainCams between SLAMTrainCams and save -- the iterations it ran and its {iter, loss} log
    int refine_iterations_done = 0;
    std::vector<SLAMPipeline::RefineLogEntry> refine_log;
    SLAMPipeline::PipelineTimes times;
    std::vector<std::string> files;    // every file / directory the session wrote
};

// The body of slam_trainer.cpp:26-75 on `reader`, which the caller has filled (loadConfig(root["READER"]) + train_vec).
//   train / recon: model.loadConfig(MODEL); createWorkSpace(config_filename) if one is given (else workspace_dir is created, not
//     emptied); pipe.loadConfig(PIPE, workspace_dir, true); SLAMTrainCams -- reader.train_vec[i].c2w_slam are the estimated poses
//     afterwards; train with PIPE.refine_iterations > 0: gesTrainCams over refine_cams (keyframes: keyframe_cam_list + the live
//     window; all: train_vec) for that many iterations; save_after_train: save, saveEngine, saveMesh, savePoses(eval_path + "/pose");
//     eval_after_train: the renders.
//   eval: model.loadConfig; loadParamsTensor(workspace_dir + "/gs_model/model.pt") (a workspace without one -- a recon run -- gives
//     an empty model, and a line on stderr says so); pipe.loadConfig(PIPE, workspace_dir, false); loadEngine; the engine's
//     per-frame poses and intrinsics (which its file does not hold) are restored from the reader's cameras: pose = c2w_slam, read from eval_path/pose/frame<id>.txt
//     first if poses_from_files; the renders.
// Every section is converted before the engine is built: a missing or unknown key throws gpsh::ConfigError with nothing allocated.
// The engine is shut down and detached before this returns (also when it throws).
SessionResult runSession(const gpsh::Node& root, DatasetReader& reader, const std::string& config_filename = "",
                         bool poses_from_files = false, uint64_t seed = 1234);
