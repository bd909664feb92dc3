#include "session.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <sstream>

namespace fs = std::filesystem;
using namespace gpsh;

// ------------------------------------------------------------------ the small files (host tensors only)
std::string cfgArgsLine(int maxSH) {
    return "Namespace(data_device='cuda', eval=False, images='images', model_path='', resolution=-1, sh_degree=" + std::to_string(maxSH) +
           ", source_path='', white_background=False)\n";
}

static void writeText(const std::string& file_name, const std::string& text) {
    std::ofstream o(file_name, std::ios::binary);
    TORCH_CHECK((bool)o, "cannot open ", file_name, " for writing");
    o << text;
    o.close();
    TORCH_CHECK((bool)o, "cannot write ", file_name);
}

void writeCfgArgs(const std::string& file_name, int maxSH) { writeText(file_name, cfgArgsLine(maxSH)); }

namespace {
// a float as nlohmann's dump() prints the double it was widened to: the fewest digits that read back to the same double, and
// ".0" behind a number that would otherwise look like an integer; NaN and the infinities are null
std::string jsonNumber(float f) {
    const double v = (double)f;
    if (!std::isfinite(v)) return "null";
    if (v == 0.0) return std::signbit(v) ? "-0.0" : "0.0";
    char buf[40];
    for (int p = 0; p <= 16; p++) {   // d.ddd...e+XX with p decimals
        snprintf(buf, sizeof buf, "%.*e", p, std::fabs(v));
        if (std::strtod(buf, nullptr) == std::fabs(v)) break;
    }
    std::string digits;
    const char* e = buf;
    for (; *e && *e != 'e'; e++)
        if (*e != '.') digits += *e;
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    const int k = (int)digits.size(), n = std::atoi(e + 1) + 1;   // value = 0.digits x 10^n
    // the layout of nlohmann's format_buffer: plain decimals for -4 < n <= 15, else d.ddde+XX with at least two exponent digits
    std::string s = v < 0 ? "-" : "";
    if (k <= n && n <= 15) return s + digits + std::string(n - k, '0') + ".0";
    if (0 < n && n <= 15) return s + digits.substr(0, n) + "." + digits.substr(n);
    if (-4 < n && n <= 0) return s + "0." + std::string(-n, '0') + digits;
    s += digits.substr(0, 1);
    if (k > 1) s += "." + digits.substr(1);
    const int ex = n - 1;
    char eb[16];
    snprintf(eb, sizeof eb, "e%c%02d", ex < 0 ? '-' : '+', ex < 0 ? -ex : ex);
    return s + eb;
}

std::string jsonString(const std::string& t) {
    std::string s = "\"";
    for (const char c : t) {
        if (c == '"' || c == '\\') { s += '\\'; s += c; }
        else if (c == '\n') s += "\\n";
        else if (c == '\t') s += "\\t";
        else if (c == '\r') s += "\\r";
        else if (c == '\b') s += "\\b";
        else if (c == '\f') s += "\\f";
        else if ((unsigned char)c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", (unsigned)(unsigned char)c); s += b; }
        else s += c;
    }
    return s + "\"";
}

torch::Tensor hostPose(const torch::Tensor& c2w, const char* who) {
    TORCH_CHECK(c2w.defined() && c2w.dim() == 2 && c2w.size(0) == 4 && c2w.size(1) == 4, who, ": a 4x4 pose is needed");
    return c2w.detach().to(torch::kCPU, torch::kFloat32).contiguous();
}
}  // namespace

std::string camerasJson(const std::vector<Camera>& cams) {
    std::string s = "[";
    for (size_t i = 0; i < cams.size(); i++) {
        const Camera& cam = cams[i];
        const auto pose = hostPose(cam.c2w_slam, "cameras.json (c2w_slam)");
        const float* m = pose.data_ptr<float>();
        if (i) s += ",";
        s += "{\"fx\":" + jsonNumber(cam.fx) + ",\"fy\":" + jsonNumber(cam.fy) + ",\"height\":" + std::to_string(cam.height) +
             ",\"id\":" + std::to_string(i) + ",\"img_name\":" + jsonString(cam.img_name) + ",\"position\":[" + jsonNumber(m[3]) + "," +
             jsonNumber(m[7]) + "," + jsonNumber(m[11]) + "],\"rotation\":[";
        for (int r = 0; r < 3; r++)
            s += std::string(r ? "," : "") + "[" + jsonNumber(m[4 * r]) + "," + jsonNumber(m[4 * r + 1]) + "," + jsonNumber(m[4 * r + 2]) + "]";
        s += "],\"width\":" + std::to_string(cam.width) + "}";
    }
    return s + "]";
}

void writeCamerasJson(const std::string& file_name, const std::vector<Camera>& cams) { writeText(file_name, camerasJson(cams)); }

std::string poseTxt(const torch::Tensor& c2w) {
    const auto pose = hostPose(c2w, "pose file");
    const float* m = pose.data_ptr<float>();
    std::ostringstream o;
    o << std::fixed << std::setprecision(6);
    for (int r = 0; r < 4; r++) {
        for (int c = 0; c < 4; c++) o << m[4 * r + c] << (c < 3 ? " " : "");
        o << "\n";
    }
    return o.str();
}

void writePoseTxt(const std::string& file_name, const torch::Tensor& c2w) { writeText(file_name, poseTxt(c2w)); }

torch::Tensor readPoseTxt(const std::string& file_name) {
    std::ifstream f(file_name);
    TORCH_CHECK((bool)f, "cannot open ", file_name);
    auto t = torch::empty({4, 4}, torch::kFloat32);
    for (int k = 0; k < 16; k++) TORCH_CHECK((bool)(f >> t.data_ptr<float>()[k]), file_name, ": sixteen numbers are needed");
    return t;
}

std::string frameIdOf(const Camera& cam, size_t fallback_index) {
    const size_t start = cam.img_name.find("frame");
    if (start != std::string::npos) {
        const size_t end = cam.img_name.find(".jpg", start + 5);
        if (end != std::string::npos) return cam.img_name.substr(start + 5, end - start - 5);
    }
    std::ostringstream o;
    o << std::setw(6) << std::setfill('0') << (cam.id >= 0 ? (long long)cam.id : (long long)fallback_index);
    return o.str();
}

bool createDirectory(const std::string& path, bool overwrite) {
    const fs::path dir(path);
    TORCH_CHECK(!path.empty() && dir != dir.root_path(), "createDirectory: refusing '", path, "'");
    if (fs::exists(dir)) {
        if (!overwrite) return false;
        // emptying the directory the process stands in, or one above it (".", "..", a home directory), is never meant
        const fs::path target = fs::weakly_canonical(dir), cwd = fs::current_path();
        const auto rel = cwd.lexically_relative(target);
        TORCH_CHECK(rel.empty() || *rel.begin() == "..", "createDirectory: refusing to empty '", path,
                    "': the current directory is that directory or lies inside it");
        fs::remove_all(dir);
    }
    return fs::create_directories(dir) || fs::is_directory(dir);
}

std::string createWorkSpace(const std::string& config_filename) {
    const std::string workspace_dir = loadYamlFile(config_filename)["workspace_dir"].as<std::string>();
    const fs::path source(config_filename);
    {   // a config file that lives inside its own workspace_dir would be removed before it could be copied
        const auto rel = fs::weakly_canonical(source).lexically_relative(fs::weakly_canonical(fs::path(workspace_dir)));
        TORCH_CHECK(rel.empty() || *rel.begin() == "..", "createWorkSpace: ", config_filename, " lies inside its own workspace_dir '",
                    workspace_dir, "', which is emptied first: keep the file elsewhere");
    }
    createDirectory(workspace_dir, true);
    fs::copy_file(source, fs::path(workspace_dir) / source.filename(), fs::copy_options::overwrite_existing);
    return workspace_dir;
}

// ------------------------------------------------------------------ SLAMPipeline: the session's output
void SLAMPipeline::createOutputDirs() {
    // src/pipeline.cpp:27-32 and slam_pipeline.cpp:188-192 (no TensorBoard directory: there is no logger)
    fs::create_directories(workspace_dir);
    for (const std::string& p : {model_path, log_path, eval_path}) {
        if (fs::path(p).lexically_normal() == fs::path(workspace_dir).lexically_normal()) continue;   // (an empty name: leave the workspace alone)
        createDirectory(p, true);
    }
    if (!saved_images.empty()) createDirectory(workspace_dir + "/" + saved_images, true);
    createDirectory(workspace_dir + "/before_opt", true);
}

std::vector<std::string> SLAMPipeline::save(SLAMGaussianModel& model_, const std::vector<Camera>& cams) {
    flush();
    std::vector<std::string> files;
    if (model_.getGaussianNum() == 0) return files;   // "empty model"
    const fs::path dir(model_path);
    createDirectory((dir / "point_cloud").string(), true);
    files = {(dir / "cfg_args").string(), (dir / "point_cloud" / "point_cloud.ply").string(), (dir / "model.pt").string(),
             (dir / "cameras.json").string()};
    writeCfgArgs(files[0], model_.getMaxSH());
    model_.saveParamsPly(files[1]);
    model_.saveParamsTensor(files[2]);
    writeCamerasJson(files[3], cams);
    return files;
}

std::vector<std::string> SLAMPipeline::savePoses(const std::string& dir, const std::vector<Camera>& cams) {
    fs::create_directories(dir);
    std::vector<std::string> files;
    for (size_t i = 0; i < cams.size(); i++) {
        files.push_back((fs::path(dir) / ("frame" + frameIdOf(cams[i], i) + ".txt")).string());
        writePoseTxt(files.back(), cams[i].c2w_slam);
    }
    return files;
}

// ------------------------------------------------------------------ the session
namespace {
// cameras as renderEvalImgs wants them: copies with the pose pack on the device (the reader's keep host tensors only)
std::vector<Camera> deviceCameras(const std::vector<Camera>& cams, const torch::Device& device) {
    std::vector<Camera> out(cams);
    for (Camera& c : out) { c.invalidate(); c.toGPU(device); }
    return out;
}

void renderForEval(SLAMPipeline& pipe, SLAMGaussianModel& model, const std::vector<Camera>& train_vec, SessionResult& res) {
    const std::vector<Camera> cams = deviceCameras(train_vec, pipe.device);
    res.renders = pipe.renderEvalImgs(cams, {"rgb"});
    bool images = !cams.empty();
    for (const Camera& c : cams) images = images && c.image.defined();
    if (images && model.getGaussianNum() > 0) {
        res.image_eval = pipe.evalImages(cams);
        res.has_image_eval = true;
    }
}
}  // namespace

SessionResult runSession(const Node& root, DatasetReader& reader, const std::string& config_filename, bool poses_from_files, uint64_t seed) {
    SessionResult res;
    res.workspace_dir = root["workspace_dir"].as<std::string>();
    res.work_mode = root["work_mode"].as<std::string>();
    (void)root["dev_id"].as<int>();   // (slam_trainer.cpp:17, :30 read it as a string and as an int; the device is the process's current one)
    if (res.work_mode != "train" && res.work_mode != "recon" && res.work_mode != "eval")
        throw ConfigError("work_mode: 'train', 'recon' or 'eval', got '" + res.work_mode + "' (" + root["work_mode"].source() + ":" +
                          std::to_string(root["work_mode"].line()) + ")", root["work_mode"].line());
    const bool train = res.work_mode != "eval";
    const std::string& workspace_dir = res.workspace_dir;
    TORCH_CHECK(!reader.train_vec.empty(), "runSession: the reader holds no cameras");
    SLAMGaussianModel model;
    SLAMPipeline pipe(seed);
    // every section converts, once, before anything is built
    TsdfConfig tsdf;
    const Config model_cfg = model.flattenConfig(root["MODEL"]);
    const Config pipe_cfg = pipe.flattenConfig(root["PIPE"]);
    const Config tsdf_cfg = flattenNode(root["PIPE"]["TSDF"], "PIPE.TSDF", [&](auto& v) { tsdf.configFields(v); });

    InfiniTAM::Engine::CLIEngine* engine = createTsdfEngine(reader, tsdf_cfg);
    struct Shutdown {   // (declared behind the pipeline: the engine goes first, and its Shutdown() detaches it from the pipeline)
        InfiniTAM::Engine::CLIEngine* e;
        ~Shutdown() { if (e) e->Shutdown(); }
    } shutdown{engine};
    pipe.setTsdfEngine(engine);
    pipe.scene_scale = reader.scene_scale;
    model.loadConfig(model_cfg);
    pipe.workspace_dir = workspace_dir;
    pipe.applyConfig(pipe_cfg, true);
    pipe.work_mode = res.work_mode;

    if (train) {
        if (!config_filename.empty()) {
            const std::string made = createWorkSpace(config_filename);
            if (fs::path(made).lexically_normal() != fs::path(workspace_dir).lexically_normal()) fs::create_directories(workspace_dir);
            res.files.push_back((fs::path(made) / fs::path(config_filename).filename()).string());
        } else {
            fs::create_directories(workspace_dir);
        }
        pipe.createOutputDirs();
        pipe.SLAMTrainCams(model, reader.train_vec);
        res.times = pipe.times;
        res.keyframe_count = (int)pipe.keyframe_cam_list.size();
        if (pipe.refine_iterations > 0 && res.work_mode == "train") {
            // the pass over all keyframes (or all cameras) once the sequence is over, before anything is saved or rendered
            res.refine_iterations_done = pipe.gesTrainCams(pipe.refine_cams == "all" ? reader.train_vec : pipe.refineKeyframeCams(),
                                                           pipe.refine_iterations);
            res.refine_log = pipe.refine_log;
        }
        if (pipe.save_after_train) {
            for (const std::string& f : pipe.save(model, reader.train_vec)) res.files.push_back(f);
            pipe.saveEngine();
            if (!pipe.saved_engine.empty()) res.files.push_back(workspace_dir + "/" + pipe.saved_engine);
            pipe.saveMesh();
            if (!pipe.saved_mesh.empty()) res.files.push_back(workspace_dir + "/" + pipe.saved_mesh);
            for (const std::string& f : pipe.savePoses(pipe.eval_path + "/pose", reader.train_vec)) res.files.push_back(f);
        }
        if (pipe.eval_after_train) renderForEval(pipe, model, reader.train_vec, res);
    } else {
        const std::string model_file = workspace_dir + "/gs_model/model.pt";   // (slam_trainer.cpp:68: not PIPE.model_path)
        if (fs::exists(model_file)) model.loadParamsTensor(model_file);
        else fprintf(stderr, "runSession: %s does not exist -- evaluating the TSDF views alone (a recon workspace, or a wrong workspace_dir?)\n",
                     model_file.c_str());
        pipe.model = &model;
        pipe.device = model.device;
        TORCH_CHECK(!pipe.saved_engine.empty(), "work_mode eval: PIPE.TSDF.saved_engine names no engine directory");
        pipe.loadEngine();
        // what the engine's file does not hold and renderEvalImgs reads per camera id: the frame's pose and intrinsics
        TsdfEngine* eng = pipe.main_engine;
        int frames = 0;
        for (const Camera& c : reader.train_vec) frames = std::max(frames, c.id + 1);
        ITMLib::ITMIntrinsics intr;
        intr.SetFrom(reader.width, reader.height, reader.fx, reader.fy, reader.cx, reader.cy);
        eng->camPoses.assign(frames, ORUtils::SE3Pose());
        eng->camIntrincs.assign(frames, intr);
        for (size_t i = 0; i < reader.train_vec.size(); i++) {
            Camera& c = reader.train_vec[i];
            if (poses_from_files) c.c2w_slam = readPoseTxt(pipe.eval_path + "/pose/frame" + frameIdOf(c, i) + ".txt");
            if (c.id < 0) continue;   // (rendered with its own c2w and intrinsics)
            // SetInvM + Coerce is not idempotent in the last bit (log, exp and two inversions), and a c2w_slam is the engine's
            // GetInvM() alone.  Where the dataset pose coerces to exactly this estimate -- use_gt_pose, every shipped config --
            // that coerced dataset pose IS the pose the engine held, M included; any other estimate (a tracked pose, a pose
            // read back from six decimals) is coerced again.
            const auto pose = c.c2w_slam.detach().to(torch::kCPU, torch::kFloat32).contiguous();
            ORUtils::SE3Pose p;
            bool exact = false;
            if (c.c2w.defined()) {
                const auto gt = c.c2w.detach().to(torch::kCPU, torch::kFloat32).contiguous();
                p.SetInvM(gt.data_ptr<float>());
                p.Coerce();
                exact = true;
                for (int r = 0; r < 4; r++)
                    for (int k = 0; k < 4; k++) exact = exact && p.GetInvM()[4 * k + r] == pose.data_ptr<float>()[4 * r + k];
            }
            if (!exact) {
                p.SetInvM(pose.data_ptr<float>());
                p.Coerce();
            }
            eng->camPoses[c.id] = p;
        }
        renderForEval(pipe, model, reader.train_vec, res);
    }
    res.gaussian_num = model.getGaussianNum();
    return res;
}
