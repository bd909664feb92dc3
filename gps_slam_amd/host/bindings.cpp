// pybind11 view of the C++ host layer (module gps_slam_amd._host): lets the Python tests and bench.py drive exactly the
// C++ classes a C++ slam_trainer would link against.
#include <torch/extension.h>

#include "session.hpp"

namespace py = pybind11;

static gpsh::Config config_from_dict(const py::dict& d) {
    gpsh::Config c;
    for (auto item : d) {
        const std::string k = py::str(item.first);
        if (py::isinstance<py::str>(item.second)) c.str[k] = py::str(item.second);
        else c.num[k] = item.second.cast<double>();
    }
    return c;
}

// gpsh::Node -> nested dict / list / str (None for a null), in file order
static py::object node_to_python(const gpsh::Node& n) {
    if (n.IsMap()) {
        py::dict d;
        for (const auto& kv : n) d[py::str(kv.first)] = node_to_python(kv.second);
        return std::move(d);
    }
    if (n.IsSequence()) {
        py::list l;
        for (const gpsh::Node& e : n.elements()) l.append(node_to_python(e));
        return std::move(l);
    }
    if (n.IsScalar()) return py::str(n.text());
    if (n.IsNull()) return py::none();
    throw gpsh::ConfigError((n.path().empty() ? std::string("<root>") : n.path()) + ": key is missing");
}

// the current value of every configuration field, through the entry point's one key list (config_fields.hpp): "settings()"
namespace {
struct FieldDumper {
    py::dict out;
    std::string prefix;
    FieldDumper section(const char* k) const { return FieldDumper{out, prefix + k + "."}; }
    template <class T> void put(const char* k, const T& v) { out[py::str(prefix + k)] = v; }
    void i(const char* k, int& v, gpsh::FieldUse = gpsh::kRequired) { put(k, v); }
    void i64(const char* k, int64_t& v, gpsh::FieldUse = gpsh::kRequired) { put(k, v); }
    void f(const char* k, float& v, gpsh::FieldUse = gpsh::kRequired) { put(k, v); }
    void d(const char* k, double& v, gpsh::FieldUse = gpsh::kRequired) { put(k, v); }
    void b(const char* k, bool& v, gpsh::FieldUse = gpsh::kRequired) { put(k, v); }
    void s(const char* k, std::string& v, gpsh::FieldUse = gpsh::kRequired) { put(k, v); }
    void ignored(const char*) {}
};
// gpsh::RandomSelector points into its items: the Python object holds them
struct PySelector {
    std::vector<int64_t> items;
    gpsh::RandomSelector<int64_t> sel;
    PySelector(std::vector<int64_t> v, uint64_t seed) : items(std::move(v)), sel(items, seed) {}
    PySelector(const PySelector&) = delete;
};
}  // namespace

PYBIND11_MODULE(_host, m) {
    m.doc() = "C++ host layer of gps_slam_amd over the C-ABI (libgpsslam_hip.so)";

    // ---- configuration files (config_node.hpp): a gpsh::ConfigError arrives as ConfigError(ValueError) with the same message
    py::register_exception<gpsh::ConfigError>(m, "ConfigError", PyExc_ValueError);
    py::class_<gpsh::Node>(m, "Node")
        .def("__getitem__", [](const gpsh::Node& n, const std::string& k) { return n[k]; })
        .def("__getitem__", [](const gpsh::Node& n, int64_t i) { return i < 0 ? n[(int)-1] : n[(size_t)i]; })
        // (indexing never raises, as in C++: an out-of-range index is an undefined node -- so iteration is defined here and does
        // not fall back to Python's index protocol, which would never end) a map gives its keys, a sequence its elements
        .def("__iter__", [](const gpsh::Node& n) -> py::object {
            py::list items;
            if (n.IsMap()) for (const auto& kv : n) items.append(py::str(kv.first));
            else if (n.IsSequence()) for (const gpsh::Node& e : n.elements()) items.append(py::cast(e));
            else throw py::type_error("a scalar, null or undefined Node is not iterable");
            return items.attr("__iter__")();
        })
        .def("__len__", &gpsh::Node::size)
        .def("size", &gpsh::Node::size)
        .def("IsDefined", &gpsh::Node::IsDefined)
        .def("IsNull", &gpsh::Node::IsNull)
        .def("IsScalar", &gpsh::Node::IsScalar)
        .def("IsSequence", &gpsh::Node::IsSequence)
        .def("IsMap", &gpsh::Node::IsMap)
        .def("keys", [](const gpsh::Node& n) { std::vector<std::string> k; for (const auto& kv : n) k.push_back(kv.first); return k; })
        .def_property_readonly("path", [](const gpsh::Node& n) { return n.path(); })
        .def_property_readonly("line", &gpsh::Node::line)
        .def("to_python", &node_to_python)
        .def("as_int", [](const gpsh::Node& n) { return n.as<int>(); })
        .def("as_int64", [](const gpsh::Node& n) { return n.as<int64_t>(); })
        .def("as_float", [](const gpsh::Node& n) { return n.as<float>(); })
        .def("as_double", [](const gpsh::Node& n) { return n.as<double>(); })
        .def("as_bool", [](const gpsh::Node& n) { return n.as<bool>(); })
        .def("as_str", [](const gpsh::Node& n) { return n.as<std::string>(); })
        .def("as_float_list", [](const gpsh::Node& n) { return n.as<std::vector<float>>(); })
        .def("as_int_list", [](const gpsh::Node& n) { return n.as<std::vector<int>>(); });
    m.def("parse_yaml", &gpsh::parseYaml, py::arg("text"), py::arg("name") = "");
    m.def("load_yaml", &gpsh::loadYamlFile, py::arg("path"));

    // ---- operator surface (gsplat_wapper.hpp)
    m.def("SphericalHarmonicsNew", [](int deg, torch::Tensor dirs, torch::Tensor coeffs, torch::Tensor masks) {
        return SphericalHarmonicsNew::apply(deg, dirs, coeffs, masks);
    });
    m.def("FullyFusedProjection", [](torch::Tensor means, torch::Tensor quats, torch::Tensor scales, torch::Tensor viewmats,
                                    torch::Tensor Ks, int w, int h, float eps2d, float near_plane, float far_plane,
                                    float radius_clip) {
        return FullyFusedProjection::apply(means, c10::nullopt, quats, scales, viewmats, Ks, w, h, eps2d, near_plane,
                                           far_plane, radius_clip, false, std::string("pinhole"));
    });
    m.def("RasterizeToPixelsGes_NewParallel",
          [](torch::Tensor means2d, torch::Tensor conics, torch::Tensor colors, torch::Tensor opacities, torch::Tensor radiis,
             torch::Tensor ref_depth_map, torch::Tensor base_color_map, int w, int h, int tile_size,
             torch::Tensor isect_offsets, torch::Tensor flatten_ids, torch::Tensor group_gs_ids, torch::Tensor group_starts,
             float delta_depth) {
              return RasterizeToPixelsGes_NewParallel::apply(means2d, conics, colors, opacities, radiis, ref_depth_map,
                                                             base_color_map, c10::nullopt, c10::nullopt, w, h, tile_size,
                                                             isect_offsets, flatten_ids, group_gs_ids, group_starts,
                                                             false, delta_depth);
          });
    m.def("RasterizeToPixelsGes",
          [](torch::Tensor means2d, torch::Tensor conics, torch::Tensor colors, torch::Tensor opacities,
             torch::Tensor ref_depth_map, torch::Tensor base_color_map, int w, int h, int tile_size,
             torch::Tensor isect_offsets, torch::Tensor flatten_ids, float delta_depth) {
              return RasterizeToPixelsGes::apply(means2d, conics, colors, opacities, ref_depth_map, base_color_map, c10::nullopt,
                                                 c10::nullopt, w, h, tile_size, isect_offsets, flatten_ids, false, delta_depth);
          });
    m.def("RasterizeToPixels",
          [](torch::Tensor means2d, torch::Tensor conics, torch::Tensor colors, torch::Tensor opacities,
             c10::optional<torch::Tensor> backgrounds, int w, int h, int tile_size, torch::Tensor isect_offsets,
             torch::Tensor flatten_ids, bool absgrad) {
              return RasterizeToPixels::apply(means2d, conics, colors, opacities, backgrounds, c10::nullopt, w, h, tile_size,
                                              isect_offsets, flatten_ids, absgrad);
          });
    m.def("FusedSSIMMap", [](double C1, double C2, torch::Tensor img1, torch::Tensor img2, std::string padding, bool train) {
        return FusedSSIMMap::apply(C1, C2, img1, img2, padding, train);
    });
    m.def("isectTiles", &isectTiles, py::arg("means2d"), py::arg("radii"), py::arg("depths"), py::arg("tile_size"),
          py::arg("tile_width"), py::arg("tile_height"), py::arg("sort") = true);
    m.def("isectOffsetEncode", &isectOffsetEncode);
    m.def("isectTilesNoDepth", &isectTilesNoDepth, py::arg("means2d"), py::arg("radii"), py::arg("depths"),
          py::arg("tile_size"), py::arg("tile_width"), py::arg("tile_height"), py::arg("sort") = true);
    m.def("isectOffsetEncodeNoDepth", &isectOffsetEncodeNoDepth);
    m.def("distCUDA2", &distCUDA2);
    m.def("simpleKNN", &simpleKNN);
    m.def("degFromSh", &degFromSh);
    m.def("numShBases", &numShBases);
    m.def("rgb2sh", &rgb2sh);
    m.def("sh2rgb", &sh2rgb);
    m.def("poseInv", &poseInv);
    m.def("RawGaussianParamsMake", &RawGaussianParams::make, py::arg("xyz"), py::arg("rgb"), py::arg("normals"),
          py::arg("max_sh_degree") = 3, py::arg("init_opacs") = 0.5f, py::arg("max_scale") = 0.01f, py::arg("min_scale") = -1.0f);
    m.def("computeNormalMap", &computeNormalMap);
    m.def("getGPUMemoryUsage", &getGPUMemoryUsage, py::arg("gpu_id") = 0);

    // ---- Camera
    py::class_<Camera>(m, "Camera")
        .def(py::init<int, int, float, float, float, float, bool, const torch::Tensor&>())
        .def_readwrite("id", &Camera::id)
        .def_readwrite("width", &Camera::width)
        .def_readwrite("height", &Camera::height)
        .def_readwrite("fx", &Camera::fx)
        .def_readwrite("fy", &Camera::fy)
        .def_readwrite("cx", &Camera::cx)
        .def_readwrite("cy", &Camera::cy)
        .def_readwrite("image", &Camera::image)
        .def_readwrite("depth", &Camera::depth)
        .def_readwrite("c2w", &Camera::c2w)
        .def_readwrite("c2w_slam", &Camera::c2w_slam)
        .def_readwrite("img_name", &Camera::img_name)
        .def("toGPU", [](Camera& c) { c.toGPU(); })
        .def("invalidate", &Camera::invalidate)
        .def("viewmat", &Camera::viewmat_tensor)
        .def("K_dev", &Camera::K_tensor)
        .def("cam_pos", &Camera::cam_pos_tensor);

    // ---- model
    py::class_<RawGaussianParams>(m, "RawGaussianParams")
        .def("getGaussianNum", &RawGaussianParams::getGaussianNum)
        .def("getMeans", &RawGaussianParams::getMeans)
        .def("getScales", &RawGaussianParams::getScales)
        .def("getQuats", &RawGaussianParams::getQuats)
        .def("getFeaturesDc", &RawGaussianParams::getFeaturesDc)
        .def("getFeaturesRest", &RawGaussianParams::getFeaturesRest)
        .def("getOpacities", &RawGaussianParams::getOpacities)
        .def("getExposure", &RawGaussianParams::getExposure)
        .def("setExposure", &RawGaussianParams::setExposure)
        .def("add", [](RawGaussianParams& p, std::vector<torch::Tensor> t) { p.add(t); })
        .def("remove", &RawGaussianParams::remove)
        .def("savePly", &RawGaussianParams::savePly)
        .def("saveTensor", &RawGaussianParams::saveTensor)
        .def("loadTensor", &RawGaussianParams::loadTensor)
        .def_static("make", &RawGaussianParams::make);

    py::class_<SLAMGaussianModel>(m, "SLAMGaussianModel")
        .def(py::init<>())
        .def("loadConfig", [](SLAMGaussianModel& s, const py::dict& d) { s.loadConfig(config_from_dict(d)); })
        .def("loadConfig", [](SLAMGaussianModel& s, const gpsh::Node& model_node) { s.loadConfig(model_node); })
        .def("settings", [](SLAMGaussianModel& s) {
            FieldDumper dump;
            int64_t capacity = s.getGaussianParms().capacity();
            s.configFields(dump, capacity);
            return dump.out;
        })
        .def("flattenConfig", [](SLAMGaussianModel& s, const gpsh::Node& model_node) {
            // what loadConfig(node) would read, as the flat route's dict; nothing is assigned or allocated
            const gpsh::Config c = s.flattenConfig(model_node);
            py::dict d;
            for (const auto& kv : c.num) d[py::str(kv.first)] = kv.second;
            for (const auto& kv : c.str) d[py::str(kv.first)] = kv.second;
            return d;
        })
        .def("saveParamsTensor", &SLAMGaussianModel::saveParamsTensor)
        .def("saveParamsPly", &SLAMGaussianModel::saveParamsPly)
        .def("loadParamsTensor", &SLAMGaussianModel::loadParamsTensor)
        .def("forward", &SLAMGaussianModel::forward, py::arg("cam"), py::arg("ref_depth"), py::arg("base_color"))
        .def("rawForward", &SLAMGaussianModel::rawForward)
        .def("setBackgrounds", [](SLAMGaussianModel& s, c10::optional<torch::Tensor> bg) {
            s.backgrounds = bg.has_value() ? *bg : torch::Tensor();
        })
        .def_readwrite("render_method", &SLAMGaussianModel::render_method)
        .def_readwrite("ordered_raw_backward", &SLAMGaussianModel::ordered_raw_backward)
        .def("computeLoss", [](SLAMGaussianModel& s, TensorDict& r, const Camera& cam, const py::dict& w) {
            return s.computeLoss(r, cam, config_from_dict(w));
        })
        .def("computeLoss", [](SLAMGaussianModel& s, TensorDict& r, const Camera& cam, const gpsh::Node& weight_configs) {
            return s.computeLoss(r, cam, weight_configs);
        })
        .def("trainStep", [](SLAMGaussianModel& s, const Camera& cam, const torch::Tensor& ref_depth,
                             const torch::Tensor& base_color, c10::optional<torch::Tensor> clamped, const Camera* next_cam,
                             const py::dict& weights) {
            s.trainStep(cam, ref_depth, base_color, clamped.has_value() ? *clamped : torch::Tensor(), next_cam,
                        config_from_dict(weights));
        }, py::arg("cam"), py::arg("ref_depth"), py::arg("base_color"), py::arg("ref_depth_clamped") = py::none(),
             py::arg("next_cam") = (const Camera*)nullptr, py::arg("weight_configs") = py::dict())
        .def("reserveWorkspace", &SLAMGaussianModel::reserveWorkspace)
        .def("checkBinningCapacity", &SLAMGaussianModel::checkBinningCapacity)
        .def_readonly("binning_overflows", &SLAMGaussianModel::binning_overflows)
        .def("capacity", [](SLAMGaussianModel& s) { return s.getGaussianParms().capacity(); })
        .def("adamState", [](SLAMGaussianModel& s) { return s.adamState(); })
        .def("lossSum", &SLAMGaussianModel::lossSum)
        .def("lossTerms", &SLAMGaussianModel::lossTerms)
        .def("initOptimizers", &SLAMGaussianModel::initOptimizers, py::arg("max_iterations") = -1,
             py::arg("scene_scale") = 1.0f)
        .def("schedulersStep", &SLAMGaussianModel::schedulersStep)
        .def("hasScheduler", &SLAMGaussianModel::hasScheduler)
        .def("meansLr", &SLAMGaussianModel::meansLr)
        .def("adamStep", &SLAMGaussianModel::adamStep)
        .def("updateSH", &SLAMGaussianModel::updateSH, py::arg("curr_iter") = -1)
        .def_readwrite("maxSH", &SLAMGaussianModel::maxSH)
        .def_readwrite("shDegreeInterval", &SLAMGaussianModel::shDegreeInterval)
        .def_readonly("degreesToUse", &SLAMGaussianModel::degreesToUse)
        .def("optimizersStep", &SLAMGaussianModel::optimizersStep)
        .def("optimizersZeroGrad", &SLAMGaussianModel::optimizersZeroGrad)
        .def("prunePoints", &SLAMGaussianModel::prunePoints)
        .def("stepPostBackward", [](SLAMGaussianModel& s, TensorDict& r, const Camera& cam, float scene_scale, int curr_iter) {
            s.stepPostBackward(r, cam, scene_scale, curr_iter);
        }, py::arg("render_res"), py::arg("cam"), py::arg("scene_scale"), py::arg("curr_iter"))
        .def("updateDensifyGrad", [](SLAMGaussianModel& s, TensorDict& r, const Camera& cam) { s.updateDensifyGrad(r, cam); })
        .def("densifiyGs", [](SLAMGaussianModel& s, float scene_scale, int curr_iter, c10::optional<torch::Tensor> samples) {
            return s.densifiyGs(scene_scale, curr_iter, samples);
        }, py::arg("scene_scale"), py::arg("curr_iter"), py::arg("split_samples") = py::none())
        .def("resetOpacities", &SLAMGaussianModel::resetOpacities)
        .def("setDensifySeed", &SLAMGaussianModel::setDensifySeed)
        .def("densifyStats", &SLAMGaussianModel::densifyStats)
        .def("lastSplitSamples", &SLAMGaussianModel::lastSplitSamples)
        .def_readwrite("densify_start_iter", &SLAMGaussianModel::densify_start_iter)
        .def_readwrite("densify_end_iter", &SLAMGaussianModel::densify_end_iter)
        .def_readwrite("densify_interval", &SLAMGaussianModel::densify_interval)
        .def_readwrite("densify_grad_thres", &SLAMGaussianModel::densify_grad_thres)
        .def_readwrite("densify_large_thres", &SLAMGaussianModel::densify_large_thres)
        .def_readwrite("reset_opacity_interval", &SLAMGaussianModel::reset_opacity_interval)
        .def_readwrite("prune_opacity_thres", &SLAMGaussianModel::prune_opacity_thres)
        .def_readwrite("pause_refine_after_reset", &SLAMGaussianModel::pause_refine_after_reset)
        .def_readonly("densify_events", &SLAMGaussianModel::densify_events)
        .def_readonly("densify_log", &SLAMGaussianModel::densify_log)
        .def_readonly("opacity_reset_log", &SLAMGaussianModel::opacity_reset_log)
        .def("grads", &SLAMGaussianModel::grads)
        .def("leafGrads", &SLAMGaussianModel::leafGrads)
        .def("getExposure", &SLAMGaussianModel::getExposure)
        .def("exposureGrad", &SLAMGaussianModel::exposureGrad)
        .def("exposureAdamState", &SLAMGaussianModel::exposureAdamState)
        .def("exposureStep", &SLAMGaussianModel::exposureStep)
        .def_readonly("use_exposure", &SLAMGaussianModel::use_exposure)
        .def("getGaussianNum", &SLAMGaussianModel::getGaussianNum)
        .def("getGaussianParms", &SLAMGaussianModel::getGaussianParms, py::return_value_policy::reference_internal)
        .def("getRealScales", &SLAMGaussianModel::getRealScales)
        .def("getRealOpacities", &SLAMGaussianModel::getRealOpacities)
        .def("addGaussians", [](SLAMGaussianModel& s, const Camera& cam, const TensorDict& maps, const torch::Tensor& mask,
                                float ratio, int frame_num) { return s.addGaussians(cam, maps, mask, ratio, frame_num); });

    // ---- gpsh::RandomSelector / gpsh::OptimScheduler (random_selector.hpp): host code, no device
    py::class_<PySelector>(m, "RandomSelector")
        .def(py::init<std::vector<int64_t>, uint64_t>(), py::arg("items"), py::arg("seed"))
        .def("getNext", [](PySelector& s) {
            const auto e = s.sel.getNext();
            return std::make_pair(*e.value, e.originalIndex);   // (value, originalIndex)
        });
    py::class_<gpsh::OptimScheduler>(m, "OptimScheduler")
        .def(py::init<int>(), py::arg("max_iterations"))
        .def_readonly("active", &gpsh::OptimScheduler::active)
        .def_readonly("gamma", &gpsh::OptimScheduler::gamma)
        .def("step", [](const gpsh::OptimScheduler& s, double lr) { s.step(lr); return lr; }, py::arg("lr"));

    // ---- geometry / trajectory evaluation (geom_eval.hpp)
    py::class_<GeomEvalResult>(m, "GeomEvalResult")
        .def_readonly("accuracy_cm", &GeomEvalResult::accuracy_cm)
        .def_readonly("completion_cm", &GeomEvalResult::completion_cm)
        .def_readonly("dist_thres", &GeomEvalResult::dist_thres)
        .def_readonly("accuracy_ratio", &GeomEvalResult::accuracy_ratio)
        .def_readonly("completion_ratio", &GeomEvalResult::completion_ratio)
        .def_readonly("f1", &GeomEvalResult::f1)
        .def_readonly("n_rec", &GeomEvalResult::n_rec)
        .def_readonly("n_gt", &GeomEvalResult::n_gt);
    py::class_<AteResult>(m, "AteResult")
        .def_readonly("ate_mean_cm", &AteResult::ate_mean_cm)
        .def_readonly("ate_rmse_cm", &AteResult::ate_rmse_cm)
        .def_readonly("trans_error", &AteResult::trans_error)
        .def_readonly("rot", &AteResult::rot)
        .def_readonly("trans", &AteResult::trans);
    m.def("nearestDistances", [](const torch::Tensor& q, const torch::Tensor& r) { return nearestDistances(q, r); }, py::arg("query"), py::arg("ref"));
    m.def("nearestDistancesStats", [](const torch::Tensor& q, const torch::Tensor& r) {
        torch::Tensor stats;
        auto out = nearestDistances(q, r, &stats);
        return std::make_tuple(out.first, out.second, stats);
    }, py::arg("query"), py::arg("ref"));
    m.def("surfaceUniforms", &surfaceUniforms, py::arg("n"), py::arg("seed"));
    m.def("sampleSurface", [](const torch::Tensor& tri, int64_t n, uint64_t seed, const c10::optional<torch::Tensor>& u) {
        return sampleSurface(tri, n, seed, u ? *u : torch::Tensor());
    }, py::arg("triangles"), py::arg("n"), py::arg("seed") = 0, py::arg("uniforms") = py::none());
    m.def("evalPointClouds", [](const torch::Tensor& rec, const torch::Tensor& gt, const c10::optional<torch::Tensor>& T,
                                const std::vector<double>& th, int64_t sample_nums, uint64_t seed) {
        return evalPointClouds(rec, gt, T ? *T : torch::Tensor(), th, sample_nums, seed);
    }, py::arg("rec_points"), py::arg("gt_points"), py::arg("transform") = py::none(), py::arg("dist_thres") = std::vector<double>{0.03},
          py::arg("sample_nums") = 1000000, py::arg("seed") = 0);
    m.def("ate", &ate, py::arg("est_c2w"), py::arg("gt_c2w"));

    // ---- image evaluation (image_eval.hpp)
    py::class_<ImageMetrics>(m, "ImageMetrics")
        .def_readonly("psnr", &ImageMetrics::psnr)
        .def_readonly("ssim", &ImageMetrics::ssim)
        .def_readonly("mse", &ImageMetrics::mse)
        .def_readonly("sse_u8", &ImageMetrics::sse_u8)
        .def_readonly("psnr_mean", &ImageMetrics::psnr_mean)
        .def_readonly("ssim_mean", &ImageMetrics::ssim_mean);
    py::class_<ImageEvalResult>(m, "ImageEvalResult")
        .def_readonly("cam_ids", &ImageEvalResult::cam_ids)
        .def_readonly("psnr", &ImageEvalResult::psnr)
        .def_readonly("ssim", &ImageEvalResult::ssim)
        .def_readonly("psnr_mean", &ImageEvalResult::psnr_mean)
        .def_readonly("ssim_mean", &ImageEvalResult::ssim_mean)
        .def_readonly("metrics", &ImageEvalResult::metrics);
    m.def("imageMetrics", [](const torch::Tensor& render, const torch::Tensor& gt, const c10::optional<torch::Tensor>& depth) {
        return imageMetrics(render, gt, depth ? *depth : torch::Tensor());
    }, py::arg("render"), py::arg("gt"), py::arg("depth") = py::none());

    // ---- failure modes (ITMLibSettings::behaviourOnFailure, ITMTrackingState::TrackingResult) and what the engine does with a verdict
    py::enum_<ITMLib::ITMLibSettings::FailureMode>(m, "FailureMode")
        .value("FAILUREMODE_RELOCALISE", ITMLib::ITMLibSettings::FAILUREMODE_RELOCALISE)
        .value("FAILUREMODE_IGNORE", ITMLib::ITMLibSettings::FAILUREMODE_IGNORE)
        .value("FAILUREMODE_STOP_INTEGRATION", ITMLib::ITMLibSettings::FAILUREMODE_STOP_INTEGRATION);
    py::enum_<ITMTrackingState::TrackingResult>(m, "TrackingResult")
        .value("TRACKING_GOOD", ITMTrackingState::TRACKING_GOOD)
        .value("TRACKING_POOR", ITMTrackingState::TRACKING_POOR)
        .value("TRACKING_FAILED", ITMTrackingState::TRACKING_FAILED);
    m.def("failureModeFromString", &ITMLib::ITMLibSettings::failureModeFromString);
    // ---- ITMMainEngine::GetImageType and what GetImage does with it (tsdf_engine.hpp, decideOnGetImage)
    {
        typedef ITMLib::ITMMainEngineTypes T;
        py::enum_<T::GetImageType>(m, "GetImageType")
            .value("InfiniTAM_IMAGE_ORIGINAL_RGB", T::InfiniTAM_IMAGE_ORIGINAL_RGB)
            .value("InfiniTAM_IMAGE_ORIGINAL_DEPTH", T::InfiniTAM_IMAGE_ORIGINAL_DEPTH)
            .value("InfiniTAM_IMAGE_SCENERAYCAST", T::InfiniTAM_IMAGE_SCENERAYCAST)
            .value("InfiniTAM_IMAGE_COLOUR_FROM_VOLUME", T::InfiniTAM_IMAGE_COLOUR_FROM_VOLUME)
            .value("InfiniTAM_IMAGE_COLOUR_FROM_NORMAL", T::InfiniTAM_IMAGE_COLOUR_FROM_NORMAL)
            .value("InfiniTAM_IMAGE_COLOUR_FROM_CONFIDENCE", T::InfiniTAM_IMAGE_COLOUR_FROM_CONFIDENCE)
            .value("InfiniTAM_IMAGE_FREECAMERA_SHADED", T::InfiniTAM_IMAGE_FREECAMERA_SHADED)
            .value("InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME", T::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME)
            .value("InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL", T::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL)
            .value("InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_CONFIDENCE", T::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_CONFIDENCE)
            .value("InfiniTAM_IMAGE_UNKNOWN", T::InfiniTAM_IMAGE_UNKNOWN);
        py::enum_<ITMLib::GetImageDecision::RaySource>(m, "GetImageRaySource")
            .value("RAYS_NONE", ITMLib::GetImageDecision::RAYS_NONE)
            .value("RAYS_LIVE_RAYCAST", ITMLib::GetImageDecision::RAYS_LIVE_RAYCAST)
            .value("RAYS_FORWARD_PROJECTION", ITMLib::GetImageDecision::RAYS_FORWARD_PROJECTION)
            .value("RAYS_FREE_RAYCAST", ITMLib::GetImageDecision::RAYS_FREE_RAYCAST);
        py::enum_<ITMLib::GetImageDecision::OutSource>(m, "GetImageOutSource")
            .value("OUT_CLEARED", ITMLib::GetImageDecision::OUT_CLEARED)
            .value("OUT_RGB", ITMLib::GetImageDecision::OUT_RGB)
            .value("OUT_DEPTH_COLOUR", ITMLib::GetImageDecision::OUT_DEPTH_COLOUR)
            .value("OUT_LIVE_RENDER", ITMLib::GetImageDecision::OUT_LIVE_RENDER)
            .value("OUT_KF_RAYCAST", ITMLib::GetImageDecision::OUT_KF_RAYCAST)
            .value("OUT_FREE_RENDER", ITMLib::GetImageDecision::OUT_FREE_RENDER);
        py::class_<ITMLib::GetImageDecision>(m, "GetImageDecision")
            .def_readonly("renderType", &ITMLib::GetImageDecision::renderType)
            .def_readonly("rays", &ITMLib::GetImageDecision::rays)
            .def_readonly("out", &ITMLib::GetImageDecision::out);
        m.def("decideOnGetImage", &ITMLib::decideOnGetImage, py::arg("type"), py::arg("age_pointCloud"), py::arg("relocalisationCount"));
    }
    py::class_<ITMLib::FailureDecision>(m, "FailureDecision")
        .def_readonly("result", &ITMLib::FailureDecision::result)
        .def_readonly("useRelocaliser", &ITMLib::FailureDecision::useRelocaliser)
        .def_readonly("harvest", &ITMLib::FailureDecision::harvest)
        .def_readonly("relocalise", &ITMLib::FailureDecision::relocalise)
        .def_readonly("fuse", &ITMLib::FailureDecision::fuse)
        .def_readonly("refreshAndRaycast", &ITMLib::FailureDecision::refreshAndRaycast)
        .def_readonly("relocalisationCount", &ITMLib::FailureDecision::relocalisationCount);
    m.def("decideOnTrackingResult", &ITMLib::decideOnTrackingResult, py::arg("mode"), py::arg("trackerVerdict"), py::arg("addedKeyframe"),
          py::arg("relocalisationCount"), py::arg("trackingInitialised"), py::arg("fusionActive"), py::arg("relocalised") = false);
    py::class_<ITMLib::PoseQualityThresholds>(m, "PoseQualityThresholds")
        .def(py::init<>())
        .def_readwrite("enabled", &ITMLib::PoseQualityThresholds::enabled)
        .def_readwrite("poorScore", &ITMLib::PoseQualityThresholds::poorScore)
        .def_readwrite("poorInlierShare", &ITMLib::PoseQualityThresholds::poorInlierShare)
        .def_readwrite("failedScore", &ITMLib::PoseQualityThresholds::failedScore)
        .def_readwrite("failedInlierShare", &ITMLib::PoseQualityThresholds::failedInlierShare);
    m.def("poseQualityVerdict", &ITMLib::poseQualityVerdict, py::arg("thresholds"), py::arg("score"), py::arg("inlierShare"));
    // ---- FernRelocLib::Relocaliser<float> over the device relocaliser (host/relocaliser.hpp); frames on the current stream
    py::class_<FernRelocLib::Relocaliser<float>>(m, "Relocaliser")
        .def(py::init<int, int, float, float, float, int, int, int, uint64_t>(), py::arg("width"), py::arg("height"), py::arg("rangeMin"),
             py::arg("rangeMax"), py::arg("harvestingThreshold") = 0.2f, py::arg("numFerns") = 500, py::arg("numDecisionsPerFern") = 4,
             py::arg("capacity") = 4096, py::arg("seed") = 0)
        .def("ProcessFrame", [](FernRelocLib::Relocaliser<float>& r, const torch::Tensor& depth, const torch::Tensor& pose, int sceneId, int k,
                                bool harvest) {
            TORCH_CHECK(depth.is_cuda() && depth.scalar_type() == torch::kFloat32 && depth.is_contiguous(), "depth must be a contiguous float32 device tensor");
            auto p = pose.to(torch::kCPU, torch::kFloat32).contiguous();
            TORCH_CHECK(p.numel() == 32, "pose must be [2,16] (M, invM)");
            r.ProcessFrame(depth.data_ptr<float>(), p.data_ptr<float>(), p.data_ptr<float>() + 16, sceneId, k, harvest, gpsh::current_stream());
        }, py::arg("depth"), py::arg("pose"), py::arg("sceneId") = 0, py::arg("k") = 1, py::arg("harvestKeyframes") = true)
        .def("ReadResult", [](FernRelocLib::Relocaliser<float>& r) {
            const gps_reloc_result x = r.ReadResult(gpsh::current_stream());
            py::dict d;
            d["added_id"] = x.added_id; d["n_found"] = x.n_found; d["n_entries"] = x.n_entries; d["overflow"] = x.overflow;
            d["ids"] = std::vector<int>(x.ids, x.ids + 4); d["distances"] = std::vector<float>(x.distances, x.distances + 4);
            return d;
        })
        .def("RetrievePose", [](FernRelocLib::Relocaliser<float>& r, int id) {
            const FernRelocLib::PoseInScene p = r.RetrievePose(id, gpsh::current_stream());
            auto t = torch::empty({2, 16}, torch::kFloat32);
            for (int i = 0; i < 16; i++) { t[0][i] = p.M[i]; t[1][i] = p.invM[i]; }
            return std::make_pair(t, p.sceneIdx);
        })
        .def("numEntries", [](FernRelocLib::Relocaliser<float>& r) { return r.numEntries(gpsh::current_stream()); })
        .def("SaveToDirectory", [](FernRelocLib::Relocaliser<float>& r, const std::string& d) { r.SaveToDirectory(d, gpsh::current_stream()); })
        .def("LoadFromDirectory", [](FernRelocLib::Relocaliser<float>& r, const std::string& d) { r.LoadFromDirectory(d, gpsh::current_stream()); });
    // the text formats alone, host code: read a database directory and write it again (both names end in '/')
    m.def("relocDatabaseRewrite", [](const std::string& in, const std::string& out, int numFerns, int numDecisions, float threshold) {
        const auto db = FernRelocLib::detail::readDatabase(in, numFerns, numDecisions, threshold);
        FernRelocLib::detail::writeDatabase(db, out);
        return db.totalEntries;
    });
    m.def("relocPoseFromParams", [](const std::vector<float>& p) {
        TORCH_CHECK(p.size() == 6, "six SE3 parameters");
        auto t = torch::empty({2, 16}, torch::kFloat32);
        FernRelocLib::detail::poseFromParams(p.data(), t.data_ptr<float>(), t.data_ptr<float>() + 16);
        return t;
    });
    m.def("relocParamsFromPose", [](const torch::Tensor& M) {
        auto m_ = M.to(torch::kCPU, torch::kFloat32).contiguous();
        TORCH_CHECK(m_.numel() >= 16, "M: 16 floats, ORUtils layout");
        std::vector<float> p(6);
        FernRelocLib::detail::paramsFromPose(m_.data_ptr<float>(), p.data());
        return p;
    });
    m.def("tsdfConfigFailureMode", [](const gpsh::Node& tsdf_node) {
        // the failure mode createTsdfEngine takes from a PIPE.TSDF node: the absent key is ignore, an unknown value throws
        TsdfConfig t;
        const gpsh::Config c = gpsh::flattenNode(tsdf_node, "PIPE.TSDF", [&](auto& v) { t.configFields(v); });
        gpsh::ConfigReader reader{c};
        t.configFields(reader);
        return ITMLib::ITMLibSettings::failureModeFromString(t.failure_mode);
    });
    m.def("tsdfConfigUseApproximateRaycast", [](const gpsh::Node& tsdf_node) {
        // what createTsdfEngine takes from a PIPE.TSDF node: the absent key is false, a misspelt key is an unknown key
        TsdfConfig t;
        const gpsh::Config c = gpsh::flattenNode(tsdf_node, "PIPE.TSDF", [&](auto& v) { t.configFields(v); });
        gpsh::ConfigReader reader{c};
        t.configFields(reader);
        return t.use_approximate_raycast;
    });
    m.def("tsdfConfigUseBilateralFilter", [](const gpsh::Node& tsdf_node) {
        // the same for TSDF.use_bilateral_filter: the absent key is false, a value that is no boolean throws
        TsdfConfig t;
        const gpsh::Config c = gpsh::flattenNode(tsdf_node, "PIPE.TSDF", [&](auto& v) { t.configFields(v); });
        gpsh::ConfigReader reader{c};
        t.configFields(reader);
        return t.use_bilateral_filter;
    });
    m.def("tsdfConfigUseBilateralFilterFlat", [](const py::dict& flat) {
        // the flat route: the gpsh::Config createTsdfEngine(data_reader, config) reads (config.flatten's dict)
        const gpsh::Config c = config_from_dict(flat);
        TsdfConfig t;
        gpsh::ConfigReader reader{c};
        t.configFields(reader);
        return t.use_bilateral_filter;
    });

    // ---- ITMRGBDCalib and the calib.txt of ITMCalibIO.cpp
    py::class_<ITMLib::ITMRGBDCalib>(m, "ITMRGBDCalib")
        .def(py::init<>())
        .def("setIntrinsicsRgb", [](ITMLib::ITMRGBDCalib& c, int w, int h, float fx, float fy, float cx, float cy) { c.intrinsics_rgb.SetFrom(w, h, fx, fy, cx, cy); })
        .def("setIntrinsicsD", [](ITMLib::ITMRGBDCalib& c, int w, int h, float fx, float fy, float cx, float cy) { c.intrinsics_d.SetFrom(w, h, fx, fy, cx, cy); })
        .def("setExtrinsics", [](ITMLib::ITMRGBDCalib& c, const std::vector<float>& calib16) {   // ORUtils layout
            TORCH_CHECK(calib16.size() == 16, "setExtrinsics: 16 values in ORUtils layout");
            ITMLib::Matrix4f m;
            for (int i = 0; i < 16; i++) m.m[i] = calib16[i];
            c.trafo_rgb_to_depth.SetFrom(m);
        })
        .def("setDisparityCalib", [](ITMLib::ITMRGBDCalib& c, float a, float b, int type) {
            TORCH_CHECK(type == 0 || type == 1, "setDisparityCalib: type is 0 (Kinect) or 1 (affine)");
            c.disparityCalib.SetFrom(a, b, (ITMLib::ITMDisparityCalib::TrafoType)type);
        })
        .def("intrinsicsRgb", [](const ITMLib::ITMRGBDCalib& c) {
            const auto& k = c.intrinsics_rgb;
            return py::make_tuple(k.imgSize.x, k.imgSize.y, k.projectionParamsSimple.fx, k.projectionParamsSimple.fy, k.projectionParamsSimple.px, k.projectionParamsSimple.py);
        })
        .def("intrinsicsD", [](const ITMLib::ITMRGBDCalib& c) {
            const auto& k = c.intrinsics_d;
            return py::make_tuple(k.imgSize.x, k.imgSize.y, k.projectionParamsSimple.fx, k.projectionParamsSimple.fy, k.projectionParamsSimple.px, k.projectionParamsSimple.py);
        })
        .def("calib", [](const ITMLib::ITMRGBDCalib& c) { return std::vector<float>(c.trafo_rgb_to_depth.calib.m, c.trafo_rgb_to_depth.calib.m + 16); })
        .def("calibInv", [](const ITMLib::ITMRGBDCalib& c) { return std::vector<float>(c.trafo_rgb_to_depth.calib_inv.m, c.trafo_rgb_to_depth.calib_inv.m + 16); })
        .def("disparityCalib", [](const ITMLib::ITMRGBDCalib& c) {
            return py::make_tuple((int)c.disparityCalib.GetType(), c.disparityCalib.GetParams().x, c.disparityCalib.GetParams().y);
        })
        // M_rgb = calib_inv * M_d as the integration entry forms it (gps_rgbd_m_rgb)
        .def("mRgb", [](const ITMLib::ITMRGBDCalib& c, const std::vector<float>& M_d) {
            TORCH_CHECK(M_d.size() == 16, "mRgb: 16 values in ORUtils layout");
            std::vector<float> out(16);
            gpsh::check(gps_rgbd_m_rgb(c.trafo_rgb_to_depth.calib_inv.m, M_d.data(), out.data()), "gps_rgbd_m_rgb");
            return out;
        });
    m.def("readRGBDCalib", [](const std::string& path) {
        ITMLib::ITMRGBDCalib c;
        TORCH_CHECK(ITMLib::readRGBDCalib(path.c_str(), c), "readRGBDCalib: cannot read ", path);
        return c;
    });
    m.def("parseRGBDCalib", [](const std::string& text) {
        ITMLib::ITMRGBDCalib c;
        std::stringstream src(text);
        TORCH_CHECK(ITMLib::readRGBDCalib(src, c), "readRGBDCalib: cannot read the text");
        return c;
    });
    m.def("writeRGBDCalib", [](const std::string& path, const ITMLib::ITMRGBDCalib& c) { ITMLib::writeRGBDCalib(path.c_str(), c); });
    m.def("formatRGBDCalib", [](const ITMLib::ITMRGBDCalib& c) {
        std::stringstream dest;
        ITMLib::writeRGBDCalib(dest, c);
        return dest.str();
    });
    // colour registered to the depth camera (gps_tsdf_register_colour; ours): depth float [Hd, Wd] metres, the depth intrinsics
    // (fx, fy, cx, cy), the calibration's colour camera and extrinsics, rgb uint8 [Hc, Wc, 4] -> uint8 [Hd, Wd, 4]
    m.def("registerColour", &registerColour);

    // ---- TSDF engine
    py::class_<TsdfEngine>(m, "ITMBasicEngine")
        // ITMBasicEngine(settings, calib, imgSize_rgb, imgSize_d) with the full calibration: the sizes are the calibration's
        .def(py::init([](const ITMLib::ITMRGBDCalib& calib, float voxel_size, float mu, float vmin, float vmax) -> TsdfEngine* {
                 ITMLib::ITMLibSettings settings;
                 settings.sceneParams.voxelSize = voxel_size; settings.sceneParams.mu = mu;
                 settings.sceneParams.viewFrustum_min = vmin; settings.sceneParams.viewFrustum_max = vmax;
                 return new ITMLib::ITMBasicEngine<ITMVoxel, ITMVoxelIndex>(&settings, calib, calib.intrinsics_rgb.imgSize, calib.intrinsics_d.imgSize);
             }),
             py::arg("calib"), py::arg("voxel_size") = 0.005f, py::arg("mu") = 0.02f, py::arg("view_frustum_min") = 0.2f,
             py::arg("view_frustum_max") = 10.0f)
        .def("hasCalibration", &TsdfEngine::hasCalibration)
        .def("registeredColour", &TsdfEngine::registeredColour)
        .def("rgbImageSize", [](TsdfEngine& e) { const Vector2i s = e.GetRGBImageSize(); return py::make_tuple(s.x, s.y); })
        .def(py::init([](int w, int h, float fx, float fy, float cx, float cy, float voxel_size, float mu, float vmin,
                         float vmax) { return new TsdfEngine(w, h, fx, fy, cx, cy, voxel_size, mu, vmin, vmax); }),
             py::arg("width"), py::arg("height"), py::arg("fx"), py::arg("fy"), py::arg("cx"), py::arg("cy"),
             py::arg("voxel_size") = 0.005f, py::arg("mu") = 0.02f, py::arg("view_frustum_min") = 0.2f,
             py::arg("view_frustum_max") = 10.0f)
        .def("pushGtPose", [](TsdfEngine& e, const torch::Tensor& c2w) { e.gtC2wPoses.push_back(c2w); })
        .def("turnOffTracking", &TsdfEngine::turnOffTracking)
        .def("turnOnTracking", [](TsdfEngine& e) { e.turnOnTracking(); })
        .def("setBarArgLine", &TsdfEngine::setBarArgLine)
        .def("usesBarArgLine", &TsdfEngine::usesBarArgLine)
        .def("setPosesRidingAlong", &TsdfEngine::setPosesRidingAlong)
        .def("posesRidingAlong", &TsdfEngine::posesRidingAlong)
        .def("setHostSummedRows", &TsdfEngine::setHostSummedRows)
        .def("hostSummedRows", &TsdfEngine::hostSummedRows)
        .def("ridingAlongStats", &TsdfEngine::ridingAlongStats)
        .def("trackerTotals", &TsdfEngine::trackerTotals)
        .def("lastPose", [](TsdfEngine& e) {
            auto t = torch::empty({2, 16}, torch::kFloat32);
            const ORUtils::SE3Pose& p = e.camPoses.back();
            for (int i = 0; i < 16; i++) { t[0][i] = p.GetM()[i]; t[1][i] = p.GetInvM()[i]; }
            return t;
        })
        .def("trackDiag", [](TsdfEngine& e) {
            auto t = torch::empty({16}, torch::kFloat32);
            for (int i = 0; i < 16; i++) t[i] = e.trackState().diag[i];
            return t;
        })
        .def("trackPollProfile", &TsdfEngine::trackPollProfile)
        .def("ProcessFrame", [](TsdfEngine& e, const torch::Tensor& rgb, const torch::Tensor& depth) {
            e.ProcessFrame(rgb, depth);
        })
        .def("setFailureMode", &TsdfEngine::setFailureMode)
        .def("failureMode", &TsdfEngine::failureMode)
        .def("setPoseQualityThresholds", &TsdfEngine::setPoseQualityThresholds)
        .def("forceTrackerResult", &TsdfEngine::forceTrackerResult, py::arg("frame"), py::arg("result"))
        .def("clearForcedTrackerResults", &TsdfEngine::clearForcedTrackerResults)
        .def("trackerResult", [](TsdfEngine& e) { return e.GetTrackingState()->trackerResult; })
        .def("lastFrameFused", &TsdfEngine::lastFrameFused)
        .def("inlierShare", [](TsdfEngine& e) {
            // of the last TrackCamera: inliers of the last accepted evaluation over the valid depth pixels (0 before the first)
            const int n = e.trackState().n_valid_max;
            return n > 0 ? e.trackState().diag[8] / (float)n : 0.0f;
        })
        .def("hasRelocaliser", [](TsdfEngine& e) { return e.relocaliser() != nullptr; })
        .def("relocaliserEntries", [](TsdfEngine& e) { return e.relocaliser() ? e.relocaliser()->numEntries(gpsh::current_stream()) : 0; })
        .def("relocaliserPose", [](TsdfEngine& e, int id) {
            TORCH_CHECK(e.relocaliser() != nullptr, "relocaliserPose: no relocaliser (failure mode is not relocalise, or no frame yet)");
            const FernRelocLib::PoseInScene p = e.relocaliser()->RetrievePose(id, gpsh::current_stream());
            auto t = torch::empty({2, 16}, torch::kFloat32);
            for (int i = 0; i < 16; i++) { t[0][i] = p.M[i]; t[1][i] = p.invM[i]; }
            return t;
        })
        .def("convertDepth", &TsdfEngine::convertDepth)
        .def("relocaliseFromPose", [](TsdfEngine& e, const torch::Tensor& pose) {
            auto p = pose.to(torch::kCPU, torch::kFloat32).contiguous();
            TORCH_CHECK(p.numel() == 32, "relocaliseFromPose: pose must be [2,16] (M, invM)");
            e.relocaliseFromPose(p.data_ptr<float>(), p.data_ptr<float>() + 16);
            auto t = torch::empty({2, 16}, torch::kFloat32);
            for (int i = 0; i < 16; i++) { t[0][i] = e.trackState().pose_M[i]; t[1][i] = e.trackState().pose_invM[i]; }
            return t;
        })
        .def("visibleIds", [](TsdfEngine& e) {
            // the live visible list: hash-slot ids of the blocks the last frame saw (host-synchronous; tests)
            auto c = e.counters().cpu();
            const int n = c.data_ptr<int32_t>()[GPS_TSDF_N_VISIBLE];
            return torch::from_blob(e.state().visible_ids, {n}, torch::TensorOptions().dtype(torch::kInt32).device(e.counters().device())).clone();
        })
        .def("allocatedSlots", [](TsdfEngine& e) {
            // hash-slot ids that hold an allocated block (ptr >= 0), ascending (host-synchronous; tests)
            const int64_t n_total = (int64_t)e.state().n_buckets + e.state().n_excess;
            auto h = torch::from_blob(e.state().hash, {n_total, 4}, torch::TensorOptions().dtype(torch::kInt32).device(e.counters().device()));
            return torch::nonzero(h.select(1, 3) >= 0).reshape({-1}).to(torch::kInt32);
        })
        .def_readwrite("trackingInitialised", &TsdfEngine::trackingInitialised)
        .def_readonly("relocalisationCount", &TsdfEngine::relocalisationCount)
        .def_readonly("framesSeen", &TsdfEngine::framesSeen)
        .def_readonly("lastRelocalisedTo", &TsdfEngine::lastRelocalisedTo)
        .def("runRaycastC2w", [](TsdfEngine& e, const torch::Tensor& c2w) {
            ORUtils::SE3Pose pose;
            auto c = c2w.to(torch::kCPU, torch::kFloat32).contiguous();
            pose.SetInvM(c.data_ptr<float>());
            e.runRaycast(&pose);
        })
        .def("GetFreeImage", [](TsdfEngine& e) { return e.GetFreeImage()->tensor(); })
        .def("GetFreeVertex", [](TsdfEngine& e) { return e.GetFreeVertex()->tensor(); })
        .def("GetLiveVertex", [](TsdfEngine& e) { return e.GetLiveVertex()->tensor(); })
        // ---- approximate raycast (ITMLibSettings::useApproximateRaycast) and the live re-render, runRaycast(NULL, NULL)
        .def("setUseApproximateRaycast", &TsdfEngine::setUseApproximateRaycast)
        .def("usesApproximateRaycast", &TsdfEngine::usesApproximateRaycast)
        .def("resetAll", &TsdfEngine::resetAll)
        .def("setUseBilateralFilter", &TsdfEngine::setUseBilateralFilter)   // ITMLibSettings::useBilateralFilter
        .def("usesBilateralFilter", &TsdfEngine::usesBilateralFilter)
        .def("hasFilterScratch", &TsdfEngine::hasFilterScratch)
        .def("stateTensors", [](TsdfEngine& e) {
            // views (no copies) of the engine's device state under the names of gps_tsdf_state, for tests that digest it
            const gps_tsdf_state& s = e.state();
            const auto dev = e.counters().device();
            const int64_t P = (int64_t)s.width * s.height, n_total = (int64_t)s.n_buckets + s.n_excess;
            auto view = [&](void* p, int64_t n, torch::ScalarType t) {
                return torch::from_blob(p, {n}, torch::TensorOptions().dtype(t).device(dev));
            };
            py::dict d;
            d["vba"] = view(s.vba, (int64_t)s.n_blocks * 512 * 8, torch::kUInt8);
            d["hash"] = view(s.hash, n_total * 16, torch::kUInt8);
            d["counters"] = e.counters();
            d["visible_type"] = view(s.visible_type, n_total, torch::kUInt8);
            d["visible_ids"] = view(s.visible_ids, s.n_blocks, torch::kInt32);
            d["depth"] = view(s.depth, P, torch::kFloat32);
            d["minmax"] = view(s.minmax, P * 2, torch::kFloat32);
            d["raycast"] = view(s.raycast, P * 4, torch::kFloat32);
            d["icp_points"] = view(s.icp_points, P * 4, torch::kFloat32);
            d["icp_normals"] = view(s.icp_normals, P * 4, torch::kFloat32);
            return d;
        })
        .def("agePointCloud", &TsdfEngine::agePointCloud)
        .def("runRaycast", [](TsdfEngine& e) { e.runRaycast(nullptr, nullptr); })
        .def("GetLiveImage", &TsdfEngine::GetLiveImage)
        .def("GetForwardProjection", &TsdfEngine::GetForwardProjection)
        .def("forwardMissingPoints", &TsdfEngine::forwardMissingPoints)
        // ---- ITMBasicEngine::GetImage: the type by name ("InfiniTAM_IMAGE_SCENERAYCAST" or "SCENERAYCAST"), enumerator or value;
        // c2w (and optionally fx, fy, cx, cy) for the free-camera types.  -> uint8 [H, W, 4] device tensor, None before the first frame
        .def("GetImage", [](TsdfEngine& e, const py::object& type, const c10::optional<torch::Tensor>& c2w,
                            const c10::optional<std::vector<float>>& intrinsics, bool to_host) -> py::object {
            typedef ITMLib::ITMMainEngineTypes T;
            T::GetImageType t;
            if (py::isinstance<py::str>(type)) {
                std::string name = type.cast<std::string>();
                if (name.rfind("InfiniTAM_IMAGE_", 0) != 0) name = "InfiniTAM_IMAGE_" + name;
                const py::dict members = py::cast(T::InfiniTAM_IMAGE_UNKNOWN).get_type().attr("__members__");
                TORCH_CHECK(members.contains(name.c_str()), "GetImage: unknown image type '", name, "'");
                t = members[name.c_str()].cast<T::GetImageType>();
            } else if (py::isinstance<T::GetImageType>(type)) {
                t = type.cast<T::GetImageType>();
            } else {
                const int v = type.cast<int>();
                TORCH_CHECK(v >= 0 && v <= (int)T::InfiniTAM_IMAGE_UNKNOWN, "GetImage: image type ", v, " out of range");
                t = (T::GetImageType)v;
            }
            ORUtils::SE3Pose pose;
            ITMLib::ITMIntrinsics in;
            if (c2w) { auto c = c2w->to(torch::kCPU, torch::kFloat32).contiguous(); pose.SetInvM(c.data_ptr<float>()); }
            if (intrinsics) {
                TORCH_CHECK(intrinsics->size() == 4, "GetImage: intrinsics are (fx, fy, cx, cy)");
                in.SetFrom(e.state().width, e.state().height, (*intrinsics)[0], (*intrinsics)[1], (*intrinsics)[2], (*intrinsics)[3]);
            }
            if (to_host) {   // the reference's signature: into a caller's host image (synchronous)
                // (the original colour image has the colour camera's size)
                const Vector2i dims = t == T::InfiniTAM_IMAGE_ORIGINAL_RGB ? e.GetRGBImageSize() : Vector2i(e.state().width, e.state().height);
                ITMUChar4Image img(dims, true, false);
                std::memset(img.GetData(MEMORYDEVICE_CPU), 0xAB, img.dataSize() * 4);   // (shows an image left untouched)
                e.GetImage(&img, t, c2w ? &pose : nullptr, intrinsics ? &in : nullptr);
                return py::cast(img.host_tensor().clone().view({dims.y, dims.x, 4}));
            }
            torch::Tensor r = e.getImageTensor(t, c2w ? &pose : nullptr, intrinsics ? &in : nullptr);
            return r.defined() ? py::cast(r) : py::none();
        }, py::arg("image_type"), py::arg("c2w") = py::none(), py::arg("intrinsics") = py::none(), py::arg("to_host") = false)
        .def("getVoxelSize", &TsdfEngine::getVoxelSize)
        .def("counters", &TsdfEngine::counters)
        .def("MeshScene", &TsdfEngine::MeshScene, py::arg("maxTriangles") = (int64_t)1 << 24)
        .def("EvalMesh", [](TsdfEngine& e, const torch::Tensor& gt, const c10::optional<torch::Tensor>& T, const std::vector<double>& th,
                            int64_t sample_nums, uint64_t seed, int64_t m) {
            return e.EvalMesh(gt, T ? *T : torch::Tensor(), th, sample_nums, seed, m);
        }, py::arg("gt_points_or_triangles"), py::arg("transform") = py::none(), py::arg("dist_thres") = std::vector<double>{0.03},
             py::arg("sample_nums") = 1000000, py::arg("seed") = 0, py::arg("maxTriangles") = (int64_t)1 << 24)
        .def("SaveSceneToMesh", [](TsdfEngine& e, const std::string& f, int64_t m) { return e.SaveSceneToMesh(f.c_str(), m); },
             py::arg("fileName"), py::arg("maxTriangles") = (int64_t)1 << 24)
        .def("SaveToFile", &TsdfEngine::SaveToFile)
        .def("LoadFromFile", &TsdfEngine::LoadFromFile)
        .def("runRaycastIntrinsics", [](TsdfEngine& e, const torch::Tensor& c2w, float fx, float fy, float cx, float cy) {
            // ITMBasicEngine::runRaycast(pose, intrinsics) with an explicit ITMIntrinsics (slam_pipeline.cpp:367-376)
            ORUtils::SE3Pose pose;
            auto c = c2w.to(torch::kCPU, torch::kFloat32).contiguous();
            pose.SetInvM(c.data_ptr<float>());
            ITMLib::ITMIntrinsics in;
            in.SetFrom(e.state().width, e.state().height, fx, fy, cx, cy);
            e.runRaycast(&pose, &in);
        })
        .def("camIntrincs", [](TsdfEngine& e) {
            auto t = torch::empty({(int64_t)e.camIntrincs.size(), 4}, torch::kFloat32);
            for (size_t i = 0; i < e.camIntrincs.size(); i++) {
                const auto& p = e.camIntrincs[i].projectionParamsSimple;
                t[i][0] = p.fx; t[i][1] = p.fy; t[i][2] = p.px; t[i][3] = p.py;
            }
            return t;
        })
        .def_readonly("framesProcessed", &TsdfEngine::framesProcessed);

    // ---- the reference's construction path: DatasetReader -> createTsdfEngine -> CLIEngine (slam_trainer.cpp:20-33)
    py::class_<DatasetReader>(m, "DatasetReader")
        .def(py::init([](int w, int h, float fx, float fy, float cx, float cy) {
            auto* r = new DatasetReader();
            r->width = w; r->height = h; r->fx = fx; r->fy = fy; r->cx = cx; r->cy = cy;
            return r;
        }))
        .def(py::init<>())
        .def("loadConfig", [](DatasetReader& r, const gpsh::Node& reader_node) { r.loadConfig(reader_node); })
        .def_readwrite("width", &DatasetReader::width)
        .def_readwrite("height", &DatasetReader::height)
        .def_readwrite("fx", &DatasetReader::fx)
        .def_readwrite("fy", &DatasetReader::fy)
        .def_readwrite("cx", &DatasetReader::cx)
        .def_readwrite("cy", &DatasetReader::cy)
        .def_readwrite("scene_scale", &DatasetReader::scene_scale)
        .def_readwrite("depth_scale", &DatasetReader::depth_scale)
        .def("addTrainCamera", [](DatasetReader& r, const Camera& c) { r.train_vec.push_back(c); })
        .def("trainCameras", [](DatasetReader& r) { return r.train_vec; })   // copies (c2w_slam: the poses the last session estimated)
        .def("size", [](DatasetReader& r) { return r.train_vec.size(); });
    py::class_<InfiniTAM::Engine::CLIEngine, std::unique_ptr<InfiniTAM::Engine::CLIEngine, py::nodelete>>(m, "CLIEngine")
        .def("ProcessFrame", &InfiniTAM::Engine::CLIEngine::ProcessFrame)
        .def("Shutdown", &InfiniTAM::Engine::CLIEngine::Shutdown)
        .def("GetDepthSize", [](InfiniTAM::Engine::CLIEngine& e) { auto d = e.GetDepthSize(); return std::make_pair(d.x, d.y); })
        .def("GetRGBSize", [](InfiniTAM::Engine::CLIEngine& e) { auto d = e.GetRGBSize(); return std::make_pair(d.x, d.y); })
        .def("getMainEngine", [](InfiniTAM::Engine::CLIEngine& e) {
            return static_cast<TsdfEngine*>(dynamic_cast<ITMLib::ITMBasicEngine<ITMVoxel, ITMVoxelIndex>*>(e.getMainEngine()));
        }, py::return_value_policy::reference)
        .def_readwrite("prefetch", &InfiniTAM::Engine::CLIEngine::prefetch)
        .def_readonly("uploadedBytes", &InfiniTAM::Engine::CLIEngine::uploadedBytes)
        .def_readonly("currentFrameNo", &InfiniTAM::Engine::CLIEngine::currentFrameNo);
    m.def("createTsdfEngine", [](const DatasetReader& r, const py::dict& cfg) { return createTsdfEngine(r, config_from_dict(cfg)); },
          py::return_value_policy::reference);
    m.def("createTsdfEngine", [](const DatasetReader& r, const gpsh::Node& tsdf_node) { return createTsdfEngine(r, tsdf_node); },
          py::return_value_policy::reference);

    // ---- pipeline
    py::class_<SLAMPipeline::PipelineTimes>(m, "PipelineTimes")
        .def_readonly("frames", &SLAMPipeline::PipelineTimes::frames)
        .def_readonly("slam_total", &SLAMPipeline::PipelineTimes::slam_total)
        .def_readonly("per_frame", &SLAMPipeline::PipelineTimes::per_frame)
        .def_readonly("keyframe_step", &SLAMPipeline::PipelineTimes::keyframe_step)
        .def_readonly("localFrameRaycast", &SLAMPipeline::PipelineTimes::localFrameRaycast)
        .def_readonly("keyFrameRaycast", &SLAMPipeline::PipelineTimes::keyFrameRaycast)
        .def_readonly("initNewGaussians", &SLAMPipeline::PipelineTimes::initNewGaussians)
        .def_readonly("localOptimize", &SLAMPipeline::PipelineTimes::localOptimize)
        .def_readonly("removeGaussian", &SLAMPipeline::PipelineTimes::removeGaussian)
        .def_readonly("checkError", &SLAMPipeline::PipelineTimes::checkError)
        .def_readonly("max_frame_after_30", &SLAMPipeline::PipelineTimes::max_frame_after_30)
        .def_readonly("max_frame_id", &SLAMPipeline::PipelineTimes::max_frame_id)
        .def_readonly("gpu_memory_mb", &SLAMPipeline::PipelineTimes::gpu_memory_mb)
        .def("fps", &SLAMPipeline::PipelineTimes::fps)
        .def("fusion_fps", &SLAMPipeline::PipelineTimes::fusion_fps)
        .def("gaussian_fps", &SLAMPipeline::PipelineTimes::gaussian_fps);
    py::class_<SLAMPipeline>(m, "SLAMPipeline")
        .def(py::init<TsdfEngine*, SLAMGaussianModel*, uint64_t, bool>(), py::arg("engine"), py::arg("model"),
             py::arg("seed") = 1234, py::arg("use_gt_pose") = true, py::keep_alive<1, 2>(), py::keep_alive<1, 3>())
        .def(py::init<uint64_t>(), py::arg("seed") = 1234)
        .def("setTsdfEngine", &SLAMPipeline::setTsdfEngine)
        .def("setModel", [](SLAMPipeline& p, SLAMGaussianModel* m) { p.model = m; p.device = m->device; }, py::keep_alive<1, 2>())
        .def("SLAMTrainCamsModel", [](SLAMPipeline& p, SLAMGaussianModel& m, std::vector<Camera>& cams) {
            p.SLAMTrainCams(m, cams);
            return cams;  // with c2w_slam filled in
        }, py::call_guard<py::gil_scoped_release>())
        // the reference's whole-run clock (LOG_PIPELINE_TIME): SLAMTrainCams over `cams` from frame 0, -> the [PIPELINE AVG TIME] numbers
        .def("SLAMTrainCamsTimed", [](SLAMPipeline& p, SLAMGaussianModel& m, std::vector<Camera>& cams) {
            { py::gil_scoped_release nogil; p.SLAMTrainCams(m, cams); }
            return p.times;
        })
        .def_readonly("times", &SLAMPipeline::times)
        .def_readwrite("log_pipeline_time", &SLAMPipeline::log_pipeline_time)
        .def_readwrite("frame_report_ms", &SLAMPipeline::frame_report_ms)
        .def_readwrite("keep_frame_ms", &SLAMPipeline::keep_frame_ms)
        .def_readonly("frame_ms", &SLAMPipeline::frame_ms)
        .def_readonly("frame_wait_ms", &SLAMPipeline::frame_wait_ms)
        .def("processFrameCLI", [](SLAMPipeline& p, int i, Camera& cam) { p.processFrame(i, cam); },
             py::call_guard<py::gil_scoped_release>())
        .def("loadConfig", [](SLAMPipeline& p, const py::dict& d) { p.loadConfig(config_from_dict(d)); })
        .def("loadConfig", [](SLAMPipeline& p, const gpsh::Node& pipe_node, const std::string& workspace_dir, bool is_train) {
            p.loadConfig(pipe_node, workspace_dir, is_train);
        }, py::arg("pipe_node"), py::arg("workspace_dir"), py::arg("is_train"))
        .def("settings", [](SLAMPipeline& p) {
            FieldDumper dump;
            p.configFields(dump);
            dump.out["workspace_dir"] = p.workspace_dir; dump.out["model_path_full"] = p.model_path;
            dump.out["log_path_full"] = p.log_path; dump.out["eval_path_full"] = p.eval_path;
            return dump.out;
        })
        .def("save", &SLAMPipeline::save, py::arg("model"), py::arg("cams"), py::call_guard<py::gil_scoped_release>())
        .def("savePoses", &SLAMPipeline::savePoses, py::arg("dir"), py::arg("cams"))
        .def("save_poses", &SLAMPipeline::savePoses, py::arg("dir"), py::arg("cams"))
        .def_readwrite("eval_after_train", &SLAMPipeline::eval_after_train)
        .def_readwrite("save_after_train", &SLAMPipeline::save_after_train)
        .def_readonly("model_path", &SLAMPipeline::model_path)
        .def_readonly("log_path", &SLAMPipeline::log_path)
        .def_readonly("eval_path", &SLAMPipeline::eval_path)
        .def_readwrite("scene_scale", &SLAMPipeline::scene_scale)
        // the optimise loop may run the autograd engine (losses beyond L1): it must not hold the GIL
        .def("processFrame", py::overload_cast<int, Camera&, const torch::Tensor&, const torch::Tensor&>(&SLAMPipeline::processFrame),
             py::call_guard<py::gil_scoped_release>())
        .def("SLAMTrainCams", py::overload_cast<std::vector<Camera>&, const std::vector<torch::Tensor>&,
                                                const std::vector<torch::Tensor>&>(&SLAMPipeline::SLAMTrainCams),
             py::call_guard<py::gil_scoped_release>())
        .def("runRaycastByCam", &SLAMPipeline::runRaycastByCam, py::arg("cam"), py::arg("use_cam_depth") = true)
        .def_readwrite("overlap_mapping", &SLAMPipeline::overlap_mapping)
        .def_readwrite("mapping_thread", &SLAMPipeline::mapping_thread)
        .def_readwrite("async_raycasts", &SLAMPipeline::async_raycasts)
        .def_readwrite("frame_stream_kind", &SLAMPipeline::frame_stream_kind)
        .def_readwrite("map_stream_kind", &SLAMPipeline::map_stream_kind)
        .def_readwrite("raycast_stream_kind", &SLAMPipeline::raycast_stream_kind)
        .def_readwrite("prefetch_next_preprocess", &SLAMPipeline::prefetch_next_preprocess)
        .def_readwrite("fused_loss_terms", &SLAMPipeline::fused_loss_terms)
        .def_readonly("autograd_iters", &SLAMPipeline::autograd_iters)
        .def_readwrite("frame_chain_reserve", &SLAMPipeline::frame_chain_reserve)
        .def_readwrite("pipeline_raycasts", &SLAMPipeline::pipeline_raycasts)
        .def_readwrite("merge_keyframe_raycasts", &SLAMPipeline::merge_keyframe_raycasts)
        .def_readwrite("pump_iters_first", &SLAMPipeline::pump_iters_first)
        .def_readwrite("pump_iters_per_frame", &SLAMPipeline::pump_iters_per_frame)
        .def("flush", &SLAMPipeline::flush, py::call_guard<py::gil_scoped_release>())
        .def_readwrite("trace_frames", &SLAMPipeline::trace_frames)
        .def("frameTrace", [](SLAMPipeline& p) {
            { py::gil_scoped_release nogil; p.flush(); }
            return std::make_tuple(p.trace_live, p.trace_counters, p.trace_poses);
        })
        .def("removeRedundantGs", &SLAMPipeline::removeRedundantGs)
        .def("checkKeyFrameError", [](SLAMPipeline& p) { { py::gil_scoped_release nogil; p.flush(); } p.checkKeyFrameError(); })
        .def("keyframeLossDict", [](SLAMPipeline& p) { { py::gil_scoped_release nogil; p.flush(); } return p.keyframe_loss_dict; })
        .def("appendOptView", [](SLAMPipeline& p, const Camera& cam, TensorDict rc) {   // tests: a history view by hand
            p.opt_cam_list.push_back(cam); p.opt_raycast_list.push_back(std::move(rc));
        })
        .def_readwrite("sample_method", &SLAMPipeline::sample_method)
        .def_readwrite("loss_thres", &SLAMPipeline::loss_thres)
        .def_readwrite("large_scale_thres", &SLAMPipeline::large_scale_thres)
        .def_readwrite("small_scale_thres", &SLAMPipeline::small_scale_thres)
        .def_readwrite("low_opac_thres", &SLAMPipeline::low_opac_thres)
        .def("stats", [](SLAMPipeline& p) {
            { py::gil_scoped_release nogil; p.flush(); }
            py::dict d;
            d["frames"] = p.stats.frames.load(); d["opt_iters"] = p.stats.opt_iters.load(); d["raycasts"] = p.stats.raycasts.load();
            d["added"] = p.stats.added.load(); d["pruned"] = p.stats.pruned.load();
            return d;
        })
        .def("keyframeCount", [](SLAMPipeline& p) { { py::gil_scoped_release nogil; p.flush(); } return (int)p.keyframe_cam_list.size(); })
        .def("optCams", [](SLAMPipeline& p) { { py::gil_scoped_release nogil; p.flush(); } return p.opt_cam_list; })
        .def("optRaycasts", [](SLAMPipeline& p) { { py::gil_scoped_release nogil; p.flush(); } return p.opt_raycast_list; })
        .def_readwrite("workspace_dir", &SLAMPipeline::workspace_dir)
        .def_readwrite("saved_mesh", &SLAMPipeline::saved_mesh)
        .def_readwrite("saved_engine", &SLAMPipeline::saved_engine)
        .def("renderEvalImgs", &SLAMPipeline::renderEvalImgs, py::arg("cams"), py::arg("names") = std::vector<std::string>{"rgb"},
             py::call_guard<py::gil_scoped_release>())
        .def("evalGeometry", [](SLAMPipeline& p, const torch::Tensor& gt, const c10::optional<torch::Tensor>& T, const std::vector<double>& th,
                                int64_t sample_nums, uint64_t seed) {
            py::gil_scoped_release nogil;
            return p.evalGeometry(gt, T ? *T : torch::Tensor(), th, sample_nums, seed);
        }, py::arg("gt_points_or_triangles"), py::arg("transform") = py::none(), py::arg("dist_thres") = std::vector<double>{0.03},
             py::arg("sample_nums") = 1000000, py::arg("seed") = 0)
        .def("evalTrajectory", &SLAMPipeline::evalTrajectory, py::call_guard<py::gil_scoped_release>())
        .def("gesTrainCams", [](SLAMPipeline& p, const std::vector<Camera>& cams, int max_iterations, int64_t seed) {
            return p.gesTrainCams(cams, max_iterations, seed);
        }, py::arg("cams"), py::arg("max_iterations") = -1, py::arg("seed") = -1, py::call_guard<py::gil_scoped_release>())
        .def("gesTrainCamsWithLayers", [](SLAMPipeline& p, const std::vector<Camera>& cams, const std::vector<TensorDict>& layers, int max_iterations,
                                          int64_t seed) { return p.gesTrainCams(cams, layers, max_iterations, seed); },
             py::arg("cams"), py::arg("base_layers"), py::arg("max_iterations") = -1, py::arg("seed") = -1, py::call_guard<py::gil_scoped_release>())
        .def("rawTrainCams", [](SLAMPipeline& p, const std::vector<Camera>& cams, int max_iterations, int64_t seed, bool densify) {
            return p.rawTrainCams(cams, max_iterations, seed, densify);
        }, py::arg("cams"), py::arg("max_iterations") = -1, py::arg("seed") = -1, py::arg("densify") = false,
             py::call_guard<py::gil_scoped_release>())
        .def("trainCams", &SLAMPipeline::trainCams, py::arg("cams"), py::arg("mode"), py::call_guard<py::gil_scoped_release>())
        .def("refineKeyframeCams", [](SLAMPipeline& p) { { py::gil_scoped_release nogil; p.flush(); } return p.refineKeyframeCams(); })
        .def("refineCacheBytes", &SLAMPipeline::refineCacheBytes, py::arg("cams"))
        .def("refineLog", [](SLAMPipeline& p) {
            std::vector<std::pair<int, float>> out;
            for (const auto& e : p.refine_log) out.emplace_back(e.iter, e.loss);
            return out;
        })
        .def_readwrite("curr_iter", &SLAMPipeline::curr_iter)
        .def_readwrite("max_iterations", &SLAMPipeline::max_iterations)
        .def_readwrite("selected_cam_idx", &SLAMPipeline::selected_cam_idx)
        .def_readwrite("log_iter", &SLAMPipeline::log_iter)
        .def_readwrite("refine_iterations", &SLAMPipeline::refine_iterations)
        .def_readwrite("refine_cams", &SLAMPipeline::refine_cams)
        .def_readwrite("refine_seed", &SLAMPipeline::refine_seed)
        .def_readwrite("refine_cache_mb", &SLAMPipeline::refine_cache_mb)
        .def_readwrite("refine_lr_decay", &SLAMPipeline::refine_lr_decay)
        .def("evalImages", &SLAMPipeline::evalImages, py::arg("cams"), py::arg("depth_mask") = false, py::arg("source") = "rgb",
             py::call_guard<py::gil_scoped_release>())
        .def("saveMesh", &SLAMPipeline::saveMesh)
        .def("saveEngine", &SLAMPipeline::saveEngine)
        .def("loadEngine", &SLAMPipeline::loadEngine)
        .def_readwrite("work_mode", &SLAMPipeline::work_mode);

    // ---- the session (session.hpp): slam_trainer.cpp after the reader
    py::class_<SessionResult>(m, "SessionResult")
        .def_readonly("work_mode", &SessionResult::work_mode)
        .def_readonly("workspace_dir", &SessionResult::workspace_dir)
        .def_readonly("renders", &SessionResult::renders)
        .def_readonly("image_eval", &SessionResult::image_eval)
        .def_readonly("has_image_eval", &SessionResult::has_image_eval)
        .def_readonly("keyframe_count", &SessionResult::keyframe_count)
        .def_readonly("gaussian_num", &SessionResult::gaussian_num)
        .def_readonly("refine_iterations_done", &SessionResult::refine_iterations_done)
        .def_property_readonly("refine_log", [](const SessionResult& r) {
            std::vector<std::pair<int, float>> out;
            for (const auto& e : r.refine_log) out.emplace_back(e.iter, e.loss);
            return out;
        })
        .def_readonly("times", &SessionResult::times)
        .def_readonly("files", &SessionResult::files);
    m.def("run_session", &runSession, py::arg("root"), py::arg("reader"), py::arg("config_filename") = "",
          py::arg("poses_from_files") = false, py::arg("seed") = 1234, py::call_guard<py::gil_scoped_release>());
    m.def("create_work_space", &createWorkSpace, py::arg("config_filename"));
    m.def("cfg_args_line", &cfgArgsLine, py::arg("sh_degree"));
    m.def("write_cfg_args", &writeCfgArgs, py::arg("file_name"), py::arg("sh_degree"));
    m.def("cameras_json", &camerasJson, py::arg("cams"));
    m.def("write_cameras_json", &writeCamerasJson, py::arg("file_name"), py::arg("cams"));
    m.def("pose_txt", &poseTxt, py::arg("c2w"));
    m.def("write_pose_txt", &writePoseTxt, py::arg("file_name"), py::arg("c2w"));
    m.def("read_pose_txt", &readPoseTxt, py::arg("file_name"));
    m.def("frame_id_of", &frameIdOf, py::arg("cam"), py::arg("fallback_index") = 0);
}
