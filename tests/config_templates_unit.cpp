// Compile-only check (tests/test_config_node_cpu.py: g++ -fsyntax-only): the five node-typed entry points instantiate with a node
// type that offers what YAML::Node offers and NOTHING else -- a const operator[], as<T>() and IsDefined() -- so that with
// <yaml-cpp/yaml.h> on the include path their YAML::Node instantiations are the reference's own signatures.  And with gpsh::Node.
#include <map>
#include <sstream>

#include "session.hpp"

class FakeYamlNode {
public:
    FakeYamlNode() = default;
    const FakeYamlNode operator[](const std::string& key) const {
        auto it = children_.find(key);
        return it == children_.end() ? FakeYamlNode() : it->second;
    }
    bool IsDefined() const { return defined_; }
    template <class T> T as() const { return Read<T>::get(text_); }

private:
    template <class T> struct Read {
        static T get(const std::string& text) { std::stringstream s(text); T v{}; s >> v; return v; }
    };
    template <class T> struct Read<std::vector<T>> {
        static std::vector<T> get(const std::string& text) { std::stringstream s(text); std::vector<T> v; T x; while (s >> x) v.push_back(x); return v; }
    };
    std::map<std::string, FakeYamlNode> children_;
    std::string text_;
    bool defined_ = false;
};

template <class N>
static void instantiate(const N& config, DatasetReader& reader, SLAMGaussianModel& model, SLAMPipeline& pipe, TensorDict& render, const Camera& cam) {
    reader.loadConfig(config["READER"]);                                                        // DatasetReader(const YAML::Node&)
    InfiniTAM::Engine::CLIEngine* engine = createTsdfEngine(reader, config["PIPE"]["TSDF"]);    // InfiniTAM_tools.h
    pipe.setTsdfEngine(engine);
    model.loadConfig(config["MODEL"]);                                                          // raw_gs_model.h:24
    pipe.loadConfig(config["PIPE"], config["workspace_dir"].template as<std::string>(), true);  // slam_pipeline.h / pipeline.h
    TensorDict loss = model.computeLoss(render, cam, config["PIPE"]["weight_configs"]);         // raw_gs_model.h:52
    TensorDict masked = model.computeLoss(render, cam, config["PIPE"]["weight_configs"], torch::Tensor());
    (void)loss; (void)masked;
}

void instantiateBoth(DatasetReader& reader, SLAMGaussianModel& model, SLAMPipeline& pipe, TensorDict& render, const Camera& cam) {
    instantiate(FakeYamlNode(), reader, model, pipe, render, cam);
    instantiate(gpsh::parseYaml("a: 1\n"), reader, model, pipe, render, cam);
    // the existing flat route still resolves to the non-template overloads
    const gpsh::Config flat;
    model.loadConfig(flat);
    pipe.loadConfig(flat);
    (void)createTsdfEngine(reader, flat);
    (void)model.computeLoss(render, cam, flat);
    (void)runSession(gpsh::parseYaml("a: 1\n"), reader);
}
