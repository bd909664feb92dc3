// Stand-alone driver of gps_slam_amd/host/config_node.hpp for the host sanitizers (tests/test_config_node_cpu.py builds it with
// -fsanitize=address,undefined and runs it as a plain process): every fixture and every malformed file, every prefix of every
// fixture, and single-byte substitutions drawn with a fixed seed from the characters the grammar gives a meaning to.  Whatever
// parses is walked, and every as<T>() is called on every node.  Exit status 0 = nothing crashed, nothing looped, every
// rejection was a gpsh::ConfigError.
//
//   config_node_main <fixture dir> <malformed dir> [substitutions per file]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <random>

#include "config_node.hpp"

namespace fs = std::filesystem;
using gpsh::ConfigError;
using gpsh::Node;

static long g_nodes = 0, g_converted = 0, g_parsed = 0, g_rejected = 0;

template <class T>
static void tryAs(const Node& n) {
    try {
        (void)n.as<T>();
        g_converted++;
    } catch (const ConfigError&) {
    }
}

static void walk(const Node& n, int depth = 0) {
    g_nodes++;
    tryAs<int>(n); tryAs<int64_t>(n); tryAs<float>(n); tryAs<double>(n); tryAs<bool>(n); tryAs<std::string>(n);
    tryAs<std::vector<float>>(n); tryAs<std::vector<int>>(n);
    (void)n.IsDefined(); (void)n.IsMap(); (void)n.IsSequence(); (void)n.IsScalar(); (void)n.size(); (void)n.path(); (void)n.line();
    if (depth > 64) return;
    if (n.IsMap())
        for (const auto& kv : n) {
            if (!n[kv.first].IsDefined()) { std::fprintf(stderr, "key '%s' listed but not found\n", kv.first.c_str()); std::exit(2); }
            walk(kv.second, depth + 1);
        }
    if (n.IsSequence())
        for (size_t i = 0; i < n.size(); i++) walk(n[i], depth + 1);
    // what is not there is undefined, and stays undefined when indexed again
    const Node u = n["no such key"][3]["nor this"];
    if (u.IsDefined() || n[n.size()].IsDefined()) { std::fprintf(stderr, "a missing entry is defined\n"); std::exit(2); }
    tryAs<int>(u); tryAs<std::string>(u);
}

static bool parse(const std::string& text, const std::string& name) {
    try {
        walk(gpsh::parseYaml(text, name));
        g_parsed++;
        return true;
    } catch (const ConfigError& e) {
        if (e.line() < 1) { std::fprintf(stderr, "%s: rejection without a line: %s\n", name.c_str(), e.what()); std::exit(2); }
        g_rejected++;
        return false;
    }
}

static std::vector<fs::path> filesUnder(const char* dir) {
    std::vector<fs::path> out;
    for (const auto& e : fs::recursive_directory_iterator(dir))
        if (e.is_regular_file() && e.path().extension() == ".yaml") out.push_back(e.path());
    std::sort(out.begin(), out.end());
    return out;
}

static std::string slurp(const fs::path& p) {
    std::ifstream f(p, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s <fixture dir> <malformed dir> [substitutions [shard shards]]\n", argv[0]); return 2; }
    const int substitutions = argc > 3 ? std::atoi(argv[3]) : 2000;
    // the inputs are numbered; a process given `shard shards` takes every shards-th one (the test runs the shards side by side:
    // most of the time goes into the exceptions of the conversions that fail, five per scalar)
    const long shard = argc > 5 ? std::atol(argv[4]) : 0, shards = argc > 5 ? std::max(1L, std::atol(argv[5])) : 1;
    long item = 0;
    const auto good = filesUnder(argv[1]), bad = filesUnder(argv[2]);
    if (good.empty() || bad.empty()) { std::fprintf(stderr, "no fixtures found\n"); return 2; }
    for (const auto& p : good) {
        (void)gpsh::loadYamlFile(p.string());   // through the file entry once
        if (!parse(slurp(p), p.string())) { std::fprintf(stderr, "%s does not parse\n", p.c_str()); return 2; }
    }
    for (const auto& p : bad)
        if (parse(slurp(p), p.string())) { std::fprintf(stderr, "%s parses\n", p.c_str()); return 2; }
    static const char alphabet[] = {'"', '\'', '[', ']', ',', ':', '#', '\t', '\n', '-', '&', '*', '|', ' '};
    std::mt19937 rng(20240607u);
    for (const auto& p : good) {
        const std::string text = slurp(p);
        for (size_t cut = 0; cut <= text.size(); cut++)
            if (item++ % shards == shard) (void)parse(text.substr(0, cut), "prefix");
        for (int k = 0; k < substitutions; k++) {
            const size_t at = rng() % text.size();
            const char c = alphabet[rng() % sizeof alphabet];
            if (item++ % shards != shard) continue;
            std::string t = text;
            t[at] = c;
            (void)parse(t, "substitution");
        }
    }
    std::printf("config_node_main ok: %zu fixtures, %zu malformed, %ld inputs parsed, %ld rejected, %ld nodes walked, %ld conversions\n",
                good.size(), bad.size(), g_parsed, g_rejected, g_nodes, g_converted);
    return 0;
}
