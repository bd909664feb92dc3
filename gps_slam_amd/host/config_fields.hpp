// One list of keys per entry point.  Every loadConfig / createTsdfEngine of the host layer names its keys ONCE, in a function
// template `fields(visitor)`; the visitors below run that list for
//   * the flat gpsh::Config route (ConfigReader: field = config.get(key, field), the behaviour the route always had),
//   * a node in the reference's nested layout (NodeFlattener<N>: YAML::Node or anything with its surface -- n[key],
//     n.as<T>(), n.IsDefined() -- into a flat Config, which then goes through the same ConfigReader),
//   * the unknown-key check (KeyLister + checkUnknownKeys), which needs to enumerate a map's keys and therefore runs for
//     gpsh::Node ONLY: a generic N offers no iteration within the surface above, so a YAML::Node section with a typo in an
//     optional key is not caught.
// Key classes: kRequired = the reference reads it with .as<T>() (missing -> gpsh::ConfigError with the key's path, before
// anything is allocated); kOptional = a key this project added (read under IsDefined()); kFlatOnly = accepted on the flat route
// alone (what the nested files keep elsewhere, e.g. READER.scene_scale); kNodeOnly = an optional key of this project that only a
// node carries: the flat route never read it and still does not (a Config that happens to hold the name changes nothing).
#pragma once
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "config_node.hpp"
#include "gps_host_common.hpp"

namespace gpsh {

enum FieldUse { kRequired, kOptional, kFlatOnly, kNodeOnly };

struct ConfigReader {
    const Config& c;
    bool from_node = false;   // the Config is a flattened node: its kNodeOnly keys count
    ConfigReader section(const char*) const { return *this; }   // (the flat route has one namespace)
    bool skip(FieldUse use) const { return use == kNodeOnly && !from_node; }
    void i(const char* k, int& v, FieldUse use = kRequired) { if (!skip(use)) v = (int)c.get(k, v); }
    void i64(const char* k, int64_t& v, FieldUse use = kRequired) { if (!skip(use)) v = (int64_t)c.get(k, (double)v); }
    void f(const char* k, float& v, FieldUse use = kRequired) { if (!skip(use)) v = (float)c.get(k, v); }
    void d(const char* k, double& v, FieldUse use = kRequired) { if (!skip(use)) v = c.get(k, v); }
    void b(const char* k, bool& v, FieldUse use = kRequired) { if (!skip(use)) v = c.get(k, v ? 1.0 : 0.0) != 0.0; }
    void s(const char* k, std::string& v, FieldUse use = kRequired) { if (!skip(use)) v = c.gets(k, v); }
    void ignored(const char*) {}
};

// the path a node reports in messages: its own for gpsh::Node, the section's usual name otherwise
template <class N> inline std::string nodePath(const N&, const char* usual) { return usual; }
inline std::string nodePath(const Node& n, const char* usual) { return n.path().empty() ? std::string(usual) : n.path(); }

template <class N>
struct NodeFlattener {
    N n;
    std::string path;
    Config* out;
    NodeFlattener section(const char* k) const { return NodeFlattener{n[std::string(k)], path + "." + k, out}; }
    template <class T>
    bool read(const char* k, FieldUse use, T& v) const {
        if (use == kFlatOnly) return false;
        const N child = n[std::string(k)];
        if (!child.IsDefined()) {
            if (use == kRequired) throw ConfigError(path + "." + k + ": required key is missing");
            return false;
        }
        v = child.template as<T>();
        return true;
    }
    void i(const char* k, int&, FieldUse use = kRequired) { int v; if (read(k, use, v)) out->num[k] = v; }
    void i64(const char* k, int64_t&, FieldUse use = kRequired) { int64_t v; if (read(k, use, v)) out->num[k] = (double)v; }
    void f(const char* k, float&, FieldUse use = kRequired) { float v; if (read(k, use, v)) out->num[k] = v; }
    void d(const char* k, double&, FieldUse use = kRequired) { double v; if (read(k, use, v)) out->num[k] = v; }
    void b(const char* k, bool&, FieldUse use = kRequired) { bool v; if (read(k, use, v)) out->num[k] = v ? 1.0 : 0.0; }
    void s(const char* k, std::string&, FieldUse use = kRequired) { std::string v; if (read(k, use, v)) out->str[k] = v; }
    void ignored(const char*) {}
};

// node -> the fields themselves, for an entry point without a flat route (DatasetReader::loadConfig); also sequences
template <class N>
struct NodeAssigner {
    N n;
    std::string path;
    template <class T>
    void read(const char* k, FieldUse use, T& v) const {
        if (use == kFlatOnly) return;
        const N child = n[std::string(k)];
        if (!child.IsDefined()) {
            if (use == kRequired) throw ConfigError(path + "." + k + ": required key is missing");
            return;
        }
        v = child.template as<T>();
    }
    void i(const char* k, int& v, FieldUse use = kRequired) { read(k, use, v); }
    void f(const char* k, float& v, FieldUse use = kRequired) { read(k, use, v); }
    void s(const char* k, std::string& v, FieldUse use = kRequired) { read(k, use, v); }
    void fv(const char* k, std::vector<float>& v, FieldUse use = kRequired) { read(k, use, v); }
    void iv(const char* k, std::vector<int>& v, FieldUse use = kRequired) { read(k, use, v); }
    void ignored(const char*) {}
};

struct KeyTree {
    std::vector<std::string> keys;
    std::map<std::string, std::unique_ptr<KeyTree>> sections;
};

struct KeyLister {
    KeyTree* t;
    KeyLister section(const char* k) const {
        t->keys.push_back(k);
        auto& s = t->sections[k];
        if (!s) s.reset(new KeyTree());
        return KeyLister{s.get()};
    }
    void add(const char* k, FieldUse use) { if (use != kFlatOnly) t->keys.push_back(k); }
    void i(const char* k, int&, FieldUse use = kRequired) { add(k, use); }
    void i64(const char* k, int64_t&, FieldUse use = kRequired) { add(k, use); }
    void f(const char* k, float&, FieldUse use = kRequired) { add(k, use); }
    void d(const char* k, double&, FieldUse use = kRequired) { add(k, use); }
    void b(const char* k, bool&, FieldUse use = kRequired) { add(k, use); }
    void s(const char* k, std::string&, FieldUse use = kRequired) { add(k, use); }
    void fv(const char* k, std::vector<float>&, FieldUse use = kRequired) { add(k, use); }
    void iv(const char* k, std::vector<int>&, FieldUse use = kRequired) { add(k, use); }
    void ignored(const char* k) { t->keys.push_back(k); }
};

inline void checkUnknownKeys(const Node& n, const KeyTree& known) {
    if (!n.IsMap()) return;
    for (const auto& kv : n) {
        bool found = false;
        for (const auto& k : known.keys) found = found || k == kv.first;
        if (!found)
            throw ConfigError(kv.second.path() + ": unknown key (" + (n.source().empty() ? std::string("line ") : n.source() + ":") +
                              std::to_string(kv.second.line()) + ")", kv.second.line());
        auto s = known.sections.find(kv.first);
        if (s != known.sections.end()) checkUnknownKeys(kv.second, *s->second);
    }
}

// for gpsh::Node: every key of the section is in `fields` (a callable taking the visitor by reference); nothing for another N
template <class N, class Fields>
inline void rejectUnknownKeys(const N& n, Fields&& fields) {
    if constexpr (std::is_same<N, Node>::value) {
        KeyTree known;
        KeyLister lister{&known};
        fields(lister);
        checkUnknownKeys(n, known);
    }
}

// node -> flat Config through `fields`; for gpsh::Node the unknown-key check first
template <class N, class Fields>
inline Config flattenNode(const N& n, const char* usual_path, Fields&& fields) {
    rejectUnknownKeys(n, fields);
    Config out;
    NodeFlattener<N> flat{n, nodePath(n, usual_path), &out};
    fields(flat);
    return out;
}

}  // namespace gpsh
