// gpsh::Node: the part of YAML::Node the reference programs against (operator[], as<T>(), IsDefined() ...) over a reader for the
// block-YAML subset its config files are written in (configs/release/*/*.yaml, configs/viewer/office0.yaml), so that a session can
// be run from one of those files without yaml-cpp.  Standard library only: no torch, no HIP -- the header compiles stand-alone
// (tests/config_node_main.cpp puts it under the host sanitizers).
//
// The subset: nested block maps by space indentation; plain, 'single-quoted' and "double-quoted" scalars; empty values; flow
// sequences of scalars ([600, 600, 599.5, 339.5]); full-line and trailing " #" comments; trailing blanks; blank lines; CRLF; a
// missing final newline.  Everything else -- tabs in indentation, block sequences, anchors / aliases / tags, | and > scalars,
// several documents, flow maps, nested flow sequences, multi-line scalars, an unterminated quote or bracket, a duplicate key,
// indentation that returns to a level that was never opened -- throws gpsh::ConfigError with the 1-based line and the reason.
//
// Conversions follow yaml-cpp (yaml-cpp/node/convert.h), which the reference relies on: a scalar is untyped text; numbers go
// through stream extraction (basefield unset) and the whole token must be consumed (5e-2 -> 0.05f, 1 -> 1.0f, 1.5 -> int fails);
// bool takes y/n, yes/no, true/false, on/off in lower, Capitalised and UPPER form; std::string is the text of any scalar.
#pragma once
#include <cstddef>
#include <cstdint>
#include <fstream>
#include <limits>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace gpsh {

class ConfigError : public std::runtime_error {
public:
    ConfigError(const std::string& what, int line = 0) : std::runtime_error(what), line_(line) {}
    int line() const { return line_; }   // 1-based source line, 0 where there is none (a missing key)

private:
    int line_;
};

class Node {
public:
    enum Kind { kUndefined, kNull, kScalar, kSequence, kMap };
    typedef std::vector<std::pair<std::string, Node>> Items;
    typedef Items::const_iterator const_iterator;

    Node() : d_(std::make_shared<Data>()) {}

    bool IsDefined() const { return d_->kind != kUndefined; }
    bool IsNull() const { return d_->kind == kNull; }       // `key:` with nothing behind it, ~, null (yaml-cpp's Null)
    bool IsScalar() const { return d_->kind == kScalar; }
    bool IsSequence() const { return d_->kind == kSequence; }
    bool IsMap() const { return d_->kind == kMap; }
    Kind kind() const { return d_->kind; }
    size_t size() const { return d_->kind == kMap ? d_->items.size() : d_->kind == kSequence ? d_->seq.size() : 0; }

    // a missing key, an index out of range, a node that is no map / sequence: an undefined node that remembers the path
    Node operator[](const std::string& key) const {
        if (d_->kind == kMap)
            for (const auto& kv : d_->items)
                if (kv.first == key) return kv.second;
        return undefined(d_->path.empty() ? key : d_->path + "." + key);
    }
    Node operator[](const char* key) const { return (*this)[std::string(key ? key : "")]; }
    Node operator[](size_t i) const {
        if (d_->kind == kSequence && i < d_->seq.size()) return d_->seq[i];
        return undefined(d_->path + "[" + std::to_string(i) + "]");
    }
    Node operator[](int i) const { return i < 0 ? undefined(d_->path + "[" + std::to_string(i) + "]") : (*this)[(size_t)i]; }

    // map entries in file order (first: the key, second: the value)
    const_iterator begin() const { return d_->items.begin(); }
    const_iterator end() const { return d_->items.end(); }
    const std::vector<Node>& elements() const { return d_->seq; }

    const std::string& path() const { return d_->path; }      // "PIPE.TSDF.voxel_size", "READER.intrinsics[2]"; "" for the root
    int line() const { return d_->line; }                      // 1-based line the node starts on
    const std::string& source() const { return d_->source; }  // the name given to parseYaml / the file's path
    const std::string& text() const { return d_->text; }      // a scalar's text, quotes and escapes resolved
    bool quoted() const { return d_->quoted; }

    template <class T> T as() const { return Convert<T>::get(*this); }

private:
    struct Data {
        Kind kind = kUndefined;
        std::string text, path, source;
        bool quoted = false;
        int line = 0;
        Items items;
        std::vector<Node> seq;
    };
    std::shared_ptr<Data> d_;
    friend class YamlReader;

    static Node undefined(const std::string& path) {
        Node n;
        n.d_->path = path;
        return n;
    }
    std::string where() const {
        std::string w = d_->path.empty() ? std::string("<root>") : d_->path;
        if (d_->line > 0) w += " (" + (d_->source.empty() ? std::string("line ") : d_->source + ":") + std::to_string(d_->line) + ")";
        return w;
    }
    [[noreturn]] void failMissing() const {
        throw ConfigError(where() + ": key is missing" + (d_->source.empty() ? "" : " in " + d_->source), 0);
    }
    [[noreturn]] void failConvert(const char* type) const {
        const char* what = d_->kind == kMap ? "a map" : d_->kind == kSequence ? "a sequence" : d_->kind == kNull ? "null" : nullptr;
        throw ConfigError(where() + ": cannot convert " + (what ? std::string(what) : "'" + d_->text + "'") + " to " + type, d_->line);
    }

    static bool flexibleCase(const std::string& s, const char* lower) {   // yaml-cpp: IsFlexibleCase + tolower
        const std::string l(lower);
        if (s.size() != l.size() || s.empty()) return false;
        bool all_lower = true, all_upper = true, rest_lower = true;
        for (size_t i = 0; i < s.size(); i++) {
            const char c = s[i], lo = l[i], up = (char)(lo - 'a' + 'A');
            if (c != lo && c != up) return false;
            if (c != lo) { all_lower = false; if (i > 0) rest_lower = false; }
            if (c != up) all_upper = false;
        }
        return all_lower || all_upper || (s[0] != l[0] && rest_lower);
    }

    template <class T, class Enable = void> struct Convert;
};

// ---- conversions (yaml-cpp/node/convert.h)
template <class T>
struct Node::Convert<T, typename std::enable_if<std::is_arithmetic<T>::value && !std::is_same<T, bool>::value>::type> {
    static const char* name() {
        return std::is_floating_point<T>::value ? (sizeof(T) == 4 ? "float" : "double") : (sizeof(T) == 8 ? "int64" : "int");
    }
    static T get(const Node& n) {
        if (!n.IsDefined()) n.failMissing();
        if (!n.IsScalar()) n.failConvert(name());
        const std::string& s = n.text();
        std::stringstream stream(s);
        stream.unsetf(std::ios::dec);
        T v{};
        if ((stream >> std::noskipws >> v) && (stream >> std::ws).eof()) return v;
        if (std::is_floating_point<T>::value) {
            if (s == ".inf" || s == ".Inf" || s == ".INF" || s == "+.inf" || s == "+.Inf" || s == "+.INF")
                return std::numeric_limits<T>::infinity();
            if (s == "-.inf" || s == "-.Inf" || s == "-.INF") return (T)(-std::numeric_limits<T>::infinity());
            if (s == ".nan" || s == ".NaN" || s == ".NAN") return std::numeric_limits<T>::quiet_NaN();
        }
        n.failConvert(name());
    }
};

template <>
struct Node::Convert<bool, void> {
    static bool get(const Node& n) {
        if (!n.IsDefined()) n.failMissing();
        if (!n.IsScalar()) n.failConvert("bool");
        static const char* const names[4][2] = {{"y", "n"}, {"yes", "no"}, {"true", "false"}, {"on", "off"}};
        for (const auto& p : names) {
            if (flexibleCase(n.text(), p[0])) return true;
            if (flexibleCase(n.text(), p[1])) return false;
        }
        n.failConvert("bool");
    }
};

template <>
struct Node::Convert<std::string, void> {
    static std::string get(const Node& n) {
        if (!n.IsDefined()) n.failMissing();
        if (n.IsNull()) return "null";   // (yaml-cpp: as<std::string>() of a Null node)
        if (!n.IsScalar()) n.failConvert("string");
        return n.text();
    }
};

template <class T>
struct Node::Convert<std::vector<T>, void> {
    static std::vector<T> get(const Node& n) {
        if (!n.IsDefined()) n.failMissing();
        if (!n.IsSequence()) n.failConvert("a sequence");
        std::vector<T> out;
        out.reserve(n.size());
        for (const Node& e : n.elements()) out.push_back(e.as<T>());
        return out;
    }
};

// ---- the reader
class YamlReader {
public:
    YamlReader(const std::string& text, const std::string& name) : text_(text), name_(name) {}

    Node parse() {
        Node root = make(Node::kMap, "", 1);
        std::vector<Level> stack;
        stack.push_back(Level{-1, root, true});
        bool content_seen = false, pending_child = false;   // pending_child: the last key had nothing behind its colon
        Node pending;                                        // ... and this is its (so far Null) value
        size_t pos = 0;
        int line_no = 0;
        while (pos <= text_.size()) {
            if (pos == text_.size()) break;
            size_t eol = text_.find('\n', pos);
            if (eol == std::string::npos) eol = text_.size();
            std::string line = text_.substr(pos, eol - pos);
            pos = eol + 1;
            line_no++;
            if (!line.empty() && line.back() == '\r') line.pop_back();
            // indentation
            size_t ind = 0;
            while (ind < line.size() && line[ind] == ' ') ind++;
            size_t first = ind;
            while (first < line.size() && (line[first] == ' ' || line[first] == '\t')) first++;
            if (first == line.size() || line[first] == '#') continue;   // blank / comment line
            if (first != ind) fail(line_no, "tab in indentation");
            const std::string body = line.substr(ind);
            if (ind == 0 && startsWith(body, "---") && (body.size() == 3 || body[3] == ' ' || body[3] == '\t')) {
                if (content_seen || rstrip(stripComment(body.substr(3))).size() > 0)
                    fail(line_no, content_seen ? "multiple documents are not supported" : "content on the document marker line is not supported");
                content_seen = true;
                continue;
            }
            if (ind == 0 && startsWith(body, "...") && (body.size() == 3 || body[3] == ' ' || body[3] == '\t'))
                fail(line_no, "document end marker is not supported");
            if (ind == 0 && body[0] == '%') fail(line_no, "directives are not supported");
            content_seen = true;
            if (body[0] == '-' && (body.size() == 1 || body[1] == ' ' || body[1] == '\t')) fail(line_no, "block sequences are not supported");
            rejectIndicator(body[0], line_no, "key");
            if (body[0] == '?' && (body.size() == 1 || body[1] == ' ')) fail(line_no, "complex keys are not supported");
            if (body[0] == '[' || body[0] == ']' || body[0] == ',' ) fail(line_no, "expected 'key: value'");

            // which map does the line belong to
            const int n = (int)ind;
            if (n > stack.back().indent) {
                if (stack.back().fresh) {
                    stack.back().indent = n;   // first entry of a map fixes its indentation
                    stack.back().fresh = false;
                } else if (pending_child) {
                    become(pending, Node::kMap);
                    stack.push_back(Level{n, pending, false});
                } else {
                    fail(line_no, "unexpected indentation (the line above opens no map)");
                }
            } else {
                while (stack.size() > 1 && stack.back().indent > n) stack.pop_back();
                if (stack.back().indent != n) {
                    if (stack.back().fresh) { stack.back().indent = n; stack.back().fresh = false; }
                    else fail(line_no, "indentation returns to a level that was never opened");
                }
            }
            pending_child = false;
            Node map = stack.back().map;

            // key
            size_t i = 0;
            std::string key;
            if (body[0] == '"' || body[0] == '\'') {
                key = quotedScalar(body, i, line_no);
                while (i < body.size() && (body[i] == ' ' || body[i] == '\t')) i++;
                if (i >= body.size() || body[i] != ':') fail(line_no, "expected ':' after the quoted key");
            } else {
                size_t c = 0;
                for (;; c++) {
                    if (c >= body.size()) fail(line_no, "expected 'key: value' (multi-line scalars are not supported)");
                    if (body[c] == '#' && c > 0 && (body[c - 1] == ' ' || body[c - 1] == '\t'))
                        fail(line_no, "expected 'key: value' (multi-line scalars are not supported)");
                    if (body[c] == ':' && (c + 1 == body.size() || body[c + 1] == ' ' || body[c + 1] == '\t')) break;
                }
                key = rstrip(body.substr(0, c));
                i = c;
            }
            if (i + 1 < body.size() && body[i + 1] != ' ' && body[i + 1] != '\t') fail(line_no, "expected a blank after ':'");
            i++;   // past ':'
            for (const auto& kv : map.d_->items)
                if (kv.first == key) fail(line_no, "duplicate key '" + key + "' (first at line " + std::to_string(kv.second.line()) + ")");
            const std::string path = map.path().empty() ? key : map.path() + "." + key;

            // value
            while (i < body.size() && (body[i] == ' ' || body[i] == '\t')) i++;
            Node value;
            if (i >= body.size() || body[i] == '#') {
                value = make(Node::kNull, path, line_no);
                pending_child = true;
                pending = value;
            } else if (body[i] == '[') {
                value = flowSequence(body, i, path, line_no);
                trailing(body, i, line_no);
            } else if (body[i] == '"' || body[i] == '\'') {
                value = make(Node::kScalar, path, line_no);
                value.d_->text = quotedScalar(body, i, line_no);
                value.d_->quoted = true;
                trailing(body, i, line_no);
            } else {
                rejectIndicator(body[i], line_no, "value");
                if (body[i] == '{' || body[i] == '}') fail(line_no, "flow maps are not supported");
                if (body[i] == '|' || body[i] == '>') fail(line_no, "block scalars (| and >) are not supported");
                if (body[i] == ']' || body[i] == ',' || body[i] == '%' || body[i] == '@' || body[i] == '`')
                    fail(line_no, std::string("a plain scalar cannot start with '") + body[i] + "'");
                if ((body[i] == '-' || body[i] == '?') && (i + 1 == body.size() || body[i + 1] == ' '))
                    fail(line_no, "block sequences are not supported");
                const std::string plain = rstrip(stripComment(body.substr(i)));
                for (size_t c = 0; c < plain.size(); c++)
                    if (plain[c] == ':' && (c + 1 == plain.size() || plain[c + 1] == ' ' || plain[c + 1] == '\t'))
                        fail(line_no, "mapping values are not allowed inside a plain scalar");
                value = plainScalar(plain, path, line_no);
            }
            map.d_->items.push_back(std::make_pair(key, value));
        }
        return root;
    }

private:
    struct Level { int indent; Node map; bool fresh; };
    const std::string& text_;
    const std::string name_;

    [[noreturn]] void fail(int line, const std::string& why) const {
        throw ConfigError((name_.empty() ? std::string("line ") : name_ + ":") + std::to_string(line) + ": " + why, line);
    }
    Node make(Node::Kind kind, const std::string& path, int line) const {
        Node n;
        n.d_->kind = kind; n.d_->path = path; n.d_->line = line; n.d_->source = name_;
        return n;
    }
    static void become(Node& n, Node::Kind kind) { n.d_->kind = kind; }
    static bool startsWith(const std::string& s, const char* p) { return s.compare(0, std::char_traits<char>::length(p), p) == 0; }
    static std::string rstrip(std::string s) {
        while (!s.empty() && (s.back() == ' ' || s.back() == '\t')) s.pop_back();
        return s;
    }
    // cut a plain scalar at a " #" comment
    static std::string stripComment(const std::string& s) {
        for (size_t c = 0; c < s.size(); c++)
            if (s[c] == '#' && (c == 0 || s[c - 1] == ' ' || s[c - 1] == '\t')) return s.substr(0, c);
        return s;
    }
    void rejectIndicator(char c, int line, const char* what) const {
        if (c == '&') fail(line, std::string("anchors are not supported (") + what + ")");
        if (c == '*') fail(line, std::string("aliases are not supported (") + what + ")");
        if (c == '!') fail(line, std::string("tags are not supported (") + what + ")");
    }
    // after a quoted scalar or a flow sequence: blanks and a comment only
    void trailing(const std::string& s, size_t i, int line) const {
        const size_t end_of_value = i;
        while (i < s.size() && (s[i] == ' ' || s[i] == '\t')) i++;
        if (i >= s.size()) return;
        if (s[i] == '#' && i > end_of_value) return;
        fail(line, "unexpected text behind the value");
    }
    Node plainScalar(const std::string& plain, const std::string& path, int line) const {
        const bool null = plain.empty() || plain == "~" || plain == "null" || plain == "Null" || plain == "NULL";
        Node v = make(null ? Node::kNull : Node::kScalar, path, line);
        v.d_->text = plain;
        return v;
    }
    // s[i] is the opening quote; returns the content and leaves i behind the closing quote
    std::string quotedScalar(const std::string& s, size_t& i, int line) const {
        const char q = s[i++];
        std::string out;
        for (;;) {
            if (i >= s.size()) fail(line, "unterminated quote (multi-line scalars are not supported)");
            const char c = s[i++];
            if (q == '\'') {
                if (c != '\'') { out += c; continue; }
                if (i < s.size() && s[i] == '\'') { out += '\''; i++; continue; }
                return out;
            }
            if (c == '"') return out;
            if (c != '\\') { out += c; continue; }
            if (i >= s.size()) fail(line, "unterminated quote (multi-line scalars are not supported)");
            const char e = s[i++];
            switch (e) {
                case 'n': out += '\n'; break;
                case 't': case '\t': out += '\t'; break;
                case 'r': out += '\r'; break;
                case '0': out += '\0'; break;
                case 'a': out += '\a'; break;
                case 'b': out += '\b'; break;
                case 'e': out += '\x1b'; break;
                case 'f': out += '\f'; break;
                case 'v': out += '\v'; break;
                case ' ': case '"': case '/': case '\\': out += e; break;
                default: fail(line, std::string("escape \\") + e + " is not supported");
            }
        }
    }
    // s[i] == '['; leaves i behind the closing bracket
    Node flowSequence(const std::string& s, size_t& i, const std::string& path, int line) const {
        Node seq = make(Node::kSequence, path, line);
        i++;
        bool want_item = true;
        for (;;) {
            while (i < s.size() && (s[i] == ' ' || s[i] == '\t')) i++;
            if (i >= s.size()) fail(line, "unterminated bracket (a flow sequence ends on the line it starts on)");
            const char c = s[i];
            const std::string ipath = path + "[" + std::to_string(seq.d_->seq.size()) + "]";
            if (c == ']') {   // (also behind a trailing comma: legal YAML)
                i++;
                return seq;
            }
            if (c == '#' && (s[i - 1] == ' ' || s[i - 1] == '\t')) fail(line, "unterminated bracket (a flow sequence ends on the line it starts on)");
            if (c == ',') {
                if (want_item) fail(line, "empty entry in the flow sequence");
                want_item = true;
                i++;
                continue;
            }
            if (!want_item) fail(line, "expected ',' or ']' in the flow sequence");
            if (c == '[') fail(line, "nested flow sequences are not supported");
            if (c == '{' || c == '}') fail(line, "flow maps are not supported");
            rejectIndicator(c, line, "flow entry");
            Node item;
            if (c == '"' || c == '\'') {
                item = make(Node::kScalar, ipath, line);
                item.d_->text = quotedScalar(s, i, line);
                item.d_->quoted = true;
            } else {
                size_t e = i;
                while (e < s.size() && s[e] != ',' && s[e] != ']') {
                    if (s[e] == '[' || s[e] == '{' || s[e] == '}') fail(line, "flow collections inside an entry are not supported");
                    if (s[e] == '#' && (s[e - 1] == ' ' || s[e - 1] == '\t')) fail(line, "unterminated bracket (a flow sequence ends on the line it starts on)");
                    if (s[e] == ':' && (e + 1 == s.size() || s[e + 1] == ' ' || s[e + 1] == ',' || s[e + 1] == ']'))
                        fail(line, "flow maps are not supported");
                    e++;
                }
                if (e >= s.size()) fail(line, "unterminated bracket (a flow sequence ends on the line it starts on)");
                item = plainScalar(rstrip(s.substr(i, e - i)), ipath, line);
                i = e;
            }
            seq.d_->seq.push_back(item);
            want_item = false;
        }
    }
};

inline Node parseYaml(const std::string& text, const std::string& name = "") { return YamlReader(text, name).parse(); }

inline Node loadYamlFile(const std::string& path) {
    std::ifstream f(path.c_str(), std::ios::binary);
    if (!f) throw ConfigError(path + ": cannot open the file");
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    return parseYaml(text, path);
}

}  // namespace gpsh
