"""The reference's configuration files (configs/release/*/*.yaml) for the Python mirror.

load_yaml(path) / parse_yaml(text) give the file as nested dicts in file order whose leaves are UNTYPED text, converted on access
by yaml-cpp's rules -- the ones the reference's `.as<T>()` calls rely on: `Scalar.as_float()` of "5e-2" is 0.05 (PyYAML, a YAML
1.1 reader, calls that a string), "1.5".as_int() raises, bool takes y/n, yes/no, true/false, on/off in lower, Capitalised and UPPER
form.  Where the C++ host layer is built this is a thin wrapper over gps_slam_amd._host (host/config_node.hpp); otherwise the same
grammar in Python (_parse_python) -- block maps by space indentation, plain / quoted scalars, empty values, flow sequences of
scalars, comments -- with the same rejections, each a ConfigError (a ValueError) that names the 1-based line.  No PyYAML: the
library does not depend on it.

flatten(section) turns a section into the flat, typed dict the mirror's constructors take (gs_model.RawGaussianModel(cfg),
slam_pipeline.SLAMPipeline(pipe_cfg=...)); SLAMPipeline.from_config(nested, ...) uses it.
"""
import re


class ConfigError(ValueError):
    def __init__(self, message, line=0):
        super().__init__(message)
        self.line = line


_BOOLS = {"y": True, "n": False, "yes": True, "no": False, "true": True, "false": False, "on": True, "off": False}
# what stream extraction with basefield unset accepts for an integer / a floating-point number, whole token
_INT = re.compile(r"[+-]?(0[xX][0-9a-fA-F]+|0[0-7]*|[1-9][0-9]*)\Z")
_FLOAT = re.compile(r"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?\Z")
_SPECIAL = {".inf": float("inf"), ".Inf": float("inf"), ".INF": float("inf"), "+.inf": float("inf"), "+.Inf": float("inf"),
            "+.INF": float("inf"), "-.inf": float("-inf"), "-.Inf": float("-inf"), "-.INF": float("-inf"), ".nan": float("nan"),
            ".NaN": float("nan"), ".NAN": float("nan")}


class Scalar(str):
    """A scalar's text (quotes and escapes resolved) with the key path and line it came from."""

    def __new__(cls, text, path="", line=0):
        s = super().__new__(cls, text)
        s.path, s.line = path, line
        return s

    def _fail(self, what):
        raise ConfigError("%s (line %d): cannot convert '%s' to %s" % (self.path or "<root>", self.line, str(self), what), self.line)

    def as_str(self):
        return str(self)

    def as_int(self):
        m = _INT.match(self)
        if not m:
            self._fail("int")
        body = self.lstrip("+-")
        v = int(body, 16) if body[:2] in ("0x", "0X") else int(body, 8) if len(body) > 1 and body[0] == "0" else int(body)
        return -v if self.startswith("-") else v

    def as_float(self):
        if _FLOAT.match(self):
            return float(self)
        if str(self) in _SPECIAL:
            return _SPECIAL[str(self)]
        self._fail("float")

    def as_bool(self):
        t = str(self)
        if t.lower() in _BOOLS and (t == t.lower() or t == t.upper() or t == t.capitalize()):
            return _BOOLS[t.lower()]
        self._fail("bool")


def _wrap(node):
    """a _host.Node -> the same tree as dicts / lists with Scalar leaves that keep the node's path and line"""
    if node.IsMap():
        return {k: _wrap(node[k]) for k in node.keys()}
    if node.IsSequence():
        return [_wrap(node[i]) for i in range(len(node))]
    return None if node.IsNull() else Scalar(node.as_str(), node.path, node.line)


def _host():
    """gps_slam_amd._host where it is built, else None (-> the Python reader below).  Only "not built" falls back: a host module
    that exists and fails to load is an error."""
    import importlib.util
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    if importlib.util.find_spec("gps_slam_amd._host") is None or not os.path.exists(os.path.join(here, "libgpsslam_hip.so")):
        return None
    from . import _lib
    _lib.load_library()
    from . import _host as h
    return h


def parse_yaml(text, name=""):
    h = _host()
    if h is None:
        return _parse_python(text, name)
    try:
        return _wrap(h.parse_yaml(text, name))
    except ValueError as e:
        m = re.match(r"(?:.*?:|line )(\d+): ", str(e))
        raise ConfigError(str(e), int(m.group(1)) if m else 0) from None


def load_yaml(path):
    with open(path, "rb") as f:
        return parse_yaml(f.read().decode("utf-8"), str(path))


# ------------------------------------------------------------------ the same grammar in Python (host/config_node.hpp, YamlReader)
_ESCAPES = {"n": "\n", "t": "\t", "\t": "\t", "r": "\r", "0": "\0", "a": "\a", "b": "\b", "e": "\x1b", "f": "\f", "v": "\v",
            " ": " ", '"': '"', "/": "/", "\\": "\\"}
_NULLS = ("", "~", "null", "Null", "NULL")


def _parse_python(text, name=""):
    def fail(line, why):
        raise ConfigError("%s%d: %s" % (name + ":" if name else "line ", line, why), line)

    def strip_comment(s):
        for c, ch in enumerate(s):
            if ch == "#" and (c == 0 or s[c - 1] in " \t"):
                return s[:c]
        return s

    def reject_indicator(ch, line, what):
        for c, word in (("&", "anchors"), ("*", "aliases"), ("!", "tags")):
            if ch == c:
                fail(line, "%s are not supported (%s)" % (word, what))

    def quoted(s, i, line):
        q = s[i]
        i += 1
        out = []
        while True:
            if i >= len(s):
                fail(line, "unterminated quote (multi-line scalars are not supported)")
            c = s[i]
            i += 1
            if q == "'":
                if c != "'":
                    out.append(c)
                elif i < len(s) and s[i] == "'":
                    out.append("'")
                    i += 1
                else:
                    return "".join(out), i
                continue
            if c == '"':
                return "".join(out), i
            if c != "\\":
                out.append(c)
                continue
            if i >= len(s):
                fail(line, "unterminated quote (multi-line scalars are not supported)")
            e = s[i]
            i += 1
            if e not in _ESCAPES:
                fail(line, "escape \\%s is not supported" % e)
            out.append(_ESCAPES[e])

    def trailing(s, i, line):
        rest = s[i:]
        t = rest.lstrip(" \t")
        if t and not (t[0] == "#" and len(t) < len(rest)):
            fail(line, "unexpected text behind the value")

    def plain(t, path, line):
        return None if t in _NULLS else Scalar(t, path, line)

    def flow(s, i, path, line):
        unterminated = "unterminated bracket (a flow sequence ends on the line it starts on)"
        seq, want = [], True
        i += 1
        while True:
            while i < len(s) and s[i] in " \t":
                i += 1
            if i >= len(s):
                fail(line, unterminated)
            c = s[i]
            ipath = "%s[%d]" % (path, len(seq))
            if c == "]":
                return seq, i + 1
            if c == "#" and s[i - 1] in " \t":
                fail(line, unterminated)
            if c == ",":
                if want:
                    fail(line, "empty entry in the flow sequence")
                want = True
                i += 1
                continue
            if not want:
                fail(line, "expected ',' or ']' in the flow sequence")
            if c == "[":
                fail(line, "nested flow sequences are not supported")
            if c in "{}":
                fail(line, "flow maps are not supported")
            reject_indicator(c, line, "flow entry")
            if c in "\"'":
                t, i = quoted(s, i, line)
                seq.append(Scalar(t, ipath, line))
            else:
                e = i
                while e < len(s) and s[e] not in ",]":
                    if s[e] in "[{}":
                        fail(line, "flow collections inside an entry are not supported")
                    if s[e] == "#" and s[e - 1] in " \t":
                        fail(line, unterminated)
                    if s[e] == ":" and (e + 1 == len(s) or s[e + 1] in " ,]"):
                        fail(line, "flow maps are not supported")
                    e += 1
                if e >= len(s):
                    fail(line, unterminated)
                seq.append(plain(s[i:e].rstrip(" \t"), ipath, line))
                i = e
            want = False

    root = {}
    stack = [[-1, root, "", True]]   # indent, map, path, fresh
    first_line = {id(root): {}}
    content_seen = False
    pending = None                   # (map, key, path) of a key with nothing behind its colon
    marker = lambda b, m: b.startswith(m) and (len(b) == 3 or b[3] in " \t")
    for line_no, line in enumerate(text.split("\n"), 1):
        if line_no == text.count("\n") + 1 and line == "":
            break
        if line.endswith("\r"):
            line = line[:-1]
        ind = len(line) - len(line.lstrip(" "))
        first = len(line) - len(line.lstrip(" \t"))
        if first == len(line) or line[first] == "#":
            continue
        if first != ind:
            fail(line_no, "tab in indentation")
        body = line[ind:]
        if ind == 0 and marker(body, "---"):
            if content_seen or strip_comment(body[3:]).rstrip(" \t"):
                fail(line_no, "multiple documents are not supported" if content_seen
                     else "content on the document marker line is not supported")
            content_seen = True
            continue
        if ind == 0 and marker(body, "..."):
            fail(line_no, "document end marker is not supported")
        if ind == 0 and body[0] == "%":
            fail(line_no, "directives are not supported")
        content_seen = True
        if body[0] == "-" and (len(body) == 1 or body[1] in " \t"):
            fail(line_no, "block sequences are not supported")
        reject_indicator(body[0], line_no, "key")
        if body[0] == "?" and (len(body) == 1 or body[1] == " "):
            fail(line_no, "complex keys are not supported")
        if body[0] in "[],":
            fail(line_no, "expected 'key: value'")
        if ind > stack[-1][0]:
            if stack[-1][3]:
                stack[-1][0], stack[-1][3] = ind, False
            elif pending is not None:
                child = {}
                pending[0][pending[1]] = child
                first_line[id(child)] = {}
                stack.append([ind, child, pending[2], False])
            else:
                fail(line_no, "unexpected indentation (the line above opens no map)")
        else:
            while len(stack) > 1 and stack[-1][0] > ind:
                stack.pop()
            if stack[-1][0] != ind:
                if stack[-1][3]:
                    stack[-1][0], stack[-1][3] = ind, False
                else:
                    fail(line_no, "indentation returns to a level that was never opened")
        pending = None
        cur, cur_path = stack[-1][1], stack[-1][2]
        multi = "expected 'key: value' (multi-line scalars are not supported)"
        if body[0] in "\"'":
            key, i = quoted(body, 0, line_no)
            while i < len(body) and body[i] in " \t":
                i += 1
            if i >= len(body) or body[i] != ":":
                fail(line_no, "expected ':' after the quoted key")
        else:
            c = 0
            while True:
                if c >= len(body) or (body[c] == "#" and c > 0 and body[c - 1] in " \t"):
                    fail(line_no, multi)
                if body[c] == ":" and (c + 1 == len(body) or body[c + 1] in " \t"):
                    break
                c += 1
            key, i = body[:c].rstrip(" \t"), c
        if i + 1 < len(body) and body[i + 1] not in " \t":
            fail(line_no, "expected a blank after ':'")
        i += 1
        if key in cur:
            fail(line_no, "duplicate key '%s' (first at line %d)" % (key, first_line[id(cur)][key]))
        first_line[id(cur)][key] = line_no
        path = cur_path + "." + key if cur_path else key
        while i < len(body) and body[i] in " \t":
            i += 1
        if i >= len(body) or body[i] == "#":
            cur[key] = None
            pending = (cur, key, path)
        elif body[i] == "[":
            cur[key], i = flow(body, i, path, line_no)
            trailing(body, i, line_no)
        elif body[i] in "\"'":
            t, i = quoted(body, i, line_no)
            cur[key] = Scalar(t, path, line_no)
            trailing(body, i, line_no)
        else:
            ch = body[i]
            reject_indicator(ch, line_no, "value")
            if ch in "{}":
                fail(line_no, "flow maps are not supported")
            if ch in "|>":
                fail(line_no, "block scalars (| and >) are not supported")
            if ch in "],%@`":
                fail(line_no, "a plain scalar cannot start with '%s'" % ch)
            if ch in "-?" and (i + 1 == len(body) or body[i + 1] == " "):
                fail(line_no, "block sequences are not supported")
            t = strip_comment(body[i:]).rstrip(" \t")
            for c, x in enumerate(t):
                if x == ":" and (c + 1 == len(t) or t[c + 1] in " \t"):
                    fail(line_no, "mapping values are not allowed inside a plain scalar")
            cur[key] = plain(t, path, line_no)
    return root


# ------------------------------------------------------------------ sections -> what the mirror's constructors take
_I, _F, _B, _S = Scalar.as_int, Scalar.as_float, Scalar.as_bool, Scalar.as_str
# key -> conversion, as the reference's .as<T>() call for it (src/raw_gs_model.cpp:16-38, slam_pipeline.cpp:178-187,
# src/pipeline.cpp:9-22, InfiniTAM_tools.cpp:49-59) and as host/*.hpp's configFields read this project's own keys
MODEL_KEYS = dict(render_method=_S, sh_degree=_I, max_init_scale=_F, min_init_scale=_F, sh_degree_interval=_I, default_opacities=_F,
                  means_lr=_F, scales_lr=_F, quats_lr=_F, featuresDc_lr=_F, featuresRest_lr=_F, exposure_lr=_F, use_exposure=_B,
                  opacities_lr=_F, max_gs_radii=_I, delta_depth=_F, isect_capacity=_I, fuse_sh_rest_adam=_I, strip_backward=_B,
                  capacity=_I)
PIPE_KEYS = dict(max_iterations=_I, selected_cam_idx=_I, enable_densify=_B, eval_after_train=_B, save_after_train=_B, log_iter=_I,
                 model_path=_S, log_path=_S, eval_path=_S, new_gs_sample_ratio=_F, keyframe_select_max=_I,
                 localframe_cam_window_length=_I, localframe_cam_window_interval=_I, local_opt_iters=_I, local_opt_interval=_I,
                 color_error_thres=_F, keyframe_theta_thres=_F, keyframe_trans_thres=_F, log_slam_state=_B,
                 ssim_weight=_F, depth_weight=_F, color_error_max=_F, depth_error_max=_F, depth_vis_max=_F, depth_vis_min=_F,
                 alpha_vis_max=_F, sample_method=_S, loss_thres=_F, large_scale_thres=_F, small_scale_thres=_F, low_opac_thres=_F,
                 saved_mesh=_S, saved_engine=_S, saved_images=_S, voxel_size=_F, trunc_dist=_F, viewFrustum_min=_F,
                 viewFrustum_max=_F, use_gt_pose=_B, use_bilateral_filter=_B,
                 refine_iterations=_I, refine_cams=_S, refine_seed=_I, refine_cache_mb=_I)
READER_KEYS = dict(depth_scale=_F, scene_scale=_F, downscale_factor=_F, start_frame=_I, end_frame=_I, frame_step=_I,
                   test_split_interval=_I, input_dir=_S, image_path=_S, pose_path=_S, depth_path=_S, pcd_name=_S)


def refine_settings(pipe_section):
    """This project's optional PIPE keys of the refinement pass (host/slam_pipeline.hpp configFields): refine_iterations (0: off),
    refine_cams ('keyframes' or 'all'), refine_seed (None: the pipeline's seed), refine_cache_mb.  A bad value raises a
    ConfigError that carries the key's path."""
    def get(key, convert, default):
        v = pipe_section.get(key)
        return default if v is None else convert(v)
    out = dict(refine_iterations=get("refine_iterations", _I, 0), refine_cams=get("refine_cams", _S, "keyframes"),
               refine_seed=get("refine_seed", _I, None), refine_cache_mb=get("refine_cache_mb", _I, 16384))
    if out["refine_cams"] not in ("keyframes", "all"):
        v = pipe_section["refine_cams"]
        raise ConfigError("%s: 'keyframes' or 'all', got '%s'" % (getattr(v, "path", "PIPE.refine_cams"), out["refine_cams"]),
                          getattr(v, "line", 0))
    if out["refine_iterations"] < 0:
        v = pipe_section["refine_iterations"]
        raise ConfigError("%s: must not be negative" % getattr(v, "path", "PIPE.refine_iterations"), getattr(v, "line", 0))
    return out


def flatten(section, keys=None):
    """A section (nested dicts with Scalar leaves) -> one flat dict of typed values: nested sections are folded into one namespace
    (PIPE.TSDF.voxel_size -> "voxel_size"), every key with a known type (`keys`, default: MODEL + PIPE + READER) is converted by it,
    a sequence becomes a list of floats, any other scalar stays text."""
    if keys is None:
        keys = dict(READER_KEYS, **dict(MODEL_KEYS, **PIPE_KEYS))
    out = {}
    for k, v in section.items():
        if isinstance(v, dict):
            out.update(flatten(v, keys))
        elif isinstance(v, list):
            out[k] = [x.as_float() for x in v]
        elif v is None:
            out[k] = None
        else:
            out[k] = keys[k](v) if k in keys else str(v)
    return out
