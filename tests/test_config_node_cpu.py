"""gpsh::Node (gps_slam_amd/host/config_node.hpp), the reader for the reference's configuration files, and what sits on it without a
device: the node-typed entry points' templates, the session's small files (cfg_args, cameras.json, pose files) and the Python mirror's
gps_slam_amd/config.py.  Fixtures: the 14 shipped config files (tests/golden/configs/) and one malformed file per rejection rule
(tests/golden/configs_bad/)."""
import glob
import json
import math
import os
import subprocess
import sysconfig
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gps_slam_amd", "host")
GOOD = os.path.join(ROOT, "tests", "golden", "configs")
BAD_DIR = os.path.join(ROOT, "tests", "golden", "configs_bad")
FIXTURES = sorted(glob.glob(os.path.join(GOOD, "**", "*.yaml"), recursive=True))
OFFICE0 = os.path.join(GOOD, "release", "gps_slam", "office0.yaml")

# malformed file -> (line the reader must name, word of the reason)
BAD = {"tab_indent.yaml": (3, "tab"), "block_sequence.yaml": (3, "block sequence"), "anchor.yaml": (3, "anchor"),
       "alias.yaml": (3, "alias"), "tag.yaml": (1, "tag"), "literal_scalar.yaml": (2, "block scalar"),
       "folded_scalar.yaml": (1, "block scalar"), "multiple_documents.yaml": (3, "multiple documents"),
       "flow_map.yaml": (2, "flow map"), "unterminated_quote.yaml": (3, "unterminated quote"),
       "unterminated_bracket.yaml": (3, "unterminated bracket"), "duplicate_key.yaml": (4, "duplicate key"),
       "dedent_to_unopened_level.yaml": (4, "never opened")}


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


def test_fixture_set_is_the_shipped_one():
    names = [os.path.relpath(p, GOOD) for p in FIXTURES]
    assert len(names) == 14 and "release/replica/office0.yaml" in names and "viewer/office0.yaml" in names
    assert sorted(BAD) == sorted(os.path.basename(p) for p in glob.glob(os.path.join(BAD_DIR, "*.yaml")))


def _leaves(node, py):
    """(node, PyYAML value) for every leaf; asserts key sets, nesting, key order and sequence lengths on the way"""
    if isinstance(py, dict):
        assert node.IsMap() and node.keys() == list(py.keys()), node.path
        assert len(node) == len(py)
        for k, v in py.items():
            yield from _leaves(node[k], v)
    elif isinstance(py, list):
        assert node.IsSequence() and len(node) == len(py), node.path
        for i, v in enumerate(py):
            yield from _leaves(node[i], v)
    else:
        yield node, py


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.relpath(p, GOOD))
def test_reader_against_pyyaml(path):
    yaml = pytest.importorskip("yaml")
    h = _host()
    raw = open(path, "rb").read().decode("utf-8")
    py = yaml.safe_load(raw)
    root = h.load_yaml(path)
    tree = root.to_python()
    assert list(tree.keys()) == list(py.keys())
    lines = raw.split("\n")
    n_leaves = exp_strings = 0
    for node, v in _leaves(root, py):
        n_leaves += 1
        text = node.as_str()
        assert node.IsScalar() and 1 <= node.line <= len(lines)
        # the file's text for that scalar stands on the node's line (quotes stripped by the reader)
        assert text in lines[node.line - 1], (node.path, text, lines[node.line - 1])
        if isinstance(v, bool):
            assert node.as_bool() is v
        elif isinstance(v, int):
            assert node.as_double() == v and node.as_int() == v and node.as_int64() == v
        elif isinstance(v, float):
            assert node.as_double() == v
            assert node.as_float() == float(np.float32(v))
        else:
            assert isinstance(v, str) and text == v
            try:
                as_number = float(v)
            except ValueError:
                continue
            # THE TRAP: PyYAML follows YAML 1.1, where a float needs a dot -- `opacities_lr: 5e-2` is the STRING '5e-2' to it;
            # yaml-cpp's as<float>() (stream extraction) gives 0.05, and the reference trains with that
            exp_strings += 1
            assert node.as_double() == as_number and node.as_float() == float(np.float32(as_number))
    assert n_leaves > 80
    assert exp_strings >= 1 and root["MODEL"]["opacities_lr"].as_double() == 0.05   # the case occurs in every shipped file


def test_reader_against_hand_written_expectations():
    h = _host()
    n = h.load_yaml(OFFICE0)
    f32 = lambda x: float(np.float32(x))
    assert n["workspace_dir"].as_str() == "output/release/gps_slam/office0"
    assert n["dev_id"].as_int() == 0 and n["dev_id"].as_str() == "0"        # slam_trainer.cpp:17 and :30
    assert n["work_mode"].as_str() == "train"
    R, P, M = n["READER"], n["PIPE"], n["MODEL"]
    assert R["intrinsics"].as_float_list() == [f32(605.371094), f32(605.245667), f32(635.308594), f32(366.510010)]
    assert R["image_shape"].as_int_list() == [1280, 720]
    assert R["intrinsics"][2].as_double() == 635.308594 and R["intrinsics"][3].as_str() == "366.510010" and R["intrinsics"].IsSequence() and len(R["intrinsics"]) == 4
    assert R["depth_scale"].as_float() == 1000.0 and R["scene_scale"].as_float() == 1.0
    assert R["downscale_factor"].as_float() == 1.0 and R["downscale_factor"].as_int() == 1   # trailing blanks and a comment behind it
    assert R["end_frame"].as_int() == R["end_frame"].as_int64() and R["test_split_interval"].as_int() == -1
    assert R["pcd_name"].as_str() == "sampled_pcd_50w.ply" and R["input_dir"].IsScalar()
    assert P["model_path"].as_str() == "/gs_model" and P["log_path"].as_str() == "/log" and P["eval_path"].as_str() == "/val"
    assert P["enable_densify"].as_bool() is False and P["save_after_train"].as_bool() is True
    assert P["max_iterations"].as_int() == 10000 and P["keyframe_select_max"].as_int() == 7
    assert P["keyframe_theta_thres"].as_float() == 30.0 and P["keyframe_trans_thres"].as_float() == f32(0.3)
    assert P["weight_configs"]["ssim_weight"].as_float() == 0.0 and P["vis_configs"]["depth_vis_max"].as_float() == 5.0
    assert P["keyframe_sample_configs"]["sample_method"].as_str() == "random"
    assert P["remove_configs"]["small_scale_thres"].as_float() == f32(0.003)
    T = P["TSDF"]
    assert T["voxel_size"].as_float() == f32(0.005) and T["voxel_size"].path == "PIPE.TSDF.voxel_size"
    assert T["use_gt_pose"].as_bool() is True and T["viewFrustum_max"].as_float() == 10.0
    assert T["saved_mesh"].as_str() == "" and T["saved_mesh"].IsScalar() and T["saved_mesh"].IsDefined()
    assert T["saved_engine"].as_str() == "tsdf_engine/" and T["saved_images"].as_str() == "raycasted"
    assert M["min_init_scale"].as_float() == -1.0 and M["min_init_scale"].as_int() == -1
    assert M["sh_degree"].as_int() == 3 and M["opacities_lr"].as_float() == f32(0.05) and M["use_exposure"].as_bool() is False
    assert M["means_lr_final"].as_double() == 0.0000016
    assert P.IsMap() and not P.IsScalar() and len(P) == len(P.keys()) and P.keys()[0] in ("train_method", "train_mode")
    # a missing key, an index out of range, an index into a scalar: undefined, and undefined again when indexed
    for miss in (n["nope"], P["TSDF"]["voxel"], R["intrinsics"][4], T["voxel_size"]["x"], n["a"]["b"][3]["c"], R["intrinsics"][-1]):
        assert not miss.IsDefined() and not miss.IsMap() and not miss.IsScalar() and len(miss) == 0
    with pytest.raises(ValueError, match=r"PIPE\.TSDF\.voxel\.deeper\[2\]") as e:
        P["TSDF"]["voxel"]["deeper"][2].as_float()
    assert isinstance(e.value, h.ConfigError)
    with pytest.raises(h.ConfigError) as e:
        T["voxel_size"].as_int()
    msg = str(e.value)
    assert "PIPE.TSDF.voxel_size" in msg and "'0.005'" in msg and "office0.yaml:%d" % T["voxel_size"].line in msg
    assert open(OFFICE0).read().split("\n")[T["voxel_size"].line - 1].strip() == "voxel_size: 0.005"
    with pytest.raises(h.ConfigError, match="PIPE.TSDF"):
        T.as_float()                       # a map is no number
    with pytest.raises(h.ConfigError, match="READER.intrinsics"):
        R["intrinsics"].as_int_list()      # 605.37 is no int


@pytest.mark.parametrize("name", sorted(BAD))
def test_rejections_name_the_line(name):
    h = _host()
    line, word = BAD[name]
    path = os.path.join(BAD_DIR, name)
    with pytest.raises(h.ConfigError) as e:
        h.load_yaml(path)
    assert "%s:%d: " % (path, line) in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(h.ConfigError, match=r"^line %d: " % line):
        h.parse_yaml(open(path, "rb").read().decode())


def test_accepted_forms_and_more_rejections_on_snippets():
    h = _host()
    ok = h.parse_yaml('a: 1\r\nb:   "x # y"   # c\r\n\r\nc: \'it\'\'s\'\nd:\n  e: [1, "2", \'3\' , 4.5]   \n  f: []\n# end\ng: no newline at the end')
    assert ok.to_python() == {"a": "1", "b": "x # y", "c": "it's", "d": {"e": ["1", "2", "3", "4.5"], "f": []}, "g": "no newline at the end"}
    assert ok["d"]["e"][3].path == "d.e[3]" and ok["g"].line == 9 and ok["d"]["e"].as_float_list() == [1.0, 2.0, 3.0, 4.5]
    assert h.parse_yaml("").to_python() == {} and h.parse_yaml("\n\n# only a comment\n").to_python() == {}
    empty = h.parse_yaml("a:\nb: ~\nc: null\n")
    assert empty.to_python() == {"a": None, "b": None, "c": None} and empty["a"].IsNull() and empty["a"].IsDefined()
    assert empty["a"].as_str() == "null"            # yaml-cpp's as<std::string>() of a Null node
    with pytest.raises(h.ConfigError):
        empty["a"].as_int()
    assert h.parse_yaml("---\na: 1\n")["a"].as_int() == 1
    for text, line in (("a: 1\n  b: 2\n", 2), ("a: [1, [2]]\n", 1), ("a: [1, 2] x\n", 1), ('a: "x" y\n', 1), ("just text\n", 1),
                       ("a: 1\n? b\n", 2), ("a: b: c\n", 1), ("a:\n  b: 1\n c: 2\n", 3), ("%YAML 1.2\n", 1), ("a: 1\n...\n", 2),
                       ("a: [1,, 2]\n", 1), ('a: "\\q"\n', 1), ("a: {}\n", 1), ("a: 'x\n", 1), ("a: !!int 3\n", 1), ("- a\n", 1),
                       ("a: 1\na : 2\n", 2)):
        with pytest.raises(h.ConfigError, match=r"^line %d: " % line):
            h.parse_yaml(text)


def test_conversion_rules_on_literals():
    h = _host()
    conv = lambda text, how: getattr(h.parse_yaml("v: " + text + "\n")["v"], how)()
    # bool: y/n, yes/no, true/false, on/off in lower, Capitalised and UPPER form -- and nothing else
    for word, value in (("y", True), ("n", False), ("yes", True), ("no", False), ("true", True), ("false", False), ("on", True), ("off", False)):
        for form in (word, word.capitalize(), word.upper()):
            assert conv(form, "as_bool") is value, form
    for bad in ("tRue", "yEs", "oN", "1", "0", "t", "ja", '""'):
        with pytest.raises(h.ConfigError, match="to bool"):
            conv(bad, "as_bool")
    # numbers: stream extraction, whole token
    assert conv("5e-2", "as_double") == 0.05 and conv("5e-2", "as_float") == float(np.float32(0.05))
    assert conv("1", "as_float") == 1.0 and conv("-1", "as_int") == -1 and conv("+7", "as_int") == 7
    assert conv("1.", "as_double") == 1.0 and conv(".5", "as_double") == 0.5 and conv("1E3", "as_double") == 1000.0
    assert conv("0x1F", "as_int") == 31 and conv("010", "as_int") == 8          # basefield unset, as yaml-cpp leaves it
    assert conv('"12"', "as_int") == 12                                         # a quoted scalar is text like any other
    assert conv("4294967296", "as_int64") == 1 << 32
    assert math.isinf(conv(".inf", "as_double")) and conv("-.INF", "as_double") < 0 and math.isnan(conv(".NaN", "as_float"))
    for bad, how in (("1.5", "as_int"), ("5e-2", "as_int"), ("1e3", "as_int"), ("abc", "as_double"), ("1.5x", "as_double"), ("1 2", "as_double"),
                     ("4294967296", "as_int"), ("0.005", "as_int64"), ("08", "as_int"), ("1e999", "as_double"), ("1e60", "as_float"),
                     ("inf", "as_double"), ("[1]", "as_double"), ("--1", "as_int")):
        with pytest.raises(h.ConfigError, match="cannot convert"):
            conv(bad, how)
    # std::string: the text of any scalar
    assert conv("0", "as_str") == "0" and conv("5e-2", "as_str") == "5e-2" and conv("true", "as_str") == "true"
    with pytest.raises(h.ConfigError):
        conv("[1, 2]", "as_str")
    assert conv("[1, 2.5]", "as_float_list") == [1.0, 2.5]
    with pytest.raises(h.ConfigError, match=r"v\[1\]"):
        conv("[1, 2.5]", "as_int_list")
    with pytest.raises(h.ConfigError):
        conv("3", "as_int_list")


def test_host_sanitizer_stand_alone(tmp_path):
    """config_node.hpp alone under AddressSanitizer + UBSan, as a plain process: every fixture, every malformed file, every prefix
    of every fixture, and seeded single-byte substitutions; every as<T>() on everything that parses.  The inputs are split over
    side-by-side processes (most of the time is the exceptions of the failing conversions, five per scalar): all prefixes, and
    250 of the 2,000 substitutions per file the plan named -- the count that keeps the run well under 20 s."""
    exe = str(tmp_path / "config_node_main")
    # the sanitizer runtimes are linked statically: the driver then runs in whatever environment the suite runs in, as it is
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-I", HOST,
           os.path.join(ROOT, "tests", "config_node_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr   # (a missing sanitizer runtime fails here, with the compiler's message)
    shards = max(1, min(8, len(os.sched_getaffinity(0))))
    t0 = time.time()
    procs = [subprocess.Popen([exe, GOOD, BAD_DIR, "250", str(s), str(shards)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for s in range(shards)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0 and "config_node_main ok: 14 fixtures, 13 malformed" in out, out[-4000:]
        assert "ERROR" not in out and "runtime error" not in out, out[-4000:]
    print("config_node_main: %d shards, %.1f s" % (shards, time.time() - t0))


def test_templates_need_only_yaml_cpps_surface():
    """tests/config_templates_unit.cpp instantiates the five node-typed entry points with a FakeYamlNode that has a const
    operator[], as<T>() and IsDefined() and nothing else (what YAML::Node offers), and with gpsh::Node: it must compile."""
    import torch
    from torch.utils import cpp_extension as ce
    inc = ce.include_paths() + ["/opt/rocm/include", sysconfig.get_paths()["include"], os.path.join(ROOT, "include"), HOST]
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
           "-D_GLIBCXX_USE_CXX11_ABI=%d" % int(torch._C._GLIBCXX_USE_CXX11_ABI), "-Wno-deprecated-declarations"]
    cmd += ["-I" + p for p in inc] + [os.path.join(ROOT, "tests", "config_templates_unit.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_node_entry_points_reject_missing_and_unknown_keys_before_anything_is_built():
    h = _host()
    text = open(OFFICE0).read()
    root = h.parse_yaml(text, "office0.yaml")
    reader = h.DatasetReader()
    reader.loadConfig(root["READER"])
    assert (reader.width, reader.height) == (1280, 720)
    assert [reader.fx, reader.fy, reader.cx, reader.cy] == [float(np.float32(v)) for v in (605.371094, 605.245667, 635.308594, 366.510010)]
    assert reader.scene_scale == float(np.float32(1.1) * np.float32(1.0)) and reader.depth_scale == 1000.0   # dataset_reader.cpp:231
    pipe = h.SLAMPipeline(1)
    pipe.loadConfig(root["PIPE"], "some/where", False)
    s = pipe.settings()
    assert s["model_path_full"] == "some/where/gs_model" and s["eval_path_full"] == "some/where/val" and s["log_path_full"] == "some/where/log"
    assert s["TSDF.saved_engine"] == "tsdf_engine/" and s["keyframe_select_max"] == 7 and s["save_after_train"] is True
    assert s["remove_configs.low_opac_thres"] == float(np.float32(0.005)) and s["keyframe_sample_configs.loss_thres"] == float(np.float32(0.02))
    assert not os.path.exists("some/where")      # is_train = False creates nothing

    def edited(old, new):
        assert old in text
        return h.parse_yaml(text.replace(old, new), "edited.yaml")

    # a key the reference reads with .as<T>() is required: its full path is in the message
    for section, old, path, call in (
            ("MODEL", "  sh_degree: 3 \n", "MODEL.sh_degree", lambda n: h.SLAMGaussianModel().loadConfig(n)),
            ("PIPE", "    voxel_size: 0.005\n", "PIPE.TSDF.voxel_size", lambda n: h.createTsdfEngine(reader, n["TSDF"])),
            ("PIPE", "    low_opac_thres: 0.005\n", "PIPE.remove_configs.low_opac_thres", lambda n: h.SLAMPipeline(1).loadConfig(n, "x", False)),
            ("PIPE", "  eval_path: \"/val\"\n", "PIPE.eval_path", lambda n: h.SLAMPipeline(1).loadConfig(n, "x", False)),
            ("PIPE", "    saved_images: raycasted\n", "PIPE.TSDF.saved_images", lambda n: h.SLAMPipeline(1).loadConfig(n, "x", False)),
            ("READER", "  scene_scale: 1.0\n", "READER.scene_scale", lambda n: h.DatasetReader().loadConfig(n))):
        with pytest.raises(h.ConfigError, match=path.replace(".", r"\.") + ": required key is missing"):
            call(edited(old, "")[section])
    # a typo in a key (here: of one this project added, which is optional) is an unknown key, with its path and line
    for section, old, new, path, call in (
            ("MODEL", "  delta_depth: 0.1\n", "  delta_depth: 0.1\n  capacty: 4096\n", "MODEL.capacty", lambda n: h.SLAMGaussianModel().loadConfig(n)),
            ("PIPE", "    use_gt_pose: true\n", "    use_gt_pose: true\n    voxelsize: 1\n", "PIPE.TSDF.voxelsize", lambda n: h.createTsdfEngine(reader, n["TSDF"])),
            ("PIPE", "  log_slam_state: false\n", "  log_slam_state: false\n  overlap_maping: true\n", "PIPE.overlap_maping", lambda n: h.SLAMPipeline(1).loadConfig(n, "x", False)),
            ("PIPE", "    ssim_weight: 0.0\n", "    ssim_weight: 0.0\n    l2_weight: 0.0\n", "PIPE.weight_configs.l2_weight", lambda n: h.SLAMPipeline(1).loadConfig(n, "x", False)),
            ("READER", "  frame_step: 1\n", "  frame_step: 1\n  framestep: 1\n", "READER.framestep", lambda n: h.DatasetReader().loadConfig(n))):
        with pytest.raises(h.ConfigError, match=path.replace(".", r"\.") + r": unknown key \(edited\.yaml:\d+\)"):
            call(edited(old, new)[section])
    # a value of the wrong type, densification, a resized reader
    with pytest.raises(h.ConfigError, match=r"PIPE\.local_opt_iters.*'2\.5' to int"):
        h.SLAMPipeline(1).loadConfig(edited("  local_opt_iters: 20\n", "  local_opt_iters: 2.5\n")["PIPE"], "x", False)
    with pytest.raises(h.ConfigError, match=r"PIPE\.enable_densify"):
        h.SLAMPipeline(1).loadConfig(edited("  enable_densify: false\n", "  enable_densify: true\n")["PIPE"], "x", False)
    with pytest.raises(h.ConfigError, match=r"READER\.downscale_factor"):
        h.DatasetReader().loadConfig(edited("  downscale_factor: 1 ", "  downscale_factor: 2 ")["READER"])
    with pytest.raises(h.ConfigError, match=r"READER\.intrinsics"):
        h.DatasetReader().loadConfig(edited("[605.371094, 605.245667, 635.308594, 366.510010]", "[605.371094, 605.245667]")["READER"])
    assert not os.path.exists("x")
    # this project's optional keys are read where they are given
    p2 = h.SLAMPipeline(1)
    p2.loadConfig(edited("  log_slam_state: false\n", "  log_slam_state: false\n  overlap_mapping: true\n  fused_loss_terms: yes\n")["PIPE"], "x", False)
    assert p2.overlap_mapping is True and p2.fused_loss_terms is True and pipe.overlap_mapping is False


def test_session_files_on_host_tensors(tmp_path):
    import torch
    h = _host()
    # cfg_args: byte for byte the line saveCfgArgs writes
    h.write_cfg_args(str(tmp_path / "cfg_args"), 3)
    assert open(tmp_path / "cfg_args", "rb").read() == (b"Namespace(data_device='cuda', eval=False, images='images', model_path='', "
                                                       b"resolution=-1, sh_degree=3, source_path='', white_background=False)\n")
    # cameras.json
    rng = np.random.default_rng(5)
    cams, poses = [], []
    values = [(600.0, 599.5), (605.37, 605.24), (0.1, 1e-5), (1234567.0, 3.0e10), (16777216.0, 1.17549435e-38)]
    for i, (fx, fy) in enumerate(values):
        c2w = np.eye(4, dtype=np.float32)
        c2w[:3, :4] = rng.standard_normal((3, 4)).astype(np.float32) * np.float32(10.0 ** (i - 2))
        cam = h.Camera(64 + i, 48, fx, fy, 32.0, 24.0, True, torch.as_tensor(np.eye(4, dtype=np.float32)))
        cam.id = 10 + i                       # "id" in the file is the INDEX (dataset_reader.cpp:429)
        cam.c2w_slam = torch.as_tensor(c2w)
        if i != 1:
            cam.img_name = "frame%06d.jpg" % (7 * i)
        cams.append(cam)
        poses.append(c2w)
    h.write_cameras_json(str(tmp_path / "cameras.json"), cams)
    raw = open(tmp_path / "cameras.json").read()
    assert raw == h.cameras_json(cams) and " " not in raw and "\n" not in raw            # nlohmann's compact dump
    assert raw.startswith('[{"fx":600.0,"fy":599.5,"height":48,"id":0,"img_name":"frame000000.jpg","position":[')
    assert '"fx":0.10000000149011612,"fy":9.999999747378752e-06,' in raw and '"fx":1234567.0,"fy":30000001024.0,' in raw
    assert '"fx":16777216.0,"fy":1.1754943508222875e-38,' in raw
    data = json.loads(raw)
    assert len(data) == 5
    for i, (d, (fx, fy)) in enumerate(zip(data, values)):
        assert list(d.keys()) == ["fx", "fy", "height", "id", "img_name", "position", "rotation", "width"]   # alphabetical
        assert d["id"] == i and d["width"] == 64 + i and d["height"] == 48 and d["img_name"] == ("" if i == 1 else "frame%06d.jpg" % (7 * i))
        # every number reads back to exactly the float32 that went in (and is that float32's value, not a rounder neighbour)
        assert d["fx"] == float(np.float32(fx)) and d["fy"] == float(np.float32(fy))
        got = np.array([r + [p] for r, p in zip(d["rotation"], d["position"])], np.float64)
        assert np.array_equal(got, poses[i][:3, :4].astype(np.float64))
        assert np.array_equal(got.astype(np.float32), poses[i][:3, :4])
    # a pose file: four lines of four numbers with six decimals (saveTensorTXT)
    pose = np.array([[0.5, -0.25, 1e-7, 12.3456789], [1, 0, 0, -3.0000004], [0, 1, 0, 100.5], [0, 0, 0, 1]], np.float32)
    h.write_pose_txt(str(tmp_path / "frame000003.txt"), torch.as_tensor(pose))
    text = open(tmp_path / "frame000003.txt").read()
    assert text == h.pose_txt(torch.as_tensor(pose))
    rows = text.split("\n")
    assert len(rows) == 5 and rows[4] == "" and rows[0] == "0.500000 -0.250000 0.000000 12.345679" and rows[3] == "0.000000 0.000000 0.000000 1.000000"
    for row, want in zip(rows[:4], pose):
        toks = row.split(" ")
        assert len(toks) == 4 and all(len(t.split(".")[1]) == 6 for t in toks)
        assert [float(t) for t in toks] == [float("%.6f" % v) for v in want]
    back = h.read_pose_txt(str(tmp_path / "frame000003.txt")).numpy()
    assert np.abs(back - pose).max() <= 0.5e-6 * 1.0001 + np.spacing(np.float32(100.5))
    # savePoses names the files like DatasetReader::savePose: the frame id of the image's name, else the camera's id
    files = h.SLAMPipeline(1).savePoses(str(tmp_path / "pose"), cams)
    assert [os.path.basename(f) for f in files] == ["frame000000.txt", "frame000011.txt", "frame000014.txt", "frame000021.txt", "frame000028.txt"]
    assert open(files[2]).read() == h.pose_txt(cams[2].c2w_slam)
    # createWorkSpace: the file's workspace_dir, emptied, with a copy of the file
    ws = tmp_path / "out" / "ws"
    os.makedirs(ws)
    open(ws / "stale.txt", "w").write("x")
    cfg = tmp_path / "run.yaml"
    cfg.write_text(open(OFFICE0).read().replace("output/release/gps_slam/office0", str(ws)))
    assert h.create_work_space(str(cfg)) == str(ws)
    assert sorted(os.listdir(ws)) == ["run.yaml"] and open(ws / "run.yaml").read() == cfg.read_text()


# ------------------------------------------------------------------ gps_slam_amd/config.py (the Python mirror's entry)
def test_python_reader_is_the_same_grammar():
    from gps_slam_amd import config
    h = _host()
    for path in FIXTURES:
        text = open(path, "rb").read().decode()
        a, b = config._parse_python(text, path), h.load_yaml(path).to_python()
        assert a == b and list(a) == list(b) and list(a["PIPE"]) == list(b["PIPE"]), path
        assert config.load_yaml(path) == a
        assert a["PIPE"]["TSDF"]["voxel_size"].path == "PIPE.TSDF.voxel_size" and a["READER"]["intrinsics"][1].path == "READER.intrinsics[1]"
    for name, (line, word) in BAD.items():
        text = open(os.path.join(BAD_DIR, name), "rb").read().decode()
        for parse in (config._parse_python, config.parse_yaml):
            with pytest.raises(config.ConfigError) as e:
                parse(text, name)
            assert e.value.line == line and ("%s:%d: " % (name, line)) in str(e.value) and word in str(e.value)
    # every prefix of a fixture: the two readers accept and reject the same inputs, with the same tree / the same line
    text = open(OFFICE0, "rb").read().decode()
    for cut in range(0, len(text), 7):
        try:
            want = h.parse_yaml(text[:cut]).to_python()
        except h.ConfigError as e:
            with pytest.raises(config.ConfigError) as pe:
                config._parse_python(text[:cut])
            assert str(pe.value) == str(e)
            continue
        assert config._parse_python(text[:cut]) == want
    snippet = 'a: 1\r\nb:   "x # y"   # c\r\nc: \'it\'\'s\'\nd:\n  e: [1, "2", \'3\' , 4.5]   \n  f: []\ng:\nh: ~'
    assert config._parse_python(snippet) == h.parse_yaml(snippet).to_python()


def test_python_scalars_convert_like_the_node():
    from gps_slam_amd import config
    h = _host()
    words = ["5e-2", "1", "-1", "+7", "1.", ".5", "1E3", "0x1F", "010", "08", "1.5", "abc", "1.5x", "1e3", "--1", "inf", ".inf", "-.INF", ".NaN",
             "y", "N", "Yes", "NO", "true", "False", "on", "OFF", "tRue", "oN", "0.005", "600", "1_000", "0b1", "1e", "e5", "+.5", "-0", "0"]
    for w in words:
        node = h.parse_yaml("v: " + w + "\n")["v"]
        s = config.Scalar(w, "v", 1)
        for mine, theirs in ((s.as_int, node.as_int64), (s.as_float, node.as_double), (s.as_bool, node.as_bool), (s.as_str, node.as_str)):
            try:
                want = theirs()
            except h.ConfigError:
                with pytest.raises(config.ConfigError, match="cannot convert '%s'" % w.replace("+", r"\+").replace(".", r"\.")):
                    mine()
                continue
            got = mine()
            assert got == want or (isinstance(want, float) and math.isnan(want) and math.isnan(got)), (w, got, want)
            assert type(got) is type(want)


def test_flatten_and_from_config_feed_the_mirror():
    from gps_slam_amd import config
    from gps_slam_amd.slam_pipeline import DEFAULT_PIPE, SLAMPipeline
    nested = config.load_yaml(os.path.join(GOOD, "release", "replica", "office0.yaml"))
    model = config.flatten(nested["MODEL"], config.MODEL_KEYS)
    assert model["sh_degree"] == 3 and model["opacities_lr"] == 0.05 and model["use_exposure"] is False and model["render_method"] == "ges"
    assert model["min_init_scale"] == -1.0 and model["means_lr"] == 0.00016 and isinstance(model["max_gs_radii"], int)
    flat = config.flatten(nested["PIPE"])
    assert flat["voxel_size"] == 0.005 and flat["use_gt_pose"] is True and flat["saved_mesh"] == "tsdf_mesh.ply" and flat["sample_method"] == "random"
    assert flat["low_opac_thres"] == 0.005 and flat["ssim_weight"] == 0.0 and flat["model_path"] == "/gs_model" and flat["train_mode"] == "ges"
    assert config.flatten(nested["READER"])["intrinsics"] == [600.0, 600.0, 599.5, 339.5]

    class _Model:
        device = "cpu"

    pipe = SLAMPipeline.from_config(nested, None, _Model(), seed=3)
    for k in DEFAULT_PIPE:
        if k != "scene_scale":
            assert pipe.cfg[k] == flat[k] and type(pipe.cfg[k]) is type(DEFAULT_PIPE[k]), k
    assert pipe.cfg["scene_scale"] == float(np.float32(1.1) * np.float32(1.0))
    assert pipe.work_mode == "train" and pipe.use_gt_pose is True and pipe.workspace_dir == "output/release/replica/office0"
    assert pipe.saved_mesh == "tsdf_mesh.ply" and pipe.saved_engine == "tsdf_engine/"
    nested["PIPE"]["enable_densify"] = config.Scalar("true", "PIPE.enable_densify", 28)
    with pytest.raises(config.ConfigError, match="enable_densify"):
        SLAMPipeline.from_config(nested, None, _Model())


def test_node_iterates_in_python():
    h = _host()
    n = h.parse_yaml("a: 1\nb:\n  c: [x, y, z]\n")
    assert list(n) == ["a", "b"] == n.keys() and [e.as_str() for e in n["b"]["c"]] == ["x", "y", "z"]
    assert list(n["b"]["c"])[2].path == "b.c[2]" and list(h.parse_yaml("")) == []
    for not_iterable in (n["a"], n["nope"], h.parse_yaml("a:\n")["a"]):
        with pytest.raises(TypeError):
            iter(not_iterable)


def test_flat_route_does_not_read_the_schedule_keys():
    """a gpsh::Config never carried overlap_mapping ... log_pipeline_time into the pipeline and still does not; a node does"""
    h = _host()
    p = h.SLAMPipeline(1)
    p.loadConfig(dict())                       # (the output paths are composed by the first loadConfig)
    before = p.settings()
    p.loadConfig(dict(overlap_mapping=1, mapping_thread=1, async_raycasts=0, pipeline_raycasts=0, merge_keyframe_raycasts=1,
                      prefetch_next_preprocess=0, log_pipeline_time=1))
    assert p.settings() == before and p.overlap_mapping is False and p.async_raycasts is True
    p.loadConfig(dict(fused_loss_terms=1, local_opt_iters=3))      # what the flat route has always read
    assert p.fused_loss_terms is True and p.settings()["local_opt_iters"] == 3


def test_python_wrapper_keeps_lines_and_paths():
    from gps_slam_amd import config
    nested = config.load_yaml(OFFICE0)
    v = nested["PIPE"]["TSDF"]["voxel_size"]
    assert v.path == "PIPE.TSDF.voxel_size" and v.line == 70 and nested["READER"]["intrinsics"][3].line == 18
    with pytest.raises(config.ConfigError, match=r"PIPE\.TSDF\.voxel_size \(line 70\): cannot convert '0\.005' to int") as e:
        v.as_int()
    assert e.value.line == 70
    py = config._parse_python(open(OFFICE0).read(), OFFICE0)
    assert py["PIPE"]["TSDF"]["voxel_size"].line == 70 and py["MODEL"]["sh_degree"].line == nested["MODEL"]["sh_degree"].line == 87


def test_directories_that_are_never_emptied(tmp_path, monkeypatch):
    import torch
    h = _host()
    work = tmp_path / "work"
    (work / "sub").mkdir(parents=True)
    (work / "keep.txt").write_text("x")
    monkeypatch.chdir(work / "sub")
    text = open(OFFICE0).read()
    for n, ws in enumerate((".", "..", str(work), str(tmp_path))):
        cfg = tmp_path.parent / ("cfg_%s_%d.yaml" % (tmp_path.name, n))
        cfg.write_text(text.replace("output/release/gps_slam/office0", ws))
        with pytest.raises(RuntimeError, match="refusing to empty"):
            h.create_work_space(str(cfg))
        os.remove(cfg)
    assert (work / "keep.txt").read_text() == "x"
    # a config file inside its own workspace_dir
    inside = work / "run.yaml"
    inside.write_text(text.replace("output/release/gps_slam/office0", str(work)))
    monkeypatch.chdir(tmp_path.parent)
    with pytest.raises(RuntimeError, match="lies inside its own workspace_dir"):
        h.create_work_space(str(inside))
    assert inside.is_file() and (work / "keep.txt").is_file()
    # nlohmann's short escapes in a name
    cam = h.Camera(4, 4, 1.0, 1.0, 2.0, 2.0, True, torch.eye(4))
    cam.img_name = 'a"b\\c\n\t\x01'
    raw = h.cameras_json([cam])
    assert '"img_name":"a\\"b\\\\c\\n\\t\\u0001"' in raw and json.loads(raw)[0]["img_name"] == cam.img_name
