"""Generates tests/golden/rgbd_calib.npz and tests/golden/rgbd_calib_<run>.txt: what the REFERENCE's own view builder and CPU engine
(InfiniTAM/ITMLib + ORUtils etc., read in place under the reference root, compiled together with
tests/golden/rgbd_calib_ref_driver.cpp into a temporary directory: -O2 -std=c++17 -DCOMPILE_WITHOUT_CUDA -ffp-contract=off, no
OpenMP) compute with a full ITMRGBDCalib on the cases of tests/rgbd_calib_cases.py: a colour camera of its own, disparity
input, an affine depth scale, the bilateral filter on calibrated depth.  Only data is stored: the converted image of every
conversion-only case; for the engine runs a CRC (tests/digests.crc) of every digest after every frame, the poses, calib_inv and
M_rgb, the calibration text the reference wrote, and one frame's depth and ORIGINAL_RGB image in full.  The inputs are NOT
stored: the tests regenerate them (rgbd_calib_cases.make_run / conv_raw).

The generator refuses to write a fixture that does not contain what the tests rely on (see main).

Run from the repo root:  python tests/golden/make_rgbd_calib_golden.py"""
import glob
import os
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import rgbd_calib_cases as cases  # noqa: E402
from tests.digests import crc, frame_digest  # noqa: E402

REF = os.path.join(os.environ.get("GPS_REFERENCE_ROOT", "/root/reference"), "InfiniTAM")
FLAGS = ["-O2", "-std=c++17", "-DCOMPILE_WITHOUT_CUDA", "-ffp-contract=off", "-w", "-I" + REF]
VOXEL_DT = np.dtype([("sdf", "<i2"), ("w_depth", "u1"), ("clr", "u1", (3,)), ("w_color", "u1"), ("pad", "u1")])


def build_driver(tmp):
    pats = ["ITMLib/CPUInstantiations.cpp", "ITMLib/Engines/LowLevel/*Factory.cpp", "ITMLib/Engines/LowLevel/CPU/*.cpp",
            "ITMLib/Engines/ViewBuilding/*Factory.cpp", "ITMLib/Engines/ViewBuilding/CPU/*.cpp",
            "ITMLib/Engines/Visualisation/Interface/*.cpp", "ITMLib/Objects/Camera/*.cpp", "ITMLib/Objects/RenderStates/*.cpp",
            "ITMLib/Trackers/CPU/*.cpp", "ITMLib/Trackers/Interface/*.cpp", "ITMLib/Utils/*.cpp", "ITMLib/Engines/MultiScene/*.cpp",
            "ORUtils/*.cpp", "FernRelocLib/FernConservatory.cpp", "FernRelocLib/PoseDatabase.cpp", "FernRelocLib/RelocDatabase.cpp",
            "MiniSlamGraphLib/*.cpp"]
    drv = os.path.join(HERE, "rgbd_calib_ref_driver.cpp")
    jobs = [(s, os.path.join(tmp, "%03d.o" % i)) for i, s in enumerate(s for p in pats for s in sorted(glob.glob(os.path.join(REF, p))))]
    jobs.append((drv, os.path.join(tmp, "drv.o")))
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda j: subprocess.check_call(["g++"] + FLAGS + ["-c", j[0], "-o", j[1]]), jobs))
    exe = os.path.join(tmp, "rgbd_calib_ref_driver")
    subprocess.check_call(["g++", "-o", exe] + [j[1] for j in reversed(jobs)] + ["-lpthread"])
    return exe


_DT = {"age": np.int32, "counts": np.int32, "visible_ids": np.int32, "vis_type_nz": np.int32, "hash": np.int32, "vba_crc": np.uint32,
       "img0": np.uint8, "img0_dims": np.int32, "calib_txt": np.uint8, "reread": np.int32, "vba_last": np.uint8}


def read_chunks(path, W, H):
    raw = open(path, "rb").read()
    out, off = {}, 0
    while off < len(raw):
        name = raw[off:off + 32].split(b"\0")[0].decode()
        frame, nbytes = struct.unpack_from("<iq", raw, off + 32)
        off += 44
        a = np.frombuffer(raw[off:off + nbytes], _DT.get(name, np.float32)).copy()
        if name in ("raycast", "icp_points", "icp_normals"):
            a = a.reshape(H, W, 4)
        elif name == "minmax":
            a = a.reshape(H, W, 2)
        elif name == "depth_f":
            a = a.reshape(H, W)
        elif name == "hash":
            a = a.reshape(-1, 6)
        elif name == "vis_type_nz":
            a = a.reshape(-1, 2)
        out[(name, frame)] = a
        off += nbytes
    return out


def run_conv(exe, tmp, raw, typ, a, b, fx, filt):
    H, W = raw.shape
    fin, fout = os.path.join(tmp, "cin.bin"), os.path.join(tmp, "cout.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4i3f", W, H, typ, 1 if filt else 0, a, b, fx))
        f.write(np.ascontiguousarray(raw, np.int16).tobytes())
    subprocess.check_call([exe, "conv", fin, fout])
    return read_chunks(fout, W, H)[("depth_f", 0)]


def run_engine(exe, tmp, run):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    typ, a, b = run["calib"]
    with open(fin, "wb") as f:
        f.write(struct.pack("<9i", 0x47505343, run["Wd"], run["Hd"], run["Wc"], run["Hc"], run["n"], typ, 1 if run["filt"] else 0,
                            1 if run["mode"] == "track" else 0))
        f.write(struct.pack("<8f", *run["intr_d"], *run["intr_c"]))
        f.write(cases.to_orutils(run["ext"]).tobytes())
        f.write(struct.pack("<6f", a, b, cases.VOXEL, cases.MU, cases.VF_MIN, cases.VF_MAX))
        for k in range(run["n"]):
            f.write(np.ascontiguousarray(run["rgb"][k]).tobytes())
            f.write(np.ascontiguousarray(run["raw"][k]).tobytes())
            f.write(np.ascontiguousarray(run["c2w"][k], dtype=np.float32).tobytes())
    subprocess.check_call([exe, "engine", fin, fout], stdout=subprocess.DEVNULL)
    return read_chunks(fout, run["Wd"], run["Hd"])


def near_surface_counts(vba_bytes):
    """(voxels near the surface with w_depth > 0 and w_color > 0, the same with w_color == 0); near the surface: |sdf| within a
    quarter of the band, where the integration takes colour"""
    v = vba_bytes.view(VOXEL_DT)
    near = (np.abs(v["sdf"].astype(np.int32)) <= 32767 // 4) & (v["w_depth"] > 0)
    return int((near & (v["w_color"] > 0)).sum()), int((near & (v["w_color"] == 0)).sum())


TRACK_BOUND = 2e-5   # the tracker's pose tolerance against the reference


def tracked_sensitivity(exe, tmp, run, M):
    """how far the REFERENCE's own tracked poses move when one raw pixel of every frame changes by one unit -- the smallest change
    its input can take -- worst matrix entry per frame over three seeded trials.  A frame where this is not well inside
    TRACK_BOUND is a frame where the reference's LM loop takes another branch for a rounding-sized cause; the bound then
    measures the sequence, not the code compared with it."""
    n = run["n"]
    worst = np.zeros(n)
    for trial in range(3):
        rng = np.random.default_rng(trial)
        raw = run["raw"].copy()
        for f in range(n):
            y, x = rng.integers(10, run["Hd"] - 10), rng.integers(10, run["Wd"] - 10)
            raw[f, y, x] += 1
        p = run_engine(exe, tmp, dict(run, raw=raw))
        M2 = np.stack([p[("M", f)] for f in range(n)])
        worst = np.maximum(worst, np.abs(M2 - M).reshape(n, -1).max(1))
    return worst


def main():
    fix = dict(voxel=np.float32(cases.VOXEL), mu=np.float32(cases.MU), vf_min=np.float32(cases.VF_MIN), vf_max=np.float32(cases.VF_MAX),
               run_names=np.array(sorted(cases.RUNS)), conv_fx=np.float32(cases.CONV_FX))
    texts = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        # ---- conversion-only images: the full converted image, with and without the five filter passes
        seen = dict(t0=0, neg=0, pos=0, raw_le0=0, unfused=0)
        for st in sorted(cases.CONV_SIZES):
            for ct in sorted(cases.CONV_CALIBS):
                typ, a, b = cases.CONV_CALIBS[ct]
                raw = cases.conv_raw(st, ct)
                for filt in (False, True):
                    ref = run_conv(exe, tmp, raw, typ, a, b, cases.CONV_FX, filt)
                    key = "%s_%s_%s" % (st, ct, "filtered" if filt else "plain")
                    fix[key] = ref
                    if not filt:
                        mine = cases.convert(raw, typ, a, b, cases.CONV_FX)
                        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), (key, "the numpy transcription disagrees with the reference")
                fix["%s_%s_input_crc" % (st, ct)] = crc(raw)
                plain = fix["%s_%s_plain" % (st, ct)]
                if typ == cases.KINECT:
                    t = np.float32(a) - raw.astype(np.float32)
                    seen["t0"] += int((t == 0).sum()); seen["neg"] += int(((t < 0) & (plain == -1)).sum()); seen["pos"] += int((plain > 0).sum())
                    assert (plain[t == 0] == -1).all()
                else:
                    seen["raw_le0"] += int((raw <= 0).sum())
                    seen["unfused"] += int((plain.view(np.uint32) != cases.convert_fused(raw, a, b).view(np.uint32)).sum())
        print("conversion images:", seen)
        assert seen["t0"] > 0 and seen["neg"] > 0 and seen["pos"] > 0, "the Kinect images miss one of the three branches"
        assert seen["raw_le0"] > 0, "the affine images have no raw value <= 0"
        assert seen["unfused"] > 0, "no affine pixel tells a fused multiply-add from a multiply and an add"
        fix["conv_unfused_pixels"] = seen["unfused"]

        # ---- engine runs
        for tag in sorted(cases.RUNS):
            run = cases.make_run(tag)
            ref = run_engine(exe, tmp, run)
            Wd, Hd, Wc, Hc, n = run["Wd"], run["Hd"], run["Wc"], run["Hc"], run["n"]
            typ, a, b = run["calib"]
            p = tag + "_"
            text = ref[("calib_txt", 0)].tobytes().decode()
            assert int(ref[("reread", 0)][0]) == 1, (tag, "calib.txt does not re-read to the same struct")
            assert text == cases.calib_text(Wc, Hc, run["intr_c"], Wd, Hd, run["intr_d"], cases.to_orutils(run["ext"]), typ, a, b), (tag, text)
            texts[tag] = text
            inv = ref[("calib_inv", 0)]
            assert np.array_equal(ref[("calib", 0)].view(np.uint32), cases.to_orutils(run["ext"]).view(np.uint32))
            assert np.array_equal(inv.view(np.uint32), cases.calib_inv(ref[("calib", 0)]).view(np.uint32)), (tag, "calib_inv transcription")
            M = np.stack([ref[("M", f)] for f in range(n)])
            invM = np.stack([ref[("invM", f)] for f in range(n)])
            M_rgb = np.stack([ref[("M_rgb", f)] for f in range(n)])
            assert np.isfinite(M).all() and np.isfinite(invM).all(), (tag, "the reference's poses are not finite")
            for f in range(n):
                assert np.array_equal(M_rgb[f].view(np.uint32), cases.mat_mul(inv, M[f]).view(np.uint32)), (tag, f, "M_rgb transcription")
            get = lambda name, f: ref[(name, f)]
            fix.update({p + "calib_inv": inv, p + "M": M, p + "invM": invM, p + "M_rgb": M_rgb, p + "n_frames": n,
                        p + "ages": np.array([ref[("age", f)][0] for f in range(n)], np.int32),
                        p + "input_crc": np.array([crc(run["rgb"]), crc(run["raw"]), crc(run["c2w"])], np.uint32)})
            for f in range(n):
                if run["mode"] == "given" and not run["filt"]:
                    mine = cases.convert(run["raw"][f], typ, a, b, run["intr_d"][0])
                    assert np.array_equal(mine.view(np.uint32), ref[("depth_f", f)].view(np.uint32)), (tag, f, "conversion transcription")
                assert tuple(ref[("img0_dims", f)]) == (Wc, Hc), (tag, "ORIGINAL_RGB is not at the colour size")
                assert np.array_equal(ref[("img0", f)].reshape(Hc, Wc, 4), run["rgb"][f]), (tag, f, "ORIGINAL_RGB")
                for k, v in frame_digest(get, f, Wd, Hd).items():
                    fix["%s%s@%d" % (p, k, f)] = v
            fix[p + "full_depth"] = ref[("depth_f", n - 1)]
            with_c, without_c = near_surface_counts(ref[("vba_last", n - 1)])
            fix[p + "near_with_colour"], fix[p + "near_without_colour"] = with_c, without_c
            print(tag, "near-surface voxels with / without colour:", with_c, without_c, "ages", fix[p + "ages"].tolist())
            if tag in cases.TWO_CAMERA_RUNS:
                assert with_c > 0 and without_c > 0, (tag, "near-surface voxels with and without colour must both occur", with_c, without_c)
                same = run_engine(exe, tmp, cases.make_run(tag, same_camera=True))
                assert same[("vba_crc", n - 1)][0] != ref[("vba_crc", n - 1)][0], (tag, "the volume equals the one-camera run's")
                assert np.array_equal(same[("hash", n - 1)], ref[("hash", n - 1)]), (tag, "the depth half must not depend on the colour camera")
                fix[p + "same_camera_vba_crc"] = np.uint32(same[("vba_crc", n - 1)][0])
            if typ == cases.KINECT:
                raw0 = run["raw"][0]
                t = np.float32(a) - raw0.astype(np.float32)
                d0 = ref[("depth_f", 0)]
                assert (t == 0).any() and ((t < 0) & (d0 == -1)).any() and (d0 > 0).any(), (tag, "the three branches")
            else:
                assert (run["raw"][0] <= 0).any(), (tag, "no raw value <= 0")
                if not run["filt"] and (a, b) != (0.001, 0.0):
                    assert (ref[("depth_f", 0)].view(np.uint32) != cases.convert_fused(run["raw"][0], a, b).view(np.uint32)).any(), (tag, "fused")
            if run["mode"] == "track":
                moved = np.abs(M[-1] - M[0]).max()
                assert moved > 1e-3, (tag, "the tracked sequence does not move")
                sens = tracked_sensitivity(exe, tmp, run, M)
                print(tag, "the reference's own pose sensitivity per frame:", ["%.2g" % v for v in sens])
                assert sens.max() < TRACK_BOUND / 4, (tag, "the reference does not hold its own tracked poses well inside the bound: "
                                                      "change the step, the pose or the size", sens.tolist())
                fix[p + "reference_sensitivity"] = sens
    for tag, text in texts.items():
        with open(os.path.join(HERE, "rgbd_calib_%s.txt" % tag), "w") as f:
            f.write(text)
    path = os.path.join(HERE, "rgbd_calib.npz")
    np.savez_compressed(path, **fix)
    size = os.path.getsize(path)
    assert size < 500000, "fixture too large: %d bytes" % size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
