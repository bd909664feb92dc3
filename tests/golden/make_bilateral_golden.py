"""Generates tests/golden/bilateral.npz: what the REFERENCE's own view builder and CPU engine (InfiniTAM/ITMLib + ORUtils etc., read
in place under the reference root, compiled together with tests/golden/bilateral_ref_driver.cpp into a temporary directory:
-O2 -std=c++17 -DCOMPILE_WITHOUT_CUDA -ffp-contract=off, no OpenMP) compute with useBilateralFilter = true on the cases of
tests/bilateral_cases.py.  Only data is stored: the full filtered image of every kernel case; for the engine runs a CRC
(tests/digests.crc) of every digest after every frame, the poses, and one frame's filtered depth in full.  The inputs are NOT
stored: the tests regenerate them (bilateral_cases.kernel_depth / sequence).

The exponential.  The driver is linked twice: with its own correctly rounded expf (-DGPS_PIN_EXPF; see the driver) -- THE
reference of this fixture -- and without, the plain-glibc reference.  How many filtered pixels of the kernel cases differ between
the two, and by how many ulp at most, is stored as data (glibc_diff_pixels, glibc_diff_max_ulp).

The generator refuses to write a fixture that does not contain what the tests rely on (see main).

Run from the repo root:  python tests/golden/make_bilateral_golden.py"""
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
from oracle import tsdf_ref as R  # noqa: E402  (the input writer)
from tests import bilateral_cases as cases  # noqa: E402
from tests.digests import crc, frame_digest  # noqa: E402

REF = os.path.join(os.environ.get("GPS_REFERENCE_ROOT", "/root/reference"), "InfiniTAM")
FLAGS = ["-O2", "-std=c++17", "-DCOMPILE_WITHOUT_CUDA", "-ffp-contract=off", "-w", "-I" + REF]


def build_drivers(tmp):
    """-> (pinned, plain): the same objects of the reference, the driver compiled with and without its own expf"""
    pats = ["ITMLib/CPUInstantiations.cpp", "ITMLib/Engines/LowLevel/*Factory.cpp", "ITMLib/Engines/LowLevel/CPU/*.cpp",
            "ITMLib/Engines/ViewBuilding/*Factory.cpp", "ITMLib/Engines/ViewBuilding/CPU/*.cpp",
            "ITMLib/Engines/Visualisation/Interface/*.cpp", "ITMLib/Objects/Camera/*.cpp", "ITMLib/Objects/RenderStates/*.cpp",
            "ITMLib/Trackers/CPU/*.cpp", "ITMLib/Trackers/Interface/*.cpp", "ITMLib/Utils/*.cpp", "ITMLib/Engines/MultiScene/*.cpp",
            "ORUtils/*.cpp", "FernRelocLib/FernConservatory.cpp", "FernRelocLib/PoseDatabase.cpp", "FernRelocLib/RelocDatabase.cpp",
            "MiniSlamGraphLib/*.cpp"]
    drv = os.path.join(HERE, "bilateral_ref_driver.cpp")
    jobs = [(s, os.path.join(tmp, "%03d.o" % i), []) for i, s in enumerate(s for p in pats for s in sorted(glob.glob(os.path.join(REF, p))))]
    lib_objs = [j[1] for j in jobs]
    jobs += [(drv, os.path.join(tmp, "drv_pinned.o"), ["-DGPS_PIN_EXPF"]), (drv, os.path.join(tmp, "drv_plain.o"), [])]
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda j: subprocess.check_call(["g++"] + FLAGS + j[2] + ["-c", j[0], "-o", j[1]]), jobs))
    exes = []
    for name in ("pinned", "plain"):
        exe = os.path.join(tmp, "bilateral_ref_driver_" + name)
        subprocess.check_call(["g++", "-o", exe, os.path.join(tmp, "drv_%s.o" % name)] + lib_objs + ["-lpthread"])
        exes.append(exe)
    return exes


_DT = {"age": np.int32, "counts": np.int32, "visible_ids": np.int32, "vis_type_nz": np.int32, "hash": np.int32, "vba_crc": np.uint32,
       "live": np.uint8, "img1": np.uint8, "code": np.uint8, "ferns_xy": np.int32, "expf_calls": np.int64}


def read_chunks(path, W, H):
    raw = open(path, "rb").read()
    out, off = {}, 0
    while off < len(raw):
        name = raw[off:off + 32].split(b"\0")[0].decode()
        frame, nbytes = struct.unpack_from("<iq", raw, off + 32)
        off += 44
        a = np.frombuffer(raw[off:off + nbytes], _DT.get(name, np.float32)).copy()
        if name in ("live", "img1", "raycast", "icp_points", "icp_normals"):
            a = a.reshape(H, W, 4)
        elif name == "minmax":
            a = a.reshape(H, W, 2)
        elif name == "depth_f":
            a = a.reshape(H, W)
        elif name in ("hash",):
            a = a.reshape(-1, 6)
        elif name in ("vis_type_nz", "ferns_xy"):
            a = a.reshape(-1, 2)
        out[(name, frame)] = a
        off += nbytes
    return out


def run_kernel(exe, tmp, tag):
    W, H = cases.KERNEL_CASES[tag]
    fin, fout = os.path.join(tmp, "kin.bin"), os.path.join(tmp, "kout.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<2i", W, H))
        f.write(cases.kernel_depth(tag).tobytes())
    subprocess.check_call([exe, "kernel", fin, fout])
    ch = read_chunks(fout, W, H)
    return ch[("depth_f", 0)], int(ch[("expf_calls", 0)][0])


def run_engine(exe, tmp, tag):
    W, H, n, _, approx, mode = cases.RUNS[tag]
    seq = cases.sequence(tag)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        R._write_input(f, seq, n, cases.VOXEL, cases.MU, cases.VF_MIN, cases.VF_MAX)
    subprocess.check_call([exe, "engine", fin, fout, "1" if approx else "0", mode], stdout=subprocess.DEVNULL)
    return seq, read_chunks(fout, W, H)


def ulp_distance(a, b):
    """|a - b| in units in the last place, for finite floats of one sign"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def main():
    fix = dict(voxel=np.float32(cases.VOXEL), mu=np.float32(cases.MU), vf_min=np.float32(cases.VF_MIN), vf_max=np.float32(cases.VF_MAX),
               kernel_names=np.array(sorted(cases.KERNEL_CASES)), run_names=np.array(sorted(cases.RUNS)))
    with tempfile.TemporaryDirectory() as tmp:
        pinned, plain = build_drivers(tmp)
        # ---- kernel cases: the full filtered image
        diff_pixels, diff_ulp, filtered = 0, 0, 0
        for tag in sorted(cases.KERNEL_CASES):
            W, H = cases.KERNEL_CASES[tag]
            mm = cases.kernel_depth(tag)
            ref, calls = run_kernel(pinned, tmp, tag)
            glibc, calls_plain = run_kernel(plain, tmp, tag)
            assert calls_plain == 0 and (calls > 0) == (W >= 5 and H >= 5), (tag, "the pinned expf was not the one called", calls, calls_plain)
            st = {}
            mine = cases.filter5(mm, st)
            assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), (tag, "the numpy transcription disagrees with the pinned reference",
                                                                                int((mine.view(np.uint32) != ref.view(np.uint32)).sum()))
            ring = cases.ring_mask(H, W)
            assert (ref[ring] == 0).all() and not np.signbit(ref[ring]).any(), (tag, "the ring is not +0")
            inner = ~ring
            assert ((cases.convert(mm) < 0)[inner] == (ref < 0)[inner]).all() and (ref[ref < 0] == -1).all(), (tag, "holes")
            d = ref.view(np.uint32) != glibc.view(np.uint32)
            diff_pixels += int(d.sum())
            filtered += int((inner & (ref >= 0)).sum())
            if d.any():
                diff_ulp = max(diff_ulp, int(ulp_distance(ref[d], glibc[d]).max()))
            if tag == "k100x52":
                # what the tests rely on
                st1 = {}
                cases.filter_pass(cases.convert(mm), st1)
                assert st1["denormal_weights"] > 0, (tag, "no denormal weight in pass 1", st1)
                assert st1["zero_weights"] > 0, (tag, "no weight that is exactly 0", st1)
                hole = cases.convert(mm) < 0
                near_ring = np.zeros_like(hole)
                near_ring[2, 2:W - 2] = near_ring[H - 3, 2:W - 2] = True
                near_ring[2:H - 2, 2] = near_ring[2:H - 2, W - 3] = True
                assert (hole & near_ring).any(), (tag, "no hole adjacent to the ring")
                assert (inner & (ref >= 0) & (ref != cases.convert(mm))).any(), (tag, "no filtered pixel differs from its input")
                for v in (200, 10000, 1):
                    assert (mm == v).any(), (tag, "value missing", v)
                fix["k_denormal_weights_pass1"], fix["k_zero_weights_pass1"] = st1["denormal_weights"], st1["zero_weights"]
                fix["k_denormal_weights"], fix["k_zero_weights"] = st["denormal_weights"], st["zero_weights"]
            elif tag == "k5x5":
                assert ref[2, 2] > 0 and (ref != 0).sum() == 1
            else:
                assert (ref == 0).all()
            fix[tag + "_W"], fix[tag + "_H"] = W, H
            fix[tag + "_input_crc"] = crc(mm)
            fix[tag + "_filtered"] = ref
            fix[tag + "_expf_calls"] = calls
            print(tag, "expf calls", calls, "stats", st, "pixels differing from plain glibc", int(d.sum()))
        fix["glibc_diff_pixels"], fix["glibc_diff_max_ulp"], fix["glibc_filtered_pixels"] = diff_pixels, diff_ulp, filtered
        print("plain glibc against the pinned expf: %d of %d filtered pixels differ, at most %d ulp" % (diff_pixels, filtered, diff_ulp))

        # ---- engine runs
        for tag in sorted(cases.RUNS):
            W, H, n, step, approx, mode = cases.RUNS[tag]
            seq, ref = run_engine(pinned, tmp, tag)
            assert int(ref[("expf_calls", 0)][0]) > 0
            p = tag + "_"
            get = lambda name, f: ref[(name, f)]
            fix.update({p + "W": W, p + "H": H, p + "n_frames": n, p + "step_deg": np.float64(step), p + "approx": approx,
                        p + "input_crc": np.array([crc(seq["rgb"]), crc(seq["depth"]), crc(seq["c2w"])], np.uint32)})
            M = np.stack([ref[("M", f)] for f in range(n)])
            invM = np.stack([ref[("invM", f)] for f in range(n)])
            assert np.isfinite(M).all() and np.isfinite(invM).all(), (tag, "the reference's poses are not finite")
            fix[p + "M"], fix[p + "invM"] = M, invM
            fix[p + "ages"] = np.array([ref[("age", f)][0] for f in range(n)], np.int32)
            for f in range(n):
                dep = ref[("depth_f", f)]
                ring = cases.ring_mask(H, W)
                assert (dep[ring] == 0).all(), (tag, f, "ring")
                assert np.array_equal(dep.view(np.uint32), cases.filter5(seq["depth"][f].astype(np.int16)).view(np.uint32)), (tag, f, "transcription")
                assert (dep[~ring] < 0).any(), (tag, f, "no hole")
                for k, v in frame_digest(get, f, W, H).items():
                    fix["%s%s@%d" % (p, k, f)] = v
            fix[p + "live_crc"] = np.array([crc(ref[("live", f)]) for f in range(n)], np.uint32)
            fix[p + "img1_crc"] = np.array([crc(ref[("img1", f)]) for f in range(n)], np.uint32)
            if approx:
                assert (fix[p + "ages"] > 0).any(), (tag, "no forward-rendered frame", fix[p + "ages"])
            if tag == "g":
                fix[p + "full_frame"] = n - 1
                fix[p + "full_depth"] = ref[("depth_f", n - 1)]
                fix[p + "full_img1"] = ref[("img1", n - 1)]
                hole0 = cases.convert(seq["depth"][0].astype(np.int16)) < 0
                assert hole0[2:H - 2, 2].any(), (tag, "frame 0 has no hole adjacent to the ring")
            if mode == "reloc":
                fix[p + "ferns_xy"], fix[p + "ferns_thr"] = ref[("ferns_xy", 0)], ref[("ferns_thr", 0)]
                codes = np.stack([ref[("code", f)] for f in range(n)])
                assert len(np.unique(codes)) > 1, (tag, "the fern codes are all one value")
                fix[p + "codes"] = codes
            print(tag, mode, "ages", fix[p + "ages"].tolist())
    path = os.path.join(HERE, "bilateral.npz")
    np.savez_compressed(path, **fix)
    size = os.path.getsize(path)
    assert size < 500000, "fixture too large: %d bytes" % size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
