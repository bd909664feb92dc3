"""Generates tests/golden/get_image.npz: every image ITMBasicEngine::GetImage of the REFERENCE's own ITMLib CPU engine answers
(InfiniTAM/ITMLib + ORUtils etc., read in place under the reference root, compiled together with
tests/golden/get_image_ref_driver.cpp into a temporary directory: -O2 -std=c++17 -DCOMPILE_WITHOUT_CUDA -ffp-contract=off, no
OpenMP) on the given-pose runs of tests/get_image_cases.py: after every frame the six live and original types, then the four
free-camera types at two free poses, always in that order.  Only data is stored: a CRC (tests/digests.crc) of every image -- of
r, g, b alone for the normal types, whose alpha the reference leaves to whatever was rendered before -- the ages of the point
cloud, and the full images of one frame per run.  The frames are NOT stored: the tests regenerate them (get_image_cases.make_run).

The generator refuses to write a fixture that does not exercise what the tests rely on (see check_run).

Run from the repo root:  python tests/golden/make_get_image_golden.py"""
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
from tests import get_image_cases as cases  # noqa: E402
from tests.digests import crc  # noqa: E402

REF = os.path.join(os.environ.get("GPS_REFERENCE_ROOT", "/root/reference"), "InfiniTAM")
FLAGS = ["-O2", "-std=c++17", "-DCOMPILE_WITHOUT_CUDA", "-ffp-contract=off", "-w", "-I" + REF]


def build_driver(tmp):
    pats = ["ITMLib/CPUInstantiations.cpp", "ITMLib/Engines/LowLevel/*Factory.cpp", "ITMLib/Engines/LowLevel/CPU/*.cpp",
            "ITMLib/Engines/ViewBuilding/*Factory.cpp", "ITMLib/Engines/ViewBuilding/CPU/*.cpp",
            "ITMLib/Engines/Visualisation/Interface/*.cpp", "ITMLib/Objects/Camera/*.cpp", "ITMLib/Objects/RenderStates/*.cpp",
            "ITMLib/Trackers/CPU/*.cpp", "ITMLib/Trackers/Interface/*.cpp", "ITMLib/Utils/*.cpp", "ITMLib/Engines/MultiScene/*.cpp",
            "ORUtils/*.cpp", "FernRelocLib/FernConservatory.cpp", "FernRelocLib/PoseDatabase.cpp", "FernRelocLib/RelocDatabase.cpp",
            "MiniSlamGraphLib/*.cpp"]
    srcs = [os.path.join(HERE, "get_image_ref_driver.cpp")] + [s for p in pats for s in sorted(glob.glob(os.path.join(REF, p)))]
    objs = [os.path.join(tmp, "%03d.o" % i) for i in range(len(srcs))]
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda so: subprocess.check_call(["g++"] + FLAGS + ["-c", so[0], "-o", so[1]]), zip(srcs, objs)))
    exe = os.path.join(tmp, "get_image_ref_driver")
    subprocess.check_call(["g++", "-o", exe] + objs + ["-lpthread"])
    return exe


def _dtype(name):
    if name == "age":
        return np.int32
    if name.startswith(("img", "fimg")):
        return np.uint8
    return np.float32


def run_reference(exe, tmp, tag):
    W, H, n, _, approx = cases.RUNS[tag]
    seq = cases.make_run(tag)
    free = [(f, c2w) for f in range(n) for c2w in cases.free_poses(seq["c2w"][f])]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        R._write_input(f, seq, n, cases.VOXEL, cases.MU, cases.VF_MIN, cases.VF_MAX, free_views=free)
    subprocess.check_call([exe, fin, fout, "1" if approx else "0"], stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    out, off = {}, 0
    while off < len(raw):
        name = raw[off:off + 32].split(b"\0")[0].decode()
        frame, nbytes = struct.unpack_from("<iq", raw, off + 32)
        off += 44
        a = np.frombuffer(raw[off:off + nbytes], _dtype(name)).copy()
        if name.startswith(("img", "fimg")):
            a = a.reshape(H, W, 4)
        elif name.startswith(("rays", "frays")):
            a = a.reshape(H, W, 4)
        elif name == "depth_f":
            a = a.reshape(H, W)
        out[(name, frame)] = a
        off += nbytes
    return seq, out


image_crc = cases.image_crc


def check_frame(tag, f, ref):
    """what the tests rely on in a frame stored in full; a run that fails one of these gets another frame, pose or step, never a
    weaker condition.  -> statistics of the image-normal pass"""
    rays = ref[("rays", f)]
    views = [("live", rays, ref[("img5", f)])] + [("free%d" % v, ref[("frays%d" % v, f)], ref[("fimg%d_6" % v, f)]) for v in (0, 1)]
    for name, r, vol in views:
        found = r[..., 3] > 0
        assert found.any() and (~found).any(), (tag, f, name, "found and not-found pixels must both occur", int(found.sum()))
        # a volume type (live: confidence, whose kept pixels have alpha >= 51; free: grey, >= 51 everywhere): found, yet drawn 0
        rejected = found & (vol[..., 3] == 0)
        assert rejected.any(), (tag, f, name, "no found pixel is rejected by !(angle > 0)")
        assert (found & (vol[..., 3] != 0)).any(), (tag, f, name, "no pixel is drawn")
        assert not (~found & (vol != 0).any(-1)).any()
    st = {}
    grey = cases.grey_image_normals(rays, ref[("invM", f)], cases.VOXEL, st)
    assert np.array_equal(grey, ref[("img2", f)]), (tag, f, "the numpy transcription of processPixelGrey_ImageNormals disagrees with the reference")
    assert st["fallback_kept"] > 0, (tag, f, "the +-1 fallback is never taken by a pixel that is kept", st)
    assert st["fallback_rejected"] > 0, (tag, f, "the +-1 fallback is never taken by a pixel that is rejected", st)
    assert st["length_fired"] > 0, (tag, f, "the length_diff test never fires", st)
    dep = ref[("img1", f)]
    assert np.array_equal(dep, cases.depth_to_uchar4(ref[("depth_f", f)])), (tag, f, "the numpy transcription of DepthToUchar4 disagrees")
    for c in range(3):
        assert ((dep[..., c] > 0) & (dep[..., c] < 255)).any(), (tag, f, "colour ramp %d does not occur" % c)
    assert (dep[..., 3] == 0).any() and (dep[..., 3] == 255).any(), (tag, f, "no invalid depth pixel")
    return st


def main():
    fix = dict(voxel=np.float32(cases.VOXEL), mu=np.float32(cases.MU), vf_min=np.float32(cases.VF_MIN), vf_max=np.float32(cases.VF_MAX),
               names=np.array(sorted(cases.RUNS)), types=np.array(cases.TYPES))
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for tag in sorted(cases.RUNS):
            W, H, n, step, approx = cases.RUNS[tag]
            seq, ref = run_reference(exe, tmp, tag)
            ages = np.array([ref[("age", f)][0] for f in range(n)], np.int32)
            p = tag + "_"
            if approx:
                assert (ages > 0).any() and (ages <= 0).any(), (tag, "the approximate run needs frames of both kinds", ages)
            else:
                assert (ages <= 0).all(), (tag, ages)
            fix.update({p + "W": W, p + "H": H, p + "n_frames": n, p + "step_deg": np.float64(step), p + "approx": approx, p + "ages": ages,
                        p + "input_crc": np.array([crc(seq["rgb"]), crc(seq["depth"]), crc(seq["c2w"])], np.uint32)})
            live = np.zeros((n, 6), np.uint32)
            free = np.zeros((n, 2, 4), np.uint32)
            for f in range(n):
                for k in range(6):
                    live[f, k] = image_crc(cases.TYPES[k], ref[("img%d" % k, f)])
                for v in range(2):
                    for k in range(4):
                        free[f, v, k] = image_crc(cases.TYPES[6 + k], ref[("fimg%d_%d" % (v, 6 + k), f)])
            fix[p + "live_crc"], fix[p + "free_crc"] = live, free
            # one frame in full: the last one that passes every condition (the approximate run: a forward frame)
            full, stats, why = None, None, None
            for f in reversed(range(n)):
                if approx and ages[f] <= 0:
                    continue
                try:
                    stats = check_frame(tag, f, ref)
                    full = f
                    break
                except AssertionError as e:
                    why = why or e
            assert full is not None, (tag, "no frame satisfies the conditions; the latest frame's failure:", why)
            fix[p + "full_frame"] = full
            fix[p + "full_live"] = np.stack([ref[("img%d" % k, full)] for k in range(6)])
            if not approx:   # (the free views of the approximate run are those of run "a": the same volume)
                fix[p + "full_free"] = np.stack([np.stack([ref[("fimg%d_%d" % (v, 6 + k), full)] for k in range(4)]) for v in range(2)])
            print(tag, "ages", ages.tolist(), "full frame", full, stats)
    path = os.path.join(HERE, "get_image.npz")
    np.savez_compressed(path, **fix)
    size = os.path.getsize(path)
    assert size < 500000, "fixture too large: %d bytes" % size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
