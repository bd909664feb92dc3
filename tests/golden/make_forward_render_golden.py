"""Generates tests/golden/forward_render.npz: what the REFERENCE's own ITMLib CPU engine (InfiniTAM/ITMLib + ORUtils etc., read in
place under the reference root, compiled together with tests/golden/forward_render_ref_driver.cpp into a temporary directory
with the flags of oracle/ref_build.sh: no OpenMP, -ffp-contract=off) does with ITMLibSettings::useApproximateRaycast = true on
synthetic sequences with given poses, and on a third one with the tracker on (TRACKED).  Only data is stored: per frame the age of the
point cloud, the branch Prepare took, the far test's squared distance, the missing count, the digests of tests/digests.py, CRCs
of the forward projection (before and after the hole fill) and of the live re-render; for one forward frame per sequence the
sorted missing list and the full forward projections.  The frames are NOT stored: the tests regenerate them from the stored
parameters (tests/synth.make_sequence).

The generator refuses to write a fixture whose sequences do not exercise what the tests rely on (see check_sequence).

Run from the repo root:  python tests/golden/make_forward_render_golden.py"""
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
from oracle import tsdf_ref as R  # noqa: E402  (the input writer and the chunk decoder of the engine dump)
from tests import synth  # noqa: E402
from tests.digests import crc, frame_digest  # noqa: E402

REF = os.path.join(os.environ.get("GPS_REFERENCE_ROOT", "/root/reference"), "InfiniTAM")
VOXEL, MU, VF_MIN, VF_MAX = 0.02, 0.08, 0.2, 10.0
# given-pose sequences: name -> (W, H, frames, step_deg)
SEQUENCES = {"a": (100, 75, 12, 0.2), "b": (64, 48, 8, 0.8)}
# the tracked run.  Not 100 x 75: below 160 x 120 the reference's own tracker answers NaN poses from the second frame on (its
# coarsest pyramid level degenerates; 64 x 48, 100 x 75 and 128 x 96 tried, at 20, 10 and 5 mm voxels) -- the smallest size at
# which it tracks, ragged against the 16-pixel workgroups in y
TRACKED = ("t", 160, 120, 12, 0.2)
FLAGS = ["-O2", "-std=c++17", "-DCOMPILE_WITHOUT_CUDA", "-ffp-contract=off", "-w", "-I" + REF]


def build_driver(tmp):
    pats = ["ITMLib/CPUInstantiations.cpp", "ITMLib/Engines/LowLevel/*Factory.cpp", "ITMLib/Engines/LowLevel/CPU/*.cpp",
            "ITMLib/Engines/ViewBuilding/*Factory.cpp", "ITMLib/Engines/ViewBuilding/CPU/*.cpp",
            "ITMLib/Engines/Visualisation/Interface/*.cpp", "ITMLib/Objects/Camera/*.cpp", "ITMLib/Objects/RenderStates/*.cpp",
            "ITMLib/Trackers/CPU/*.cpp", "ITMLib/Trackers/Interface/*.cpp", "ITMLib/Utils/*.cpp", "ITMLib/Engines/MultiScene/*.cpp",
            "ORUtils/*.cpp", "FernRelocLib/FernConservatory.cpp", "FernRelocLib/PoseDatabase.cpp", "FernRelocLib/RelocDatabase.cpp",
            "MiniSlamGraphLib/*.cpp"]
    srcs = [os.path.join(HERE, "forward_render_ref_driver.cpp")] + [s for p in pats for s in sorted(glob.glob(os.path.join(REF, p)))]
    objs = [os.path.join(tmp, "%03d.o" % i) for i in range(len(srcs))]
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda so: subprocess.check_call(["g++"] + FLAGS + ["-c", so[0], "-o", so[1]]), zip(srcs, objs)))
    exe = os.path.join(tmp, "forward_render_ref_driver")
    subprocess.check_call(["g++", "-o", exe] + objs + ["-lpthread"])
    return exe


_EXTRA = {"prep": np.int32, "diff": np.float32, "pc_M": np.float32, "live": np.uint8, "fwd": np.float32, "fwd_pre": np.float32,
          "missing": np.int32}


def run_reference(exe, tmp, seq, n, track):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        R._write_input(f, seq, n, VOXEL, MU, VF_MIN, VF_MAX)
    subprocess.check_call([exe, fin, fout] + (["track"] if track else []), stdout=subprocess.DEVNULL)
    raw = open(fout, "rb").read()
    std, extra, off = {}, {}, 0
    while off < len(raw):
        name = raw[off:off + 32].split(b"\0")[0].decode()
        frame, nbytes = struct.unpack_from("<iq", raw, off + 32)
        off += 44
        if name in _EXTRA:
            extra[(name, frame)] = np.frombuffer(raw[off:off + nbytes], _EXTRA[name]).copy()
        else:
            std[(name, frame)] = raw[off:off + nbytes]
        off += nbytes
    out = R.decode(std, seq["W"], seq["H"])
    out.update(extra)
    return out


def check_sequence(tag, ref, n, P):
    """what the tests rely on; a sequence that fails one of these gets another step_deg or frame count, never a weaker condition"""
    prep = np.stack([ref[("prep", f)] for f in range(n)])
    diff = np.array([ref[("diff", f)][0] for f in range(n)])
    assert not ((diff >= 0.0004) & (diff <= 0.0006)).any(), (tag, "a far-test distance inside [0.0004, 0.0006]", diff)
    fwd = prep[:, 2] == 1
    assert fwd.any(), (tag, "no forward frame")
    assert ((prep[fwd, 3] > 0) & (prep[fwd, 3] < 0.25 * P)).all(), (tag, "missing share outside (0, 25 %)", prep[:, 3])
    age_rule = (prep[:, 0] > 5).any()
    dist_rule = ((prep[:, 0] >= 0) & (prep[:, 0] <= 5) & (diff > 0.0005)).any()
    return prep, diff, age_rule, dist_rule, bool((prep[fwd, 4] > 0).any())


def main():
    fix = dict(voxel=np.float32(VOXEL), mu=np.float32(MU), vf_min=np.float32(VF_MIN), vf_max=np.float32(VF_MAX),
               names=np.array(sorted(SEQUENCES)))
    fired = {"age": False, "distance": False, "multi": False}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for tag, (W, H, n, step) in sorted(SEQUENCES.items()):
            seq = synth.make_sequence(W, H, n, step_deg=step)
            ref = run_reference(exe, tmp, seq, n, False)
            prep, diff, age_rule, dist_rule, multi = check_sequence(tag, ref, n, W * H)
            fired["age"] |= age_rule; fired["distance"] |= dist_rule; fired["multi"] |= multi
            p = tag + "_"
            fix.update({p + "W": W, p + "H": H, p + "n_frames": n, p + "step_deg": np.float64(step), p + "prep": prep, p + "diff": diff,
                        p + "M": np.stack([ref[("M", f)] for f in range(n)]), p + "invM": np.stack([ref[("invM", f)] for f in range(n)]),
                        p + "pc_M": np.stack([ref[("pc_M", f)] for f in range(n)]),
                        p + "live_crc": np.array([crc(ref[("live", f)]) for f in range(n)], np.uint32),
                        p + "input_crc": np.array([crc(seq["rgb"]), crc(seq["depth"]), crc(seq["c2w"])], np.uint32)})
            get = lambda k, f: ref[(k, f)]
            for f in range(n):
                for k, v in frame_digest(get, f, W, H).items():
                    fix["%s%s@%d" % (p, k, f)] = v
            fwd_frames = [f for f in range(n) if prep[f, 2] == 1]
            fix[p + "fwd_crc"] = np.array([crc(ref[("fwd", f)]) if f in fwd_frames else 0 for f in range(n)], np.uint32)
            fix[p + "fwd_pre_crc"] = np.array([crc(ref[("fwd_pre", f)]) if f in fwd_frames else 0 for f in range(n)], np.uint32)
            fix[p + "missing_crc"] = np.array([crc(np.sort(ref[("missing", f)])) if f in fwd_frames else 0 for f in range(n)], np.uint32)
            # one forward frame in full: the one with the most multiply-hit targets (the winner rule shows there)
            full = max(fwd_frames, key=lambda f: (prep[f, 4], -f))
            fix[p + "full_frame"] = full
            fix[p + "full_missing"] = np.sort(ref[("missing", full)])
            fix[p + "full_fwd"] = ref[("fwd", full)].reshape(H, W, 4)
            fix[p + "full_fwd_pre"] = ref[("fwd_pre", full)].reshape(H, W, 4)
            print(tag, "ages", prep[:, 1].tolist(), "branch", prep[:, 2].tolist(), "missing", prep[:, 3].tolist(), "multi", prep[:, 4].tolist())
            print(tag, "diff", ["%.2e" % d for d in diff])
        tag, W, H, n, step = TRACKED
        seq = synth.make_sequence(W, H, n, step_deg=step)
        trk = run_reference(exe, tmp, seq, n, True)
        tprep, tdiff, _, _, _ = check_sequence(tag, trk, n, W * H)
        M = np.stack([trk[("M", f)] for f in range(n)])
        assert np.isfinite(M).all(), "the reference's tracker lost the pose"
        p = tag + "_"
        fix.update({p + "W": W, p + "H": H, p + "n_frames": n, p + "step_deg": np.float64(step), p + "prep": tprep, p + "diff": tdiff,
                    p + "M": M, p + "invM": np.stack([trk[("invM", f)] for f in range(n)]),
                    p + "input_crc": np.array([crc(seq["rgb"]), crc(seq["depth"]), crc(seq["c2w"])], np.uint32)})
        print(tag, "tracked branch", tprep[:, 2].tolist(), "missing", tprep[:, 3].tolist(), "diff", ["%.2e" % d for d in tdiff])
    assert fired["age"], "the age rule (point cloud older than 5 frames) never fired"
    assert fired["distance"], "the distance rule never fired"
    assert fired["multi"], "no forward frame has a target pixel with more than one source: nothing pins the winner rule"
    path = os.path.join(HERE, "forward_render.npz")
    np.savez_compressed(path, **fix)
    size = os.path.getsize(path)
    assert size < 500000, "fixture too large: %d bytes" % size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
