"""Generates tests/golden/reloc_fern.npz: what the REFERENCE's own FernRelocLib (InfiniTAM/FernRelocLib + ORUtils, read in place
under the reference root, compiled together with tests/golden/reloc_ref_driver.cpp into a temporary directory, run on the CPU)
answers for synthetic depth sequences.  Only data is stored: the fern tables used, per frame the code, hasAddedKeyframe and the
neighbours and distances for k = 1 and k = 3, the blurred images, the poses (M / invM, ORUtils layout), the Gaussian coefficients
and the four text files of the database the 320 x 240 sequence leaves behind.  The depth frames themselves are NOT stored: the
tests regenerate them from the stored frame specs and hole seed (tests/reloc_cases.py).

Run from the repo root:  python tests/golden/make_reloc_golden.py   (needs the built kernel library for the default fern tables:
host code, no GPU)"""
import glob
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from gps_slam_amd import relocaliser as RL  # noqa: E402
from tests import reloc_cases as cases  # noqa: E402

REF = os.path.join(os.environ.get("GPS_REFERENCE_ROOT", "/root/reference"), "InfiniTAM")
NUM_FERNS, NUM_DEC, RANGE, THRESHOLD, HOLE_SEED, FERN_SEED = 500, 4, (0.2, 5.0), 0.2, 20, 7


def build_driver(tmp):
    exe = os.path.join(tmp, "reloc_ref_driver")
    srcs = [os.path.join(HERE, "reloc_ref_driver.cpp")] + sorted(glob.glob(os.path.join(REF, "ORUtils", "*.cpp"))) + \
        [os.path.join(REF, "FernRelocLib", f) for f in ("FernConservatory.cpp", "PoseDatabase.cpp", "RelocDatabase.cpp")]
    # -ffp-contract=off: the plain IEEE sequence (x86-64 has no contraction by default; said anyway, as oracle/ref_build.sh does)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCOMPILE_WITHOUT_CUDA", "-ffp-contract=off", "-w", "-I" + REF, "-o", exe] + srcs)
    return exe


def fern_table(W, H):
    xy, thr = RL.default_ferns(W, H, NUM_FERNS, NUM_DEC, RANGE, FERN_SEED)
    # thresholds that survive the reference's ferns.txt (6 significant digits): the saved database then reloads to this very table
    thr = np.array([np.float32(float("%.6g" % t)) for t in thr], np.float32)
    return xy, thr


def pose_params(spec, i):
    """six SE3 parameters per frame (tx ty tz rx ry rz): any fixed, distinct values do -- the relocaliser only stores them"""
    a = 0.1 * float(spec[1]) + 0.01 * i
    return [0.3 * np.sin(a), -0.2 * np.cos(a), 0.05 * i, 0.2 * a, -0.1 * a, 0.05 * a]


def run_reference(exe, tmp, W, H, specs, harvest, tag):
    d = os.path.join(tmp, tag)
    os.makedirs(os.path.join(d, "init"))
    os.makedirs(os.path.join(d, "saved"))
    xy, thr = fern_table(W, H)
    n = len(specs)
    with open(os.path.join(d, "init", "ferns.txt"), "w") as f:
        for (x, y), t in zip(xy, thr):
            f.write("%d %d %.9g\n" % (x, y, t))
    with open(os.path.join(d, "init", "frames.txt"), "w") as f:
        f.write("%d %d 0\n" % (NUM_FERNS, 1 << NUM_DEC) + "0 \n" * (NUM_FERNS << NUM_DEC))
    with open(os.path.join(d, "init", "poses.txt"), "w") as f:
        f.write("0\n")
    params = np.array([pose_params(s, i) for i, s in enumerate(specs)], np.float32)
    with open(os.path.join(d, "meta.bin"), "wb") as f:
        f.write(struct.pack("<5i3f", W, H, NUM_FERNS, NUM_DEC, n, RANGE[0], RANGE[1], THRESHOLD))
        for i in range(n):
            f.write(struct.pack("<2i6f", int(harvest[i]), 0, *[float(v) for v in params[i]]))
    cases.sequence_depths(W, H, specs, HOLE_SEED).tofile(os.path.join(d, "depth.bin"))
    subprocess.check_call([exe, d])
    w4, h4 = W // 16, H // 16
    rd = lambda name, dt, shape: np.fromfile(os.path.join(d, name), dt).reshape(shape)
    res, dist = rd("res.bin", np.int32, (n, 6)), rd("dist.bin", np.float32, (n, 4))
    assert np.array_equal(res[:, 0], res[:, 2]), "k = 1 and k = 3 must harvest the same frames"
    out = dict(specs=np.array(specs, np.float64), harvest=np.array(harvest, np.int32), fern_xy=xy, fern_thr=thr,
               codes=rd("codes.bin", np.uint8, (n, NUM_FERNS)), blurred=rd("blurred.bin", np.float32, (n, h4, w4)),
               added=res[:, 0].copy(), nn1=res[:, 1].copy(), nn3=res[:, 3:6].copy(), dist1=dist[:, 0].copy(), dist3=dist[:, 1:4].copy(),
               pose=rd("pose.bin", np.float32, (n, 32)), pose_params=params)
    files = {name: np.frombuffer(open(os.path.join(d, "saved", name + ".txt"), "rb").read(), np.uint8)
             for name in ("config", "ferns", "frames", "poses")}
    return out, rd("coeff.bin", np.float32, (17,)), files


# the 320 x 240 sequence: orbit out in steps of two positions, come back over positions in between; positions 10 and 0 are seen
# again exactly (identical frames), some frames are not offered for harvesting, one frame is empty, the last is the tie probe
SEQ_OUT = [(0, p) for p in range(0, 21, 2)]
SEQ_BACK = [(0, 19), (0, 16), (1, 0), (0, 13), (0, 10), (0, 10), (0, 7), (0, 4), (0, 1), (0, 0)]
SEQ_HARVEST_OFF = {12, 15, 16, 19}   # indices into SEQ_OUT + SEQ_BACK


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        fix = {}
        small = [(0, 0), (0, 3), (1, 0), (0, 6), (2, 1.7), (0, 3)]
        for W, H in ((64, 48), (72, 52)):
            out, coeff, _ = run_reference(exe, tmp, W, H, small, [1] * len(small), "s%dx%d" % (W, H))
            assert out["blurred"][2].max() == 0.0 and out["blurred"][0].min() > 0.0
            for k, v in out.items():
                fix["s%dx%d_%s" % (W, H, k)] = v
        # pass 1: the sequence followed by candidate probe planes (never harvested: they leave the database alone); pick a plane
        # whose two nearest stored entries are at exactly the same distance
        seq = SEQ_OUT + SEQ_BACK
        harvest = [0 if i in SEQ_HARVEST_OFF else 1 for i in range(len(seq))]
        probes = [(2, round(0.3 + 0.02 * j, 2)) for j in range(235)]
        out, _, _ = run_reference(exe, tmp, 320, 240, seq + probes, harvest + [0] * len(probes), "pass1")
        n = len(seq)
        ties = [j for j in range(len(probes)) if out["nn3"][n + j, 1] >= 0 and out["dist3"][n + j, 0] == out["dist3"][n + j, 1]]
        assert ties, "no probe plane with an exact tie for the first place"
        probe = probes[ties[0]]
        # pass 2: the sequence as stored
        seq, harvest = seq + [probe], harvest + [0]
        out, coeff, files = run_reference(exe, tmp, 320, 240, seq, harvest, "pass2")
        tie = len(seq) - 1
        few = [i for i in range(len(seq)) if (out["nn3"][i] < 0).any()]
        near = [i for i in range(len(seq)) if out["added"][i] == 0 and out["nn1"][i] >= 0 and out["dist1"][i] <= THRESHOLD]
        # what the tests rely on
        assert int(out["added"].sum()) >= 3, "fewer than 3 harvested keyframes"
        assert near, "no non-harvested frame with a nearest distance <= the threshold"
        assert out["dist3"][tie, 0] == out["dist3"][tie, 1] and out["nn3"][tie, 0] > out["nn3"][tie, 1] >= 0, "no exact tie"
        assert out["nn1"][tie] == out["nn3"][tie, 0]
        assert few and out["nn3"][few[0], 2] == -1 and out["dist3"][few[0], 2] == 1.0, "no frame with fewer than k neighbours"
        assert any(out["added"][i] == 0 and harvest[i] == 1 and out["dist1"][i] == 0.0 for i in range(len(seq))), "no identical frame"
        assert out["blurred"][seq.index((1, 0))].max() == 0.0
        for k, v in out.items():
            fix["q_" + k] = v
        for name, v in files.items():
            fix["q_file_" + name] = v
        fix.update(q_tie_frame=tie, q_few_frames=np.array(few, np.int32), q_near_frames=np.array(near, np.int32))
    fix.update(num_ferns=NUM_FERNS, num_decisions=NUM_DEC, depth_range=np.array(RANGE, np.float32), threshold=np.float32(THRESHOLD),
               hole_seed=HOLE_SEED, fern_seed=FERN_SEED, coeff=coeff)
    path = os.path.join(HERE, "reloc_fern.npz")
    np.savez_compressed(path, **fix)
    print("wrote", path, os.path.getsize(path), "bytes;", int(out["added"].sum()), "keyframes, tie frame", tie, "ids",
          out["nn3"][tie].tolist(), "dist", out["dist3"][tie].tolist(), "; fewer than k:", few, "; near:", near)
    print("added:", out["added"].tolist())
    print("dist1:", [round(float(v), 3) for v in out["dist1"]])


if __name__ == "__main__":
    main()
