"""Inputs of the relocaliser fixture (tests/golden/reloc_fern.npz), regenerated from stored parameters by the generator
(tests/golden/make_reloc_golden.py) and by the tests alike: synthetic depth frames (tests/synth.py) with holes punched by a seeded
generator -- single pixels, whole 16 x 16 blocks (a pixel of the relocaliser's 1/16 image without any contributor) and one empty
frame -- and constant-depth probe planes."""
import numpy as np

from tests import synth

STEP_DEG = 6.0          # orbit step of the sequences: large enough that views a few frames apart become keyframes of their own
HOLE_SHARE = 0.05       # single pixels punched out
N_BLOCK_HOLES = 6       # whole 16 x 16 blocks punched out per frame


def frame_depth(W, H, spec, hole_seed):
    """One float32 depth image [H,W] in metres (0: hole).  spec: (kind, value) with kind 0: the synthetic room seen from orbit
    position `value` (an index into synth.orbit_poses at STEP_DEG), holes punched; 1: the empty frame; 2: a plane at depth `value`
    metres without holes."""
    kind, value = int(spec[0]), float(spec[1])
    if kind == 1:
        return np.zeros((H, W), np.float32)
    if kind == 2:
        return np.full((H, W), np.float32(value), np.float32)
    idx = int(round(value))
    pose = synth.orbit_poses(idx + 1, step_deg=STEP_DEG)[idx]
    fx = 0.5 * W
    _, mm = synth.render_rgbd(pose, fx, fx, (W - 1) / 2.0, (H - 1) / 2.0, W, H)
    depth = mm.astype(np.float32) * np.float32(0.001)
    rng = np.random.default_rng([int(hole_seed), idx, W, H])
    depth[rng.random((H, W)) < HOLE_SHARE] = 0.0
    for _ in range(N_BLOCK_HOLES):
        by, bx = int(rng.integers(0, H // 16)), int(rng.integers(0, W // 16))
        depth[16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = 0.0
    return depth


def sequence_depths(W, H, specs, hole_seed):
    return np.stack([frame_depth(W, H, s, hole_seed) for s in specs])
