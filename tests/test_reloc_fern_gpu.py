"""The device relocaliser (gps_reloc_*, csrc/reloc_fern.hip) through the C ABI against tests/golden/reloc_fern.npz: what the
reference's own FernRelocLib answers on the CPU for the same depth frames and the same fern table (written by
tests/golden/make_reloc_golden.py; the frames are regenerated here from the stored specs, tests/reloc_cases.py).  Everything is
compared for equality: the blurred image and the distances bit for bit, codes, neighbours and harvested ids exactly."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import reloc_cases as cases

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reloc_fern.npz")
SIZES = {"s64x48_": (64, 48), "s72x52_": (72, 52), "q_": (320, 240)}


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(GOLD))


@functools.lru_cache(maxsize=None)
def _depths(prefix):
    g = _gold()
    W, H = SIZES[prefix]
    d = cases.sequence_depths(W, H, [tuple(s) for s in g[prefix + "specs"]], int(g["hole_seed"]))
    return torch.as_tensor(d).cuda().contiguous()


def _make(prefix, capacity=64):
    from gps_slam_amd import relocaliser as RL
    g = _gold()
    W, H = SIZES[prefix]
    r = RL.FernRelocaliser(W, H, depth_range=tuple(float(v) for v in g["depth_range"]), harvesting_threshold=float(g["threshold"]),
                           num_ferns=int(g["num_ferns"]), num_decisions=int(g["num_decisions"]), capacity=capacity, seed=1)
    r.set_ferns(g[prefix + "fern_xy"], g[prefix + "fern_thr"])
    return r


def _enqueue(r, prefix, i, k):
    g = _gold()
    r.process_frame(_depths(prefix)[i], g[prefix + "pose"][i, :16], g[prefix + "pose"][i, 16:], scene_id=0, k=k,
                    harvest=bool(g[prefix + "harvest"][i]))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_frame(res, prefix, i, k, n_before):
    """one frame's result record against the fixture; returns the number of entries after it"""
    g = _gold()
    nn = g[prefix + "nn1"][i:i + 1] if k == 1 else g[prefix + "nn3"][i]
    dist = g[prefix + "dist1"][i:i + 1] if k == 1 else g[prefix + "dist3"][i]
    added = bool(g[prefix + "added"][i])
    assert res["added_id"] == (n_before if added else -1), (prefix, i, k, res)
    assert res["ids"][:k] == [int(v) for v in nn], (prefix, i, k, res, nn)
    assert np.array_equal(_bits(res["distances"][:k]), _bits(dist)), (prefix, i, k, res, dist)
    assert res["ids"][k:] == [-1] * (4 - k) and all(float(d) == 1.0 for d in res["distances"][k:])
    assert res["n_found"] == int((nn >= 0).sum())
    assert res["n_entries"] == n_before + int(added) and res["overflow"] == 0
    return res["n_entries"]


def test_fixture_holds_the_cases_the_tests_name():
    g = _gold()
    tie = int(g["q_tie_frame"])
    assert int(g["q_added"].sum()) >= 3
    assert g["q_dist3"][tie, 0] == g["q_dist3"][tie, 1] and g["q_nn3"][tie, 0] > g["q_nn3"][tie, 1] >= 0   # the later entry first
    assert len(g["q_few_frames"]) > 0 and all((g["q_nn3"][i] == -1).any() for i in g["q_few_frames"])
    assert any(g["q_added"][i] == 0 and g["q_dist1"][i] <= g["threshold"] for i in g["q_near_frames"])
    assert (g["q_harvest"] == 0).any() and (g["q_specs"][:, 0] == 1).any()


@pytest.mark.parametrize("prefix", ["s64x48_", "s72x52_"])
def test_blurred_image_and_code_are_the_references_bit_for_bit(prefix):
    """64 x 48: a 4 x 3 final image; 72 x 52: odd intermediate sizes (9 wide, 13 high), whose last column / row is dropped"""
    g = _gold()
    r = _make(prefix)
    r.enable_debug_outputs()
    W, H = SIZES[prefix]
    assert (r.small_width, r.small_height) == (W // 16, H // 16) == g[prefix + "blurred"].shape[:0:-1] and r.taps == 17
    n = 0
    for i in range(len(g[prefix + "specs"])):
        _enqueue(r, prefix, i, 1)
        res = r.read_result()
        assert np.array_equal(_bits(r.blurred.cpu().numpy()), _bits(g[prefix + "blurred"][i])), (prefix, i)
        assert np.array_equal(r.code.cpu().numpy(), g[prefix + "codes"][i]), (prefix, i)
        n = _check_frame(res, prefix, i, 1, n)
    empty = [i for i, s in enumerate(g[prefix + "specs"]) if s[0] == 1]
    assert empty and not g[prefix + "blurred"][empty[0]].any()   # a frame without any contributor blurs to zeros
    r.close()


@pytest.mark.parametrize("k", [1, 3])
def test_whole_sequence_matches_the_reference(k):
    g = _gold()
    r = _make("q_")
    r.enable_debug_outputs()
    n_frames = len(g["q_specs"])
    tie, few = int(g["q_tie_frame"]), [int(i) for i in g["q_few_frames"]]
    n, results = 0, []
    for i in range(n_frames):
        _enqueue(r, "q_", i, k)
        res = r.read_result()
        results.append(res)
        assert np.array_equal(r.code.cpu().numpy(), g["q_codes"][i]), i
        assert np.array_equal(_bits(r.blurred.cpu().numpy()), _bits(g["q_blurred"][i])), i
        n = _check_frame(res, "q_", i, k, n)
    assert n == int(g["q_added"].sum()) >= 3
    # the exact tie: two stored entries at the same distance from the probe plane, the LATER one first
    t = results[tie]
    if k == 3:
        assert t["distances"][0] == t["distances"][1] and t["ids"][0] > t["ids"][1] >= 0
    assert t["ids"][0] == int(g["q_nn3"][tie, 0]) == int(g["q_nn1"][tie])
    # fewer than k neighbours: id -1 at distance 1.0 behind the ones found
    if k == 3:
        f = results[few[0]]
        assert f["n_found"] < 3 and f["ids"][2] == -1 and float(f["distances"][2]) == 1.0
        assert results[0]["n_found"] == 0 and results[0]["ids"][:3] == [-1, -1, -1]
    # the stored poses are the harvested frames'
    kf = [i for i in range(n_frames) if g["q_added"][i]]
    for idx, i in enumerate(kf):
        M, iM, scene = r.retrieve_pose(idx)
        assert np.array_equal(_bits(M), _bits(g["q_pose"][i, :16])) and np.array_equal(_bits(iM), _bits(g["q_pose"][i, 16:])) and scene == 0
    db = r.export_database()
    assert np.array_equal(db["codes"], g["q_codes"][kf]) and np.array_equal(_bits(db["poses"]), _bits(g["q_pose"][kf]))
    assert r.guards_intact()
    r.close()


def test_full_database_adds_nothing_and_writes_nothing_behind_its_arrays():
    g = _gold()
    r = _make("q_", capacity=2)
    want_kf = int(g["q_added"].sum())
    assert want_kf > 2
    refused = 0
    for i in range(len(g["q_specs"])):
        _enqueue(r, "q_", i, 1)
        res = r.read_result()
        assert res["n_entries"] <= 2 and res["added_id"] in (-1, 0, 1)
        if res["overflow"] > refused:
            assert res["added_id"] == -1 and res["n_entries"] == 2
            refused = res["overflow"]
    assert refused >= want_kf - 2 and r.counts() == (2, refused)
    assert r.guards_intact()
    db = r.export_database()
    kf = [i for i in range(len(g["q_specs"])) if g["q_added"][i]][:2]
    assert np.array_equal(db["codes"], g["q_codes"][kf])   # the two that fitted are the reference's first two, unchanged
    r.close()


def test_export_then_import_into_a_fresh_state_answers_the_same():
    g = _gold()
    n_frames = len(g["q_specs"])
    half = 9   # after the third keyframe
    assert int(g["q_added"][:half].sum()) >= 3 and int(g["q_added"][half:].sum()) >= 1
    a = _make("q_")
    n = 0
    for i in range(half):
        _enqueue(a, "q_", i, 3)
        n = _check_frame(a.read_result(), "q_", i, 3, n)
    db = a.export_database()
    b = _make("q_", capacity=16)
    b.import_database(db["codes"], db["poses"], db["scene_ids"])
    assert b.counts() == (n, 0)
    nb = n
    for i in range(half, n_frames):
        _enqueue(a, "q_", i, 3)
        _enqueue(b, "q_", i, 3)
        ra, rb = a.read_result(), b.read_result()
        assert ra["ids"] == rb["ids"] and np.array_equal(_bits(ra["distances"]), _bits(rb["distances"])) and ra["added_id"] == rb["added_id"]
        nb = _check_frame(rb, "q_", i, 3, nb)
    da, dbb = a.export_database(), b.export_database()
    assert np.array_equal(da["codes"], dbb["codes"]) and np.array_equal(_bits(da["poses"]), _bits(dbb["poses"]))
    assert np.array_equal(da["scene_ids"], dbb["scene_ids"])
    # importing more than fits is refused and leaves the database alone
    from gps_slam_amd._lib import lib
    c = _make("q_", capacity=2)
    big = np.zeros((3, c.num_ferns), np.uint8)
    assert lib.gps_reloc_import(c._h, 3, big.ctypes.data, np.zeros((3, 32), np.float32).ctypes.data,
                                np.zeros(3, np.int32).ctypes.data, None) == -3
    assert c.counts() == (0, 0)
    for s in (a, b, c):
        s.close()


def test_frames_enqueued_back_to_back_give_the_sequential_results():
    """no read-back, no synchronisation between frames: frame 7's neighbours depend on the keyframe frame 6 harvests, and the tie
    probe at the end on every keyframe before it"""
    g = _gold()
    n_frames = len(g["q_specs"])
    assert g["q_added"][6] == 1 and g["q_nn1"][7] == int(g["q_added"][:7].sum()) - 1
    r = _make("q_")
    depths = _depths("q_")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for i in range(8):
            _enqueue(r, "q_", i, 3)
        _check_frame(r.read_result(), "q_", 7, 3, int(g["q_added"][:7].sum()))
        for i in range(8, n_frames):
            _enqueue(r, "q_", i, 3)
        last = n_frames - 1
        _check_frame(r.read_result(), "q_", last, 3, int(g["q_added"][:last].sum()))
        db = r.export_database()
    kf = [i for i in range(n_frames) if g["q_added"][i]]
    assert np.array_equal(db["codes"], g["q_codes"][kf]) and np.array_equal(_bits(db["poses"]), _bits(g["q_pose"][kf]))
    del depths
    r.close()


def test_argument_checks_on_a_live_state():
    from gps_slam_amd._lib import lib
    g = _gold()
    r = _make("q_", capacity=4)
    d = _depths("q_")[0]
    M = np.ascontiguousarray(g["q_pose"][0, :16])
    iM = np.ascontiguousarray(g["q_pose"][0, 16:])
    for k in (0, 5, -1):
        assert lib.gps_reloc_process_frame(r._h, d.data_ptr(), M.ctypes.data, iM.ctypes.data, 0, k, 1, None) == -1
    assert lib.gps_reloc_process_frame(r._h, None, M.ctypes.data, iM.ctypes.data, 0, 1, 1, None) == -1
    assert lib.gps_reloc_process_frame(r._h, d.data_ptr(), None, iM.ctypes.data, 0, 1, 1, None) == -1
    xy, thr = r.ferns()
    assert np.array_equal(xy, g["q_fern_xy"]) and np.array_equal(thr, g["q_fern_thr"])
    assert lib.gps_reloc_set_ferns(r._h, xy.ctypes.data, thr.ctypes.data, len(thr) - 1, None) == -1          # size mismatch
    bad = xy.copy()
    bad[17, 0] = r.small_width                                                                               # outside the 1/16 image
    assert lib.gps_reloc_set_ferns(r._h, bad.ctypes.data, thr.ctypes.data, len(thr), None) == -1
    bad[17] = (0, -1)
    assert lib.gps_reloc_set_ferns(r._h, bad.ctypes.data, thr.ctypes.data, len(thr), None) == -1
    out = np.zeros(16, np.float32)
    assert lib.gps_reloc_retrieve_pose(r._h, 0, out.ctypes.data, out.ctypes.data, None, None) == -1          # empty database
    assert r.counts() == (0, 0)   # none of the refused calls did anything
    r.close()
