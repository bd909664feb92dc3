"""The binning case set (tests/binning_cases.py), vetted without a GPU.

Every case goes through the C oracle (orc.isect_tiles / orc.isect_tiles_depth; the model-path scenes through orc.proj_fwd first,
radii clamped to max_gs_radii as the model does) and must really have the property it exists for: the exact intersection count,
the tile-id width, "every pair in one tile", the longest list, the pairs of one tile inside one superblock, the band of every
superblock, the all-zero block, the length classes, the superblock shift and count.  The designed scenes must project to the
designed radii with none of them decided within rounding of an integer.  This is what keeps tests/test_binning_edges_gpu.py
from passing vacuously.
"""
import numpy as np
import pytest

from tests import binning_cases as bc
from tests import scenes


def _oracle(case):
    from oracle import splat_ref as orc
    tw, th = bc.grid(case["W"], case["H"])
    if "depths" in case:
        tpg, ids, flat, offs = orc.isect_tiles_depth(case["m2"], case["radii"], case["depths"], bc.TS, tw, th)
        return tpg, ids, flat, None, None, offs
    return orc.isect_tiles(case["m2"], case["radii"], bc.TS, tw, th)


def test_restated_constants_match_the_sources():
    """the constants this module restates from splat_bin.hpp / splat_bin.hip / splat_bin_sb.hip are the sources'"""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gps_slam_amd", "csrc")
    text = "".join(open(os.path.join(root, f)).read() for f in ("splat_bin.hpp", "splat_bin.hip", "splat_bin_sb.hip"))

    def const(name):
        return re.search(r"constexpr int %s = ([^;]+);" % name, text).group(1).strip()
    assert const("SB_MAX") == str(bc.SB_MAX) and const("SB_MAX_TILES") == str(bc.SB_MAX_TILES)
    assert const("BIN_BLOCK") == str(bc.BIN_BLOCK) and const("WIDE_MAX_BINS") == str(bc.WIDE_MAX_BINS)
    assert const("SORT_THREADS") == "256" and const("SORT_ITEMS") == "8" and bc.SORT_TILE == 256 * 8
    assert const("SCAT_THREADS") == "512" and const("SCAT_ITEMS") == "4" and bc.SCAT_CHUNK == 512 * 4
    for N, (shift, n_sb) in bc._BLOCK_EDGE_SB.items():
        assert (bc.sb_shift_for(N), bc.n_superblocks(N)) == (shift, n_sb), N
    assert [bc.tile_id_bits(t) for t in (1, 2, 3, 4096, 4097, 8192, 16385, 32768, 65536)] == [1, 1, 2, 12, 13, 13, 15, 15, 16]


@pytest.mark.parametrize("name", list(bc.sorted_key_cases()))
def test_sorted_key_case_has_the_property_it_was_built_for(name):
    case = bc.sorted_key_cases()[name]
    tpg, ids, flat, ggs, gst, offs = _oracle(case)
    bc.check_expect(case, case["radii"], tpg, flat, offs)
    tw, th = bc.grid(case["W"], case["H"])
    assert np.array_equal(tpg, bc.tiles_of(case["m2"], case["radii"], tw, th))   # (the module's own box arithmetic)
    assert np.array_equal(ids, np.repeat(np.arange(tw * th), np.diff(np.concatenate([offs.reshape(-1), [flat.shape[0]]]))))


def test_tile_count_cases_cover_both_sort_routes_and_every_uneven_split():
    cases = [c for n, c in bc.sorted_key_cases().items() if n.startswith("tiles_")]
    assert sorted(c["expect"]["bits"] for c in cases) == [1, 1, 12, 13, 15, 16]
    assert sorted(c["expect"]["n_tiles"] for c in cases) == [1, 2, 4096, 4160, 23168, 65536]
    for c in cases:
        N = c["radii"].size
        assert 2000 <= N <= 5000 and 0.25 < (c["radii"] == 0).mean() < 0.35 and 1 <= c["radii"][c["radii"] > 0].min() and c["radii"].max() == 40


def test_isect_count_cases_hit_their_counts():
    got = [bc.sorted_key_cases()["n_isects_%d" % n]["expect"]["n_isects"] for n in bc.ISECT_COUNTS]
    assert got == [0, 1, 2047, 2048, 2049, 4096]
    assert bc.sorted_key_cases()["n_isects_0"]["radii"].size > 0


@pytest.mark.parametrize("name", list(bc.depth_key_cases()))
def test_depth_case_has_the_property_it_was_built_for(name):
    case = bc.depth_key_cases()[name]
    tpg, ids, flat, _, _, offs = _oracle(case)
    bc.check_expect(case, case["radii"], tpg, flat, offs)
    e, d, vis = case["expect"], case["depths"], case["radii"] > 0
    bits = d.view(np.uint32)
    assert (d > 0).all()
    if "n_depths" in e:
        assert np.unique(bits[vis]).size == e["n_depths"]
    if name == "depth_one_byte":
        u = np.unique(bits)
        assert [bin(int(a) ^ 0x40404040).count("1") for a in u] == [1, 1, 1, 1]
        assert sorted(int(a ^ 0x40404040).bit_length() // 8 for a in u) == [0, 1, 2, 3]           # one value per byte position
        assert (np.diff(bits[vis].astype(np.int64)) < 0).any() and (np.diff(bits[vis].astype(np.int64)) > 0).any()   # shuffled
    if e.get("denormals"):
        assert (bits[vis] < 0x00800000).sum() >= 50 and d[vis].min() < 1e-38 and d[vis].max() > 1e29
    # inside a tile the list is ordered by (depth bits, id): the stable depth sort
    n = flat.shape[0]
    if n:
        tile = (ids >> 32).astype(np.int64)
        assert np.array_equal((ids & 0xFFFFFFFF).astype(np.uint32), bits[flat])
        key = np.stack([tile, bits[flat].astype(np.int64), flat.astype(np.int64)], 1)
        order = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))
        assert np.array_equal(order, np.arange(n))


MODEL_NAMES = list(bc.MODEL_BUILDERS)


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_model_case_projects_to_its_design_and_has_its_property(name):
    from oracle import splat_ref as orc
    case = bc.model_case(name)
    W, H, s = case["W"], case["H"], case["scene"]
    tw, th = bc.grid(W, H)
    radii, m2, depths, conics = orc.proj_fwd(s["means"], s["quats"], s["scales"], scenes.pose_inv(s["c2w"]), s["K"], W, H)
    vis = radii > 0
    assert not scenes.radius_is_borderline(conics[vis]).any(), name
    radii = np.minimum(radii, bc.MAX_RADIUS)
    assert np.array_equal(radii, case["design_radii"]), (name, np.nonzero(radii != case["design_radii"])[0][:8])
    tpg, ids, flat, ggs, gst, offs = orc.isect_tiles(m2, radii, bc.TS, tw, th)
    bc.check_expect(case, radii, tpg, flat, offs)
    bc.check_superblock_route(case)


def test_model_cases_are_the_listed_ones():
    assert [bc.model_case("block_edges_%d" % n)["N"] for n in bc.BLOCK_EDGE_N] == list(bc.BLOCK_EDGE_N)
    for n in bc.BLOCK_EDGE_N[1:]:
        r = bc.model_case("block_edges_%d" % n)["design_radii"]
        assert n // 4 - 3 <= (r == 0).sum() <= n // 4 and r[r > 0].min() == bc.MIN_MODEL_RADIUS and r.max() == 40, n
    sizes = {k: (bc.model_case(k)["N"], bc.model_case(k)["W"], bc.model_case(k)["H"]) for k in bc.MODEL_BUILDERS if not k.startswith("block")}
    assert sizes == {"one_tile": (3000, 640, 480), "one_tile_wide": (2048, 640, 480), "chunk_in_one_tile": (131073 + 2000, 96, 64),
                     "chunk_in_one_tile_sb1024": (255 * 1024 + 3000, 96, 64), "alternating_rows": (4096, 640, 480),
                     "one_row": (4096, 4080, 16), "too_wide": (2000, 4096, 16), "grid_4096": (20000, 1024, 1024),
                     "grid_4160": (20000, 1040, 1024), "uniform_lengths": (9600, 640, 480), "long_tile": (9600 + 2100, 640, 480)}
    assert (bc.model_case("one_tile_wide")["design_radii"] == 100).all()
    for k in ("grid_4096", "grid_4160"):
        r = bc.model_case(k)["design_radii"]
        assert r.max() == 100 and r[r > 0].min() == 2
    assert not bc.model_case("too_wide")["expect"]["superblock_path"] and not bc.model_case("grid_4160")["expect"]["superblock_path"]
    assert bc.model_case("grid_4096")["expect"]["superblock_path"] and bc.model_case("one_row")["expect"]["superblock_path"]
