"""Densification without a device: the argument checks of gps_densify_accumulate / _plan / _apply (every refusal comes before a
launch, so it needs no GPU), the two statements of the oracle against each other over every case (tests/densify_cases.py), the
MODEL keys of the shipped configuration files, and the SLAM configuration's refusal of enable_densify."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import densify_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = os.path.join(ROOT, "tests", "golden", "configs")
FIXTURES = sorted(glob.glob(os.path.join(GOOD, "**", "*.yaml"), recursive=True))
ERR_ARG, ERR_CAPACITY = -1, -3


def _lib():
    from gps_slam_amd import _lib
    return _lib.load_library()


def _host():
    _lib()
    import gps_slam_amd._host as h
    return h


@pytest.fixture(scope="module")
def cases():
    return dc.all_cases()


def test_case_set_covers_what_it_names(cases):
    assert len(cases) == 2 * 19 and len({c.name for c in cases}) == len(cases)
    by = {c.name: c for c in cases}
    for K in (1, 16):
        t = "k%d_" % K
        for lab, counts in (("plain", [1, 0, 0, 0, 1]), ("clone", [2, 0, 0, 1, 1]), ("split", [2, 1, 1, 0, 0]), ("low", [0, 0, 0, 0, 0])):
            assert dc.oracle_index(by[t + "one_" + lab]).counts.tolist() == counts
        e = dc.oracle_index(by[t + "all_split"])
        assert e.counts.tolist() == [82, 41, 41, 0, 0]
        assert dc.oracle_index(by[t + "all_pruned"]).M == 0
        e = dc.oracle_index(by[t + "no_split"]); assert e.counts[1] == 0 and e.counts[3] > 0
        e = dc.oracle_index(by[t + "no_clone"]); assert e.counts[3] == 0 and e.counts[1] > 0
        e = dc.oracle_index(by[t + "no_low"]); assert e.counts[4] + e.counts[1] == by[t + "no_low"].N   # nothing pruned but the split parents
        e = dc.oracle_index(by[t + "no_plain"]); assert e.counts[4] == e.counts[3] > 0                   # every kept row is a clone parent
        e = dc.oracle_index(by[t + "split_low"]); assert 0 < e.counts[2] < e.counts[1]
        c = by[t + "clone_low"]; e = dc.oracle_index(c)
        assert e.counts[3] == c.labels.count("clone") and c.labels.count("clone_low") > 0
        off, on = dc.oracle_index(by[t + "scale_prune_off"]), dc.oracle_index(by[t + "scale_prune_on"])
        assert by[t + "scale_prune_off"].labels == by[t + "scale_prune_on"].labels
        assert off.counts[4] > on.counts[4] and off.counts[2] > on.counts[2] > 0 and off.counts[1] == on.counts[1]
        c = by[t + "vis0"]; e = dc.oracle_index(c)
        assert e.counts[3] == c.labels.count("vis0") > 0 and c.labels.count("vis0_zero") > 0
        for n in (255, 256, 257, 513):
            c = by[t + "n%d" % n]
            assert c.N == n and set(c.labels) == set(dc.CLASSES) and c.K == K


def test_no_decision_is_near_its_threshold(cases):
    for c in cases:
        assert dc.check_margins(c), c
    # the check itself: a row moved onto a threshold fails it
    c = dc.make_case("probe", 1, ["plain", "split"], seed=7)
    c.grad_sum[0] = np.float32(dc.GRAD_THRES * (1 + 0.5 * dc.MARGIN)) * c.vis_count[0]
    assert not dc.check_margins(c)
    c = dc.make_case("probe", 1, ["plain", "split"], seed=7)
    c.log_scales[1] = np.float32(np.log(dc.PRUNE_SCALE * dc.SIZE_FAC * (1 - 0.5 * dc.MARGIN)))   # the child's scale on prune_scale
    assert not dc.check_margins(c)


def test_both_statements_of_the_oracle_agree(cases):
    for c in cases:
        a, b = dc.oracle_index(c), dc.oracle_cat(c)
        assert a.counts.tolist() == b.counts.tolist(), c
        assert np.array_equal(a.src, b.src) and np.array_equal(a.kind, b.kind) and np.array_equal(a.sample, b.sample), c
        for k, (x, y) in enumerate(zip(a.params, b.params)):
            assert x.shape == y.shape == (a.M,) + c.params[k].shape[1:], (c, k)
            copied = np.ones(a.M, bool) if k > 1 else a.kind != 1
            assert np.array_equal(x[copied], y[copied]), (c, k)                      # the same source rows, bit for bit
            np.testing.assert_allclose(x[~copied], y[~copied], rtol=1e-13, atol=1e-15, err_msg=repr((c, k)))
        # the header's layout, spelled out once more: three groups, children sample-major, everything ascending inside
        M, n_split, n_ss, n_ds, n_keep = a.counts.tolist()
        assert a.kind.tolist() == [0] * n_keep + [1] * (2 * n_ss) + [2] * n_ds
        for lo, hi in ((0, n_keep), (n_keep, n_keep + n_ss), (n_keep + n_ss, n_keep + 2 * n_ss), (n_keep + 2 * n_ss, M)):
            assert np.all(np.diff(a.src[lo:hi]) > 0)
        s0, s1 = slice(n_keep, n_keep + n_ss), slice(n_keep + n_ss, n_keep + 2 * n_ss)
        assert np.array_equal(a.src[s0], a.src[s1]) and np.array_equal(a.sample[s0] + n_split, a.sample[s1])
        assert np.all(a.sample[s0] < n_split)


def _plan_args(N, ptr=0x1000, cap=None, ws_bytes=None, lib=None):
    cap = 2 * N if cap is None else cap
    ws_bytes = lib.gps_densify_plan_workspace_bytes(N) if ws_bytes is None else ws_bytes
    return [N, ptr, ptr, ptr, ptr, 0.1, 0.1, 0.1, 0.1, ptr, ptr, cap, ptr, None, ptr, ws_bytes, None]


def test_bad_arguments_are_refused_before_any_launch():
    """the pointers are not memory: a call that got past its checks would fault (and without a device, fail to launch)"""
    lib = _lib()
    p = 0x1000
    # accumulate
    assert lib.gps_densify_accumulate(-1, p, p, 64, 48, p, p, None) == ERR_ARG
    assert lib.gps_densify_accumulate(5, p, p, 0, 48, p, p, None) == ERR_ARG
    for hole in range(4):
        a = [5, p, p, 64, 48, p, p, None]
        a[(1, 2, 5, 6)[hole]] = None
        assert lib.gps_densify_accumulate(*a) == ERR_ARG
    assert lib.gps_densify_accumulate(5, p + 4, p, 64, 48, p, p, None) == ERR_ARG      # float2 loads
    assert lib.gps_densify_accumulate(0, None, None, 64, 48, None, None, None) == 0
    # plan
    assert lib.gps_densify_plan_workspace_bytes(-1) < 0
    assert lib.gps_densify_plan_workspace_bytes(0) >= 0
    assert lib.gps_densify_plan_workspace_bytes(257) >= 257 + 4 * 4 * 2
    a = _plan_args(-1, lib=lib); a[15] = 1 << 20
    assert lib.gps_densify_plan(*a) == ERR_ARG
    for hole in (1, 2, 3, 4, 9, 10, 12, 14):
        a = _plan_args(300, lib=lib)
        a[hole] = None
        assert lib.gps_densify_plan(*a) == ERR_ARG, hole
    assert lib.gps_densify_plan(*_plan_args(300, cap=599, lib=lib)) == ERR_CAPACITY
    assert lib.gps_densify_plan(*_plan_args(300, ws_bytes=lib.gps_densify_plan_workspace_bytes(300) - 1, lib=lib)) == ERR_CAPACITY
    host = (C.c_int32 * 5)(7, 7, 7, 7, 7)
    a = _plan_args(0, lib=lib)
    a[1:5] = [None] * 4; a[9] = a[10] = None; a[13] = C.addressof(host)
    assert lib.gps_densify_plan(*a) == 0 and list(host) == [0] * 5
    # apply
    six = (C.c_void_p * 6)(*[p + 0x100 * k for k in range(6)])
    alt = (C.c_void_p * 6)(*[p + 0x100 * k + 0x10000 for k in range(6)])
    good = dict(N=10, K=16, M=9, n_split=2, n_ss=1, n_ds=2, n_keep=5)

    def apply(samples=p, src=six, dst=alt, sm=six, dm=alt, sv=six, dv=alt, table=p, **kw):
        g = dict(good, **kw)
        return lib.gps_densify_apply(g["N"], g["K"], g["M"], g["n_split"], g["n_ss"], g["n_ds"], g["n_keep"], table, table, samples,
                                     src, dst, sm, dm, sv, dv, None)

    assert apply(N=-1) == ERR_ARG and apply(K=0) == ERR_ARG and apply(M=-1) == ERR_ARG
    assert apply(M=8) == ERR_ARG                         # M != n_keep + 2 n_ss + n_ds
    assert apply(n_ss=3, M=13) == ERR_ARG                # more surviving parents than parents
    assert apply(n_keep=9, M=13) == ERR_ARG              # kept rows + split parents exceed N
    assert apply(n_ds=6, M=13) == ERR_ARG                # more clones than kept rows
    assert apply(samples=None) == ERR_ARG                # samples == NULL with n_split > 0
    assert apply(samples=None, n_ss=0, M=7) == ERR_ARG   # ... even when no child survives: the draw is per split parent
    assert apply(table=None) == ERR_ARG
    assert apply(src=None) == ERR_ARG and apply(dst=None) == ERR_ARG
    assert apply(dst=six) == ERR_ARG                     # in place
    assert apply(dm=None) == ERR_ARG and apply(sv=None) == ERR_ARG      # the moments: all four arrays or none
    assert apply(dm=six) == ERR_ARG
    holed = (C.c_void_p * 6)(*[None if k == 2 else p + 0x100 * k for k in range(6)])
    assert apply(src=holed) == ERR_ARG
    norest = (C.c_void_p * 6)(*[None if k == 4 else p + 0x100 * k for k in range(6)])
    assert apply(src=norest) == ERR_ARG                  # K = 16 has a featuresRest tensor
    # nothing to write: 0 without a launch, also with every row pruned
    assert apply(N=0, M=0, n_split=0, n_ss=0, n_ds=0, n_keep=0, samples=None) == 0
    assert apply(N=10, M=0, n_split=3, n_ss=0, n_ds=0, n_keep=0) == 0


def test_header_and_ctypes_agree_on_the_block_size():
    txt = open(os.path.join(ROOT, "include", "gps_slam_hip.h")).read()
    assert "#define GPS_DENSIFY_PLAN_BLOCK %d\n" % dc.BLOCK in txt and "#define GPS_DENSIFY_COUNTS 5\n" in txt


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.relpath(p, GOOD))
def test_model_keys_are_read_from_the_shipped_files(path):
    h = _host()
    M = h.load_yaml(path)["MODEL"]
    flat = h.SLAMGaussianModel().flattenConfig(M)
    for key in ("densify_start_iter", "densify_end_iter", "densify_interval", "reset_opacity_interval"):
        assert flat[key] == M[key].as_int() > 0, key
    for key in ("densify_grad_thres", "densify_large_thres", "prune_opacity_thres"):
        assert flat[key] == float(np.float32(M[key].as_double())) > 0, key
    assert "split_screen_size" in M.keys() and "split_screen_size" not in flat        # read by the reference, used nowhere
    assert "means_lr_final" not in flat


def test_slam_configuration_still_refuses_enable_densify():
    h = _host()
    root = h.load_yaml(os.path.join(GOOD, "release", "replica", "office0.yaml"))
    text = open(os.path.join(GOOD, "release", "replica", "office0.yaml")).read()
    assert text.count("  enable_densify: false\n") == 1
    edited = h.parse_yaml(text.replace("  enable_densify: false\n", "  enable_densify: true\n"), "edited.yaml")
    h.SLAMPipeline(1).loadConfig(root["PIPE"], "x", False)                              # the shipped file loads
    with pytest.raises(h.ConfigError, match=r"PIPE\.enable_densify"):
        h.SLAMPipeline(1).loadConfig(edited["PIPE"], "x", False)
    assert not os.path.exists("x")
