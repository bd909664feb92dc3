"""The host pieces of the refinement pass (SLAMPipeline::gesTrainCams) that need no device: the means' rate scheduler, updateSH,
gpsh::RandomSelector against its Python twin, and the PIPE.refine_* keys on both hosts."""
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFICE0 = os.path.join(ROOT, "tests", "golden", "configs", "release", "replica", "office0.yaml")


def _host():
    import gps_slam_amd._lib as L
    L.load_library()
    import gps_slam_amd._host as h
    return h


def reference_rates(lr0, max_iterations, steps):
    """the rate after each of `steps` scheduler steps, as the reference computes it: a float64 loop lr *= gamma with
    gamma = pow(0.01, float32(1) / float32(max_iterations)) (raw_gs_model.cpp:673-674, optim_scheduler.hpp)"""
    gamma = math.pow(0.01, float(np.float32(1.0) / np.float32(max_iterations)))
    out, lr = [], float(lr0)
    for _ in range(steps):
        lr = lr * gamma
        out.append(lr)
    return out


@pytest.mark.parametrize("max_iterations", [1, 7, 10000])
def test_scheduler_arithmetic_is_the_references_bit_for_bit(max_iterations):
    h = _host()
    from gps_slam_amd.gs_model import scheduler_gamma
    lr0 = float(np.float32(1.6e-4) * np.float32(3.3))     # means_lr x scene_scale as initOptimizers forms it
    want = reference_rates(lr0, max_iterations, max_iterations)
    sched = h.OptimScheduler(max_iterations)
    assert sched.active and sched.gamma == scheduler_gamma(max_iterations)
    lr_c, lr_p, got_c, got_p = lr0, lr0, [], []
    for _ in range(max_iterations):
        lr_c = sched.step(lr_c)
        lr_p = lr_p * scheduler_gamma(max_iterations)
        got_c.append(lr_c)
        got_p.append(lr_p)
    head = min(20, max_iterations)
    assert got_c[:head] == want[:head] and got_p[:head] == want[:head]          # == on floats: bit for bit (no NaN here)
    assert got_c[-1] == want[-1] and got_p[-1] == want[-1]
    # after max_iterations steps the rate is 0.01 x the start.  The float exponent 1/max_iterations is off by at most 2^-24 relative,
    # which moves 0.01^(1 + d) by at most |ln 0.01| x 6e-8 = 2.8e-7 relative; the product's own rounding is 1e-16 per step
    assert abs(got_c[-1] / (0.01 * lr0) - 1.0) < 1e-6, got_c[-1] / (0.01 * lr0)
    # no scheduler for max_iterations <= 0
    for off in (0, -1):
        s = h.OptimScheduler(off)
        assert not s.active and s.step(lr0) == lr0 and scheduler_gamma(off) is None


@pytest.mark.parametrize("max_sh", [0, 3])
@pytest.mark.parametrize("interval", [0, 1, 2, 1000])
def test_update_sh_is_the_references_expression(interval, max_sh):
    h = _host()
    m = h.SLAMGaussianModel()
    m.maxSH, m.shDegreeInterval = max_sh, interval
    for it in range(-1, 10):
        want = min(max_sh, it // interval) if it >= 0 and interval > 0 else max_sh       # raw_gs_model.h:26-32
        m.updateSH(it)
        assert m.degreesToUse == want, (interval, it, max_sh)
    m.updateSH()
    assert m.degreesToUse == max_sh


@pytest.mark.parametrize("seed", [0, 7, (1 << 40) + 12345])
@pytest.mark.parametrize("size", [1, 2, 5, 17])
def test_random_selector_blocks_are_permutations_and_both_hosts_draw_alike(size, seed):
    h = _host()
    from gps_slam_amd.random_selector import RandomSelector
    items = [100 + 3 * i for i in range(size)]
    cpp, py = h.RandomSelector(items, seed), RandomSelector(items, seed)
    draws_c = [cpp.getNext() for _ in range(3 * size)]
    draws_p = [py.getNext() for _ in range(3 * size)]
    assert draws_c == draws_p
    for value, index in draws_c:
        assert value == items[index]
    for b in range(3):
        assert sorted(i for _, i in draws_c[b * size:(b + 1) * size]) == list(range(size)), b


def test_mt19937_twin_gives_the_standards_ten_thousandth_output():
    from gps_slam_amd.random_selector import MT19937
    g = MT19937()            # default seed 5489: the C++ standard names the 10000th output of std::mt19937
    for _ in range(9999):
        g()
    assert g() == 4123659995


def _pipe_text(extra=""):
    text = open(OFFICE0).read()
    assert text.count("  log_iter: 1000\n") == 1
    return text.replace("  log_iter: 1000\n", "  log_iter: 1000\n" + extra)


def test_refine_keys_parse_and_default_to_off_on_both_hosts():
    h = _host()
    from gps_slam_amd import config
    # absent: off
    p = h.SLAMPipeline(99)
    p.loadConfig(h.parse_yaml(_pipe_text())["PIPE"], "/nonexistent", False)
    s = p.settings()
    assert (s["refine_iterations"], s["refine_cams"], s["refine_seed"], s["refine_cache_mb"]) == (0, "keyframes", 99, 16384)
    assert config.refine_settings(config.parse_yaml(_pipe_text())["PIPE"]) == dict(refine_iterations=0, refine_cams="keyframes", refine_seed=None,
                                                                                   refine_cache_mb=16384)
    # given
    extra = "  refine_iterations: 250\n  refine_cams: all\n  refine_seed: 5\n  refine_cache_mb: 64\n"
    p = h.SLAMPipeline(99)
    p.loadConfig(h.parse_yaml(_pipe_text(extra))["PIPE"], "/nonexistent", False)
    s = p.settings()
    assert (s["refine_iterations"], s["refine_cams"], s["refine_seed"], s["refine_cache_mb"]) == (250, "all", 5, 64)
    assert (p.refine_iterations, p.refine_cams, p.refine_seed, p.refine_cache_mb) == (250, "all", 5, 64)
    assert p.max_iterations == 10000 and p.selected_cam_idx == -1 and p.log_iter == 1000      # the reference's own keys, untouched
    assert config.refine_settings(config.parse_yaml(_pipe_text(extra))["PIPE"]) == dict(refine_iterations=250, refine_cams="all", refine_seed=5,
                                                                                        refine_cache_mb=64)
    flat = config.flatten(config.parse_yaml(_pipe_text(extra))["PIPE"], config.PIPE_KEYS)
    assert flat["refine_iterations"] == 250 and flat["refine_cams"] == "all" and flat["refine_cache_mb"] == 64
    # the flat route reads them as well
    p = h.SLAMPipeline(99)
    p.loadConfig(dict(refine_iterations=3, refine_cams="all"))
    assert p.refine_iterations == 3 and p.refine_cams == "all" and p.refine_seed == 99


def test_bad_refine_cams_raises_with_its_path_on_both_hosts():
    h = _host()
    from gps_slam_amd import config
    extra = "  refine_cams: some\n"
    with pytest.raises(h.ConfigError, match=r"PIPE\.refine_cams.*'keyframes' or 'all'.*some"):
        h.SLAMPipeline(1).loadConfig(h.parse_yaml(_pipe_text(extra))["PIPE"], "/nonexistent", False)
    with pytest.raises(config.ConfigError, match=r"PIPE\.refine_cams.*'keyframes' or 'all'.*some"):
        config.refine_settings(config.parse_yaml(_pipe_text(extra))["PIPE"])
    with pytest.raises(h.ConfigError, match=r"PIPE\.refine_iterations"):
        h.SLAMPipeline(1).loadConfig(h.parse_yaml(_pipe_text("  refine_iterations: -2\n"))["PIPE"], "/nonexistent", False)
