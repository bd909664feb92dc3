"""Loss terms together with an exposure row on the C ABI, host side only: the trailing exposure_terms field of gps_splat_step, the
gps_loss_terms_exposure exports, the slab they share with the other exposure kernels, and the inputs of the GPU cases."""
import ctypes as C

import torch


def test_splat_step_ends_with_exposure_terms_and_it_defaults_to_off():
    from gps_slam_amd._lib import SplatStep
    assert SplatStep._fields_[-1] == ("exposure_terms", C.c_int32)
    assert SplatStep().exposure_terms == 0


def test_the_exposure_exports_are_declared_and_exported():
    from gps_slam_amd import _build, _lib
    assert len(_lib.PROTOTYPES["gps_loss_terms_exposure"][1]) == 23
    assert _lib.PROTOTYPES["gps_loss_terms_exposure"][1][:20] == _lib.PROTOTYPES["gps_loss_terms"][1][:20]   # same order, then row, slab
    _build.build()
    lib = _lib.load_library()
    assert lib.gps_loss_terms_exposure_partials(640, 480) == 300
    assert lib.gps_loss_terms_exposure_partials(37, 50) == 4
    assert lib.gps_loss_terms_exposure_partials(0, 48) == 0
    for w, h in ((640, 480), (1200, 680), (37, 50), (64, 48)):   # one slab serves the rasterizer's tiles, gps_exposure_bwd and this stage
        assert 12 * lib.gps_loss_terms_exposure_partials(w, h) <= lib.gps_exposure_slab_floats(w, h)
    # gps_loss_terms keeps its workspace, which serves both entry points
    assert lib.gps_loss_terms_workspace_floats(640, 480) == 12 * 300 + 9 * 640 * 480


def test_oracle_inputs_of_the_gpu_cases_stay_under_the_exclusion_cap():
    """tests/test_loss_terms_exposure_gpu.py leaves pixels out of its gradient comparison whose L1 sign (|gt - rgb| < 1e-6) or depth
    validity (|depth| < 1e-6) the float64 oracle itself decides within rounding: at most 0.1 % of the pixels for the seeded inputs
    of every case (0 or 1 pixel each)."""
    from tests.test_loss_terms_gpu import SIZES, WEIGHTS, _excluded
    from tests.test_loss_terms_exposure_gpu import SPREADS, ROW, _case_e, _row_table
    from tests.test_exposure_gpu import _table  # noqa: F401  (the construction _row_table repeats on the CPU)
    assert SIZES == [(37, 50), (64, 48)] and SPREADS == [0.02, 0.8] and ROW == 2
    for spread in SPREADS:
        gen = torch.Generator().manual_seed(7)
        want = torch.eye(3, 4).repeat(4, 1, 1) + spread * (torch.rand((4, 3, 4), generator=gen) - 0.5)
        assert torch.equal(_row_table(spread), want)
        for W, H in SIZES:
            for s, d in WEIGHTS:
                ins, table, o = _case_e(W, H, s, d, spread)
                ex = _excluded(o, ins[4], d)
                assert int(ex.sum()) <= 1e-3 * W * H, (W, H, s, d, spread, int(ex.sum()))
                assert bool(o["terms"].isfinite().all()) and bool(o["v_rc"].isfinite().all()) and bool(o["v_ra"].isfinite().all())
                assert bool(o["dE"].isfinite().all()) and float(o["dE"][ROW].abs().max()) > 0
                assert float(o["dE"][torch.arange(4) != ROW].abs().max()) == 0
