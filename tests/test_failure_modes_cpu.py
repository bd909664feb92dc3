"""The engine's failure modes without a device: decideOnTrackingResult (host/tsdf_engine.hpp) against a transcription of
ITMBasicEngine::ProcessFrame (ITMBasicEngine.tpp:286-366) over every mode, verdict, flag and counter value, and the
TSDF.failure_mode key of createTsdfEngine's node."""
import itertools

import pytest

GOOD, POOR, FAILED = "TRACKING_GOOD", "TRACKING_POOR", "TRACKING_FAILED"
RELOCALISE, IGNORE, STOP = "FAILUREMODE_RELOCALISE", "FAILUREMODE_IGNORE", "FAILUREMODE_STOP_INTEGRATION"


def _host():
    from gps_slam_amd import _build, _build_host, _lib
    _build.build()
    _lib.load_library()
    _build_host.build()
    import gps_slam_amd._host as h
    return h


def _transcription(mode, tracker, added, count, initialised, fusion_active, second_tracker):
    """ITMBasicEngine.tpp:286-366 line by line; the relocaliser and the two TrackCamera calls are their outcomes (added,
    tracker, second_tracker).  -> what happened on the frame."""
    did = dict(relocaliser=False, harvest=False, relocalised=False, fused=False, refreshed=False, raycast=False, old_pose=False)
    result = GOOD                                                     # :286
    if mode == RELOCALISE:                                            # :289-291
        result = tracker
    elif mode == STOP:                                                # :292-297
        result = tracker if tracker != FAILED else POOR
    if mode == RELOCALISE:                                            # :304
        if result == GOOD and count > 0:                              # :306-307
            count -= 1
        did["relocaliser"] = True                                     # :314
        did["harvest"] = result == GOOD and count == 0
        if not added and result == FAILED:                            # :317
            count = 10                                                # :319
            did["relocalised"] = True                                 # :324-329
            result = second_tracker                                   # :331
    did_fusion = False
    if (result == GOOD or not initialised) and fusion_active and count == 0:   # :338
        did["fused"] = did_fusion = True
    if result in (GOOD, POOR):                                        # :349
        if not did_fusion:
            did["refreshed"] = True                                   # :351-352
        did["raycast"] = True                                         # :355
    else:
        did["old_pose"] = True                                        # :366
    return result, count, did


def test_decision_function_is_the_transcription_over_the_whole_table():
    h = _host()
    R, M = h.TrackingResult, h.FailureMode
    n = 0
    for mode, tracker, added, count, init, fusion, second in itertools.product(
            (RELOCALISE, IGNORE, STOP), (GOOD, POOR, FAILED), (False, True), (0, 1, 10), (False, True), (False, True), (GOOD, POOR, FAILED)):
        want_result, want_count, did = _transcription(mode, tracker, added, count, init, fusion, second)
        d = h.decideOnTrackingResult(getattr(M, mode), getattr(R, tracker), added, count, init, fusion)
        case = (mode, tracker, added, count, init, fusion, second)
        assert d.useRelocaliser == did["relocaliser"] and d.harvest == did["harvest"] and d.relocalise == did["relocalised"], case
        if d.relocalise:
            # the first evaluation fuses nothing and leaves the tail to the second TrackCamera's verdict
            assert not d.fuse and not d.refreshAndRaycast and d.relocalisationCount == 10, case
            d = h.decideOnTrackingResult(getattr(M, mode), getattr(R, second), added, d.relocalisationCount, init, fusion, True)
            assert not d.useRelocaliser and not d.harvest and not d.relocalise, case
        assert d.result == getattr(R, want_result), case
        assert d.relocalisationCount == want_count, case
        assert d.fuse == did["fused"], case
        assert d.refreshAndRaycast == did["raycast"], case
        assert (d.refreshAndRaycast and not d.fuse) == did["refreshed"], case
        assert (not d.refreshAndRaycast) == did["old_pose"], case
        n += 1
    assert n == 3 * 3 * 2 * 3 * 2 * 2 * 3


def test_decision_function_named_cases():
    h = _host()
    R, M = h.TrackingResult, h.FailureMode
    f = h.decideOnTrackingResult
    # IGNORE: whatever the tracker says the frame is GOOD and fuses; no relocaliser
    for v in (R.TRACKING_GOOD, R.TRACKING_POOR, R.TRACKING_FAILED):
        d = f(M.FAILUREMODE_IGNORE, v, False, 0, True, True)
        assert d.result == R.TRACKING_GOOD and d.fuse and d.refreshAndRaycast and not d.useRelocaliser and not d.relocalise
    # STOP_INTEGRATION: FAILED becomes POOR -- no fusion once tracking is initialised, no relocalisation, the raycast goes on
    d = f(M.FAILUREMODE_STOP_INTEGRATION, R.TRACKING_FAILED, False, 0, True, True)
    assert d.result == R.TRACKING_POOR and not d.fuse and d.refreshAndRaycast and not d.relocalise and not d.useRelocaliser
    assert f(M.FAILUREMODE_STOP_INTEGRATION, R.TRACKING_FAILED, False, 0, False, True).fuse   # ... before that it still fuses (:338)
    # RELOCALISE: GOOD with a running counter counts down and neither harvests nor fuses until it reaches 0
    d = f(M.FAILUREMODE_RELOCALISE, R.TRACKING_GOOD, False, 10, True, True)
    assert d.relocalisationCount == 9 and not d.harvest and not d.fuse and d.refreshAndRaycast
    d = f(M.FAILUREMODE_RELOCALISE, R.TRACKING_GOOD, False, 1, True, True)
    assert d.relocalisationCount == 0 and d.harvest and d.fuse
    # ... POOR does not count down, FAILED restarts the counter
    assert f(M.FAILUREMODE_RELOCALISE, R.TRACKING_POOR, False, 5, True, True).relocalisationCount == 5
    d = f(M.FAILUREMODE_RELOCALISE, R.TRACKING_FAILED, False, 3, True, True)
    assert d.relocalise and d.relocalisationCount == 10 and not d.harvest
    # ... and a second TrackCamera that fails too leaves the previous raycast and the old pose
    d = f(M.FAILUREMODE_RELOCALISE, R.TRACKING_FAILED, False, 10, True, True, True)
    assert d.result == R.TRACKING_FAILED and not d.fuse and not d.refreshAndRaycast and d.relocalisationCount == 10


def test_failure_mode_key_of_the_tsdf_node():
    h = _host()
    M = h.FailureMode
    base = "voxel_size: 0.01\ntrunc_dist: 0.04\nviewFrustum_min: 0.2\nviewFrustum_max: 10.0\nuse_gt_pose: false\n"
    assert h.tsdfConfigFailureMode(h.parse_yaml(base)) == M.FAILUREMODE_IGNORE          # the absent key: every shipped config
    for name, want in (("ignore", M.FAILUREMODE_IGNORE), ("stop_integration", M.FAILUREMODE_STOP_INTEGRATION),
                       ("relocalise", M.FAILUREMODE_RELOCALISE)):
        assert h.tsdfConfigFailureMode(h.parse_yaml(base + "failure_mode: %s\n" % name)) == want
        assert h.failureModeFromString(name) == want
    for bad in ("relocalize", "RELOCALISE", "stop", "1", ""):
        with pytest.raises(Exception) as e:
            h.tsdfConfigFailureMode(h.parse_yaml(base + "failure_mode: '%s'\n" % bad))
        assert "failure_mode" in str(e.value), (bad, str(e.value))
    with pytest.raises(Exception):   # still a closed key list
        h.tsdfConfigFailureMode(h.parse_yaml(base + "failure_modes: ignore\n"))


def test_engine_defaults_are_the_reference_defaults():
    h = _host()
    for name in ("setFailureMode", "failureMode", "forceTrackerResult", "setPoseQualityThresholds", "relocalisationCount", "lastFrameFused"):
        assert hasattr(h.ITMBasicEngine, name), name
    t = h.PoseQualityThresholds()
    assert t.enabled is False and t.poorScore == 0.0 and t.failedScore == 0.0   # off, and no values shipped
