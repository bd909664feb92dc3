"""PIPE.refine_iterations in a session (host/session.cpp): runSession refines between SLAMTrainCams and save.  The fixture is
tests/test_session_gpu.py's (64 x 48, 12 frames, one map update).  In a module of its own: createTsdfEngine hands out THE CLIEngine
of the process, as the reference's CLIEngine::Instance() does, so a session cannot run while tests/test_refine_gpu.py's scene holds
its engine."""
import os
import subprocess
import sys

import pytest
import torch

from tests import digests, synth
from tests import test_session_gpu as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, SEED = S.W, S.H, S.N, S.SEED
NAMES = ("getMeans", "getScales", "getQuats", "getFeaturesDc", "getFeaturesRest", "getOpacities")


def _host():
    return S._host()


def _params(m):
    torch.cuda.synchronize()
    p = m.getGaussianParms()
    return [getattr(p, n)().clone() for n in NAMES]


def _session_yaml(seq, ws, work_mode="train", refine=None):
    text = S._yaml(seq, str(ws), work_mode)
    if refine is not None:
        assert text.count("  log_iter: 1000\n") == 1
        text = text.replace("  log_iter: 1000\n", "  log_iter: 1000\n  refine_iterations: %d\n" % refine)
    return text


def _model_file_tensors(h, path):
    m = h.SLAMGaussianModel()
    m.loadConfig(S.FLAT_MODEL)
    m.loadParamsTensor(str(path))
    return _params(m)


EVAL_CHILD = """
import sys, numpy as np, torch
from tests import digests, synth
from tests import test_session_gpu as S
h = S._host()
seq = synth.make_sequence(S.W, S.H, S.N, step_deg=0.5)
root = h.load_yaml(sys.argv[1])
reader = h.DatasetReader()
reader.loadConfig(root["READER"])
for cam, pose in zip(S._cameras(h, seq), torch.load(sys.argv[2])):
    cam.c2w_slam = pose                     # the training session's estimates, exactly (pose files hold six decimals)
    reader.addTrainCamera(cam)
res = h.run_session(root, reader, "", False, S.SEED)
print("CRCS", res.gaussian_num, " ".join(str(int(digests.crc(r["rgb_u8"].cpu().numpy()))) for r in res.renders))
"""


def test_session_refines_between_the_run_and_the_save(tmp_path):
    h = _host()
    seq = synth.make_sequence(W, H, N, step_deg=0.5)

    def run(tag, refine):
        ws = tmp_path / tag
        cfg = tmp_path / (tag + ".yaml")
        cfg.write_text(_session_yaml(seq, ws, refine=refine))
        root = h.load_yaml(str(cfg))
        reader = S._session_reader(h, seq, root)
        res = h.run_session(root, reader, str(cfg), False, SEED)
        return res, ws, [c.c2w_slam.clone() for c in reader.trainCameras()]

    absent, ws_a, poses_a = run("absent", None)
    zero, ws_z, poses_z = run("zero", 0)
    assert absent.refine_iterations_done == zero.refine_iterations_done == 0 and absent.refine_log == zero.refine_log == []
    ta, tz = _model_file_tensors(h, ws_a / "gs_model" / "model.pt"), _model_file_tensors(h, ws_z / "gs_model" / "model.pt")
    assert all(torch.equal(x, y) for x, y in zip(ta, tz)) and all(torch.equal(x, y) for x, y in zip(poses_a, poses_z))
    for a, z in zip(absent.renders, zero.renders):
        assert torch.equal(a["rgb_u8"], z["rgb_u8"])

    done, ws, poses = run("refined", 20)
    assert done.refine_iterations_done == 20 and done.gaussian_num == absent.gaussian_num
    assert [i for i, _ in done.refine_log] == [19] and done.refine_log[0][1] > 0
    assert all(torch.equal(x, y) for x, y in zip(poses, poses_a))
    tr = _model_file_tensors(h, ws / "gs_model" / "model.pt")
    assert tr[0].shape == ta[0].shape and not any(torch.equal(x, y) for x, y in zip(tr, ta))      # every tensor moved
    assert done.has_image_eval and absent.has_image_eval
    print("session: mean PSNR %.3f dB without, %.3f dB with 20 refinement iterations" % (absent.image_eval.psnr_mean, done.image_eval.psnr_mean))
    # work_mode eval from disk, in a fresh child process, renders the refined model: byte for byte the renders of the training
    # session's eval_after_train (which ran behind the refinement), and not the unrefined model's
    cfg_eval = tmp_path / "refined_eval.yaml"
    cfg_eval.write_text(_session_yaml(seq, ws, "eval", refine=20))
    torch.save(poses, str(tmp_path / "poses.pt"))
    out = subprocess.run([sys.executable, "-c", EVAL_CHILD, str(cfg_eval), str(tmp_path / "poses.pt")], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("CRCS")][0].split()
    assert int(line[1]) == done.gaussian_num and len(line) == 2 + N
    from_disk = [int(x) for x in line[2:]]
    refined = [int(digests.crc(r["rgb_u8"].cpu().numpy())) for r in done.renders]
    unrefined = [int(digests.crc(r["rgb_u8"].cpu().numpy())) for r in absent.renders]
    assert from_disk == refined
    assert all(a != b for a, b in zip(from_disk, unrefined))
