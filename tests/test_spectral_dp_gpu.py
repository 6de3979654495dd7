"""Data parallelism with spectral normalization (SPEC.md D5s): 2 ranks x batch 2 against 1 rank x batch 4 -- the broadcast of
u / v, the projection inside D's Adam on the communication stream, D's refresh after the wait for that update.  Fresh child
processes sharing GPU 0 over gloo, as tests/test_dp_gpu.py does."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _run(world, tmp):
    port = str(_free_port())
    outs = [os.path.join(tmp, "sn_w%d_r%d.pt" % (world, r)) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_sn_worker.py"), str(r), str(world), port, outs[r]],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    for p in procs:
        try:
            log, _ = p.communicate(timeout=420)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, log.decode()[-3000:]
    return [torch.load(o) for o in outs]


def test_two_ranks_with_spectral_norm_match_one_rank(hip_device, tmp_path):
    single = _run(1, str(tmp_path))[0]
    r0, r1 = _run(2, str(tmp_path))
    assert r0["world"] == r1["world"] == 2 and single["world"] == 1
    # rank 1 was seeded differently: the broadcast gives it rank 0's u / v (= the one-rank run's, same seed)
    for a, b, c in zip(r0["uv0"], r1["uv0"], single["uv0"]):
        assert torch.equal(a, b) and torch.equal(a, c)
    # ranks stay bitwise in lock-step: u, v and masters after two iterations.  (Against the one-rank run only iteration 1 is
    # compared: Adam's first step is sign-like where a gradient is ~0, so from iteration 2 on the two runs' weights -- and the
    # u / v that follow them -- differ by up to a learning rate, which is not a tolerance of the exchange.)
    for k in ("uv1", "uv2"):
        for a, b in zip(r0[k], r1[k]):
            assert torch.equal(a, b), k
    assert torch.equal(r0["wG"], r1["wG"]) and torch.equal(r0["wD"], r1["wD"])
    # iteration 1 against the one-rank run on the full batch: projected gradients (tolerance of test_dp_gpu.py) and u / v, which
    # depend on the weights alone and so are bitwise the same
    for k in ("gG", "gD"):
        err = float((r0[k].double() - single[k].double()).norm() / single[k].double().norm())
        print("SN DP vs single-process %s: rel-L2 %.3e" % (k, err))
        assert err < 1e-5, (k, err)
    for a, c in zip(r0["uv1"], single["uv1"]):
        assert torch.equal(a, c)
    for k, v in single["losses1"].items():
        avg = 0.5 * (r0["losses1"][k] + r1["losses1"][k])
        assert abs(avg - v) <= 1e-4 * max(abs(v), 1e-2), (k, avg, v)
