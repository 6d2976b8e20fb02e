"""GPU: the several-rank path of the set losses -- two ranks share cuda:0 over gloo (tests/set_loss_multirank_worker.py):
one all-reduce per loss(), the reduced normalisers are the mean of both ranks' inputs, the finalize takes the reduced
classification normaliser only for warm-up or sync_cls_avg_factor, and FocalLoss does no collective."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_set_loss_two_ranks_gloo():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "280", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "set_loss_multirank_worker.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    reports = {ln[:5]: json.loads(ln[6:]) for ln in r.stdout.splitlines() if ln.startswith("RANK")}
    assert sorted(reports) == ["RANK0", "RANK1"], r.stdout[-2000:]
    for rep in reports.values():
        for k in ("warm0_sync0", "warm0_sync1", "warm1_sync0"):
            c = rep[k]
            assert c["calls"] == 1 and c["reduced_is_mean"] and c["losses_ok"] and c["ranks_differ"], (k, c)
        assert rep["loss_set_calls"] == 1, rep
        assert rep["focal_calls"] == 0, rep
