"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` -- the headline line only (what --full adds stays
out), `steps` / `ms_per_step` of the timed steps, and DIR holding what the last timed step computed: every MSDA group's forward
output and gradients, the pseudo labels, the assignments and the EMA teacher, float32 / float64, 64 MB at most."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=550)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and "roofline" in d
    assert not {"cpu_baseline", "microbench", "flavours", "supervised_dino_bs2", "warmup_stage"} & set(d)
    names = {os.path.basename(f)[:-4] for f in glob.glob(os.path.join(str(tmp_path), "*.npy"))}
    groups = {k for k in d["breakdown_ms_per_step"] if k.startswith("msda_fwd_")}
    assert groups and groups <= names
    for k in d["breakdown_ms_per_step"]:
        if k.startswith("msda_bwd_"):
            assert {k + "_grad_value", k + "_grad_offsets", k + "_grad_logits"} <= names
    assert {"ema_teacher", "pseudo_boxes", "pseudo_boxes_warped", "pseudo_counts", "hungarian_0_gt_inds"} <= names
    total = 0
    for n in names:
        a = np.load(os.path.join(str(tmp_path), n + ".npy"))
        assert a.dtype in (np.float32, np.float64), n
        assert np.isfinite(a).all(), n
        total += a.nbytes
    assert total <= 64 << 20
