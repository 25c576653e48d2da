"""bench.py's N > 1 path as the driver will run it, rehearsed on the one GPU of the test box: `python bench.py --gpus 2` becomes a
launcher (no GPU call in it) that starts the two ranks through torch.distributed.run -- the command line the driver uses for
--gpus N -- with `--same-device --backend gloo` (RCCL refuses two ranks on one device).  Asserts the JSON contract of the N > 1
line: whole-job value, the ranks that really ran, and the `comm` object (collective time on the reducer stream, bytes, and the
exposed part the main stream waited for) that makes a scaling number explainable."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_bench_two_ranks_on_one_gpu_through_the_launcher():
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--same-device", "--backend", "gloo", "--steps", "1", "--warmup", "1",
           "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                 # rank 0 alone prints, one line
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["rccl_ranks"]["world_size"] == 2 and j["rccl_ranks"]["backend"] == "gloo"
    assert j["rccl_ranks"]["same_device"] is True and j["scaling"] == "weak" and j["config"]["global_batch"] == 16
    assert j["config"]["losses_finite"] is True and "cpu_baseline" not in j
    assert abs(j["value"] - 16 / (j["ms_per_step"] * 1e-3)) < 1e-2 * j["value"]          # whole-job images/s over both ranks
    c = j["comm"]
    # one D bucket + five G buckets per step: the two flat fp32 gradients, 26.4 + 74.1 MB at S=256
    assert c["collectives"] == 6 and c["bytes"] == 4 * (6605504 + 18525569)
    assert c["d_bucket_ms"] > 0 and c["g_buckets_ms"] > 0 and 0 <= c["exposed_ms"] <= j["ms_per_step"]
    # the per-kernel replay ran on rank 0 under N = 2 as well (its durations are not asserted: under this host-staged rehearsal
    # backend an event bracket also absorbs collective stalls)
    assert j["roofline"]["kernel"] and j["roofline"]["launches"] > 0


def test_bench_plain_run_reports_the_headline_and_dumps_outputs(tmp_path):
    """A plain `bench.py --gpus 1` run times exactly --steps steps and prints the headline alone (the replay, extra configurations,
    north-star block and CPU baseline are --full's); --dump-outputs writes the last timed step's outputs as float32 / float64 .npy."""
    import numpy as np
    out = tmp_path / "dump"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--image-size", "64", "--filter-size", "16",
           "--batch", "2", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["warmup"] == 1 and j["dtype"] == "f32" and j["higher_is_better"] is True
    assert abs(j["value"] - 2 / (j["ms_per_step"] * 1e-3)) < 1e-2 * j["value"]
    for k in ("roofline", "roofline_hbm", "extra", "extra_configs", "north_star_block", "cpu_baseline"):
        assert k not in j, k
    files = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert {"gen_rgb", "cyc_rgb", "grad_g", "grad_d", "weights_g", "weights_d", "loss_total_Generator_loss"} <= set(files)
    assert files["gen_rgb"].shape == (2, 64, 64, 3) and files["cyc_rgb"].shape == (10, 64, 64, 3)
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    for name, a in files.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    assert float(np.abs(files["grad_g"]).max()) > 0
