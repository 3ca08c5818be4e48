"""bench.py's measured region and its output dump: `--steps K` is the number of timed steps (`ms_per_step` is their mean), and
`--dump-outputs DIR` writes what the last timed step handed out -- float32 / float64 arrays, under the size cap, the same bytes on
every run of the same arguments, from a run whose in-run parity check against the oracle is clean (--full).  A plain run (no --full) times
the same steps and dumps the same bytes, and does nothing else."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--level", "PickupLoc", "--no-pixel", "--envs", "4096", "--steps", "12", "--warmup", "3", "--no-extra-configs", "--no-cpu-baseline",
        "--prewarm-seconds", "0", "--parity-envs", "64"]


def _bench(tmp_path, tag, full=True):
    out = str(tmp_path / tag)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("BBAI_BENCH_LINE", None)
    extra = ["--full", "--full-out", out + ".json"] if full else []
    p = subprocess.run([sys.executable, "bench.py"] + ARGS + ["--dump-outputs", out] + extra,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    return line, {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(out, "*.npy")))}


@pytest.mark.gpu
def test_bench_times_exactly_steps_and_dumps_the_same_outputs_twice(gpu, tmp_path):
    a, da = _bench(tmp_path, "a")
    b, db = _bench(tmp_path, "b")
    for line in (a, b):
        assert line["steps"] == 12 and line["timing"]["timed_steps"] == 12 and line["timing"]["blocks"] == 1
        assert line["ms_per_step"] > 0 and line["parity"]["mismatches_all_ranks"] == 0
    assert set(da) == {"env_ids", "image", "direction", "reward", "reward64", "done"} == set(db)
    assert sum(x.nbytes for x in da.values()) <= 64 << 20
    for k in da:
        assert da[k].dtype in (np.float32, np.float64) and da[k].dtype == db[k].dtype, k
        assert np.array_equal(da[k], db[k]), k
    n = len(da["env_ids"])
    assert da["image"].shape == (n, 7, 7, 3) and n == 1024
    assert da["env_ids"][0] == 0 and da["env_ids"][-1] == 4095 and np.all(np.diff(da["env_ids"]) > 0)
    assert np.array_equal(da["reward"], da["reward64"].astype(np.float32))
    assert set(np.unique(da["done"])) <= {0.0, 1.0} and np.all(da["image"] == np.round(da["image"]))


@pytest.mark.gpu
def test_plain_run_times_and_dumps_what_the_full_run_does(gpu, tmp_path):
    full, dfull = _bench(tmp_path, "full")
    plain, dplain = _bench(tmp_path, "plain", full=False)
    assert full["parity"]["mismatches_all_ranks"] == 0 and full["roofline"]["kernel"] and full["kernel_avg_ms"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus", "scaling"):
        assert plain[k] == full[k], k
    assert plain["timing"]["timed_steps"] == 12 and plain["timing"]["blocks"] == 1 and plain["ms_per_step"] > 0
    assert abs(plain["value"] * plain["ms_per_step"] - 4096e3) < 1e-3 * 4096e3          # env-steps/s = envs / (ms per step)
    assert plain["config"]["resets_in_timed_region"] == full["config"]["resets_in_timed_region"]
    for k in ("roofline", "parity", "cpu_baseline", "configs", "full_record"):
        assert plain[k] is None, k
    assert set(dplain) == set(dfull)
    for k in dfull:
        assert dplain[k].dtype == dfull[k].dtype and np.array_equal(dplain[k], dfull[k]), k
