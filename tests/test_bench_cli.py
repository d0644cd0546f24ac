"""bench.py's plain run (set up, warm up, timed steps, result line) and
`--dump-outputs`, on CPU with a small shard."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cache_check", "rccl_placement", "gang_admit_open_loop", "nodes1024", "service_mode", "scenarios",
             "gpu_probes")


def run_bench(*extra: str) -> dict:
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--nodes", "8",
           "--waves-per-step", "2", "--cpus", "none", *extra]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return d, run_bench("--dump-outputs", str(d))


def test_plain_run_prints_the_headline_line_only(dumped):
    _, line = dumped
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype"):
        assert k in line
    assert line["steps"] == 3 and line["value"] > 0 and line["unit"] == "pods/s"
    c = line["config"]
    # --steps sets the timed steps: ms_per_step is the timed region over them.
    assert abs(line["ms_per_step"] - c["timed_region_s"] * 1000 / 3) <= 0.5
    assert sum(v["n"] for v in c["gang_admit"].values()) > 0
    assert not [k for k in FULL_ONLY if k in c], list(c)


def test_dump_outputs_holds_the_last_step(dumped, tmp_path):
    d, line = dumped
    arrays = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert set(arrays) == {"gang_wave", "gang_size", "gang_nodes", "gang_hostable", "wave_pods"}
    assert all(a.dtype == np.float64 for a in arrays.values())
    n = len(arrays["gang_size"])
    assert n > 0 and all(len(arrays[k]) == n for k in ("gang_wave", "gang_nodes", "gang_hostable"))
    # One step = --waves-per-step waves; every wave of it is there, in order.
    assert len(arrays["wave_pods"]) == 2 and arrays["wave_pods"].sum() == line["config"]["global_batch"]
    assert sorted(set(arrays["gang_wave"])) == [0.0, 1.0] and (np.diff(arrays["gang_wave"]) >= 0).all()
    assert set(arrays["gang_size"]) <= {1.0, 2.0, 4.0, 8.0}
    assert (arrays["gang_nodes"] >= 1).all() and (arrays["gang_nodes"] <= arrays["gang_size"]).all()
    assert set(arrays["gang_hostable"]) <= {-1.0, 0.0, 1.0}
    # The same arguments schedule the same inputs: gang for gang the same sizes.
    run_bench("--dump-outputs", str(tmp_path))
    for k in ("gang_wave", "gang_size", "wave_pods"):
        assert np.array_equal(np.load(tmp_path / f"{k}.npy"), arrays[k]), k
