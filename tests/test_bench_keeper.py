"""bench.py's LineKeeper on the CPU: the ONE stdout line survives the death of the process that measured it
(an abort from a library thread inside a side measurement must not lose the SCALE record)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import os, sys
sys.path.insert(0, {root!r})
import bench
k = bench.LineKeeper(os.dup(1))
k.primary({{"value": 1, "n_gpus": 8}})
mode = sys.argv[1]
if mode == "abort":
    os.abort()                      # what c10d's watchdog does to the process: no Python clean-up runs
if mode == "kill":
    os.kill(os.getpid(), 9)
k.final({{"value": 1, "n_gpus": 8, "variants": {{"x": 2}}}})
if mode == "abort_after_final":
    os.abort()
k.close()
"""


def _run(mode):
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT), mode], capture_output=True, text=True, timeout=300, cwd=ROOT)
    lines = [ln for ln in r.stdout.split("\n") if ln.strip()]
    assert len(lines) == 1, (r.stdout, r.stderr[-500:])
    return r.returncode, json.loads(lines[0])


def test_primary_line_survives_abort_and_kill():
    for mode in ("abort", "kill"):
        rc, d = _run(mode)
        assert rc != 0 and d == {"value": 1, "n_gpus": 8}


def test_final_line_replaces_the_primary_one():
    rc, d = _run("clean")
    assert rc == 0 and d["variants"] == {"x": 2}
    rc, d = _run("abort_after_final")
    assert rc != 0 and d["variants"] == {"x": 2}


def test_bare_gpus_n_becomes_its_own_launcher():
    """`python bench.py --gpus 2` with no WORLD_SIZE around it re-executes itself under torch.distributed.run (VERDICT r4
    item 1).  Without a GPU the two ranks it starts stop at `require_gpu` - loudly, no CPU fallback - which is enough to see
    here that BOTH exist; the measured form of this test is tests/test_gpu_bench_contract.py."""
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("the GPU form of this test runs the whole job")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and r.stdout.strip() == ""
    assert "local_rank: 0" in r.stderr and "local_rank: 1" in r.stderr, r.stderr[-1500:]
    assert "no CPU fallback" in r.stderr


def test_dump_outputs_keep_a_fixed_sample_under_the_limit(tmp_path, monkeypatch):
    """bench.dump_outputs: float32 .npy per array; beyond the size limit every array keeps the same seeded rows (rows.npy)"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench

    class Loop:
        def outputs(self):
            return {"scores": torch.arange(1000.0).reshape(1000, 1), "grad": torch.arange(7000.0, dtype=torch.float64).reshape(1000, 7)}
    bench.dump_outputs(Loop(), str(tmp_path / "full"))
    full = {k: np.load(tmp_path / "full" / f"{k}.npy") for k in ("scores", "grad")}
    assert sorted(os.listdir(tmp_path / "full")) == ["grad.npy", "scores.npy"]
    assert full["scores"].dtype == np.float32 and full["grad"].dtype == np.float64 and full["grad"].shape == (1000, 7)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20000)
    for run in ("a", "b"):
        bench.dump_outputs(Loop(), str(tmp_path / run))
    a, b = ({k: np.load(tmp_path / run / f"{k}.npy") for k in ("scores", "grad", "rows")} for run in ("a", "b"))
    assert sum(v.nbytes for v in a.values()) <= 20000 and all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["rows"].astype(np.int64)
    assert len(rows) > 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["scores"], full["scores"][rows]) and np.array_equal(a["grad"], full["grad"][rows])
