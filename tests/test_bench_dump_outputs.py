"""bench.py --dump-outputs and --steps, on CPU: the real step loop of the anim workload with the rehearsal engine
(PYANI_BENCH_REHEARSAL=1, a stub whose records are a function of the pair), and the size cap of the dump itself."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
FIELDS = ["ref_genome", "qry_genome", "ref_aln_len", "qry_aln_len", "sim_errors", "n_alignments", "identity", "status"]


def _bench(out_dir, steps, warmup):
    env = dict(os.environ, PYANI_BENCH_REHEARSAL="1", PYANI_BENCH_REHEARSAL_SCALE="0")
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--genomes", "100", "--length", "2000",
           "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_dump_outputs_holds_the_last_timed_step(tmp_path):
    line = _bench(tmp_path / "a", steps=3, warmup=1)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    # 100 genomes, 10 rows per step: the timed steps are steps 1, 2, 3; the last one covers rows 30 ... 39
    from pyani_amd import parallel
    want = parallel.anim_pair_array(100, list(range(30, 40)), symmetric=True)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in FIELDS}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(f"{k}.npy" for k in FIELDS)
    assert all(a.dtype == np.float64 and a.shape == (len(want),) for a in got.values())
    assert (got["ref_genome"] == want[:, 0]).all() and (got["qry_genome"] == want[:, 1]).all()
    # the rehearsal engine's records: ref_aln_len = r * 1000 + q, qry_aln_len = q * 1000 + r
    assert (got["ref_aln_len"] == want[:, 0] * 1000 + want[:, 1]).all() and (got["qry_aln_len"] == want[:, 1] * 1000 + want[:, 0]).all()
    # same arguments, same outputs
    _bench(tmp_path / "b", steps=3, warmup=1)
    assert all((np.load(tmp_path / "b" / f"{k}.npy") == got[k]).all() for k in FIELDS)


def test_steps_sets_the_timed_steps(tmp_path):
    one, two = _bench(tmp_path / "one", steps=1, warmup=0), _bench(tmp_path / "two", steps=2, warmup=0)
    assert (one["steps"], two["steps"]) == (1, 2)
    assert two["config"]["pairs_timed"] == 2 * one["config"]["pairs_timed"]


def test_dump_is_capped_by_a_fixed_sample(tmp_path, monkeypatch):
    sys.path.insert(0, str(ROOT))
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 1000)
    a, b = np.arange(5000, dtype=np.int64), np.arange(5000, dtype=np.float64) * 0.5
    for d in ("x", "y"):
        bench.dump_outputs(tmp_path / d, {"a": a, "b": b})
    rows = np.load(tmp_path / "x" / "sample_rows.npy")
    total = sum(np.load(p).nbytes for p in (tmp_path / "x").iterdir())
    assert total <= 8 * 1000 and len(rows) > 0 and (np.diff(rows) > 0).all()
    assert (np.load(tmp_path / "x" / "a.npy") == rows).all() and (np.load(tmp_path / "x" / "b.npy") == rows * 0.5).all()
    assert (np.load(tmp_path / "y" / "sample_rows.npy") == rows).all()
