"""bench.py --full, on CPU with the rehearsal engine (PYANI_BENCH_REHEARSAL=1): a plain run times the steps and prints the line
without the records that take runs of their own; --full adds them and leaves the timed steps' records as they were."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _bench(*extra):
    env = dict(os.environ, PYANI_BENCH_REHEARSAL="1", PYANI_BENCH_REHEARSAL_SCALE="0")
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--genomes", "100", "--length", "2000", "--steps", "10", "--warmup", "1", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_leaves_the_roofline_pass_to_full():
    plain, full = _bench(), _bench("--full")
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[key] == full[key], key
    assert plain["roofline"] is None
    # the one-worker pass over every tile of the grid: ten tiles of 10 rows at 100 genomes
    assert full["roofline"]["tiles"] == 10 and full["roofline"]["one_worker_step"]["pairs"] == 100 * 99
    # the timed steps cover the grid either way: the same records, hence the same hash
    assert plain["config"]["results_sha1_full_grid"] and plain["config"]["results_sha1_full_grid"] == full["config"]["results_sha1_full_grid"]
    assert plain["config"]["pairs_timed"] == full["config"]["pairs_timed"] == 100 * 99
