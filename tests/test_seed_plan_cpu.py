"""CPU-only: the pass arithmetic of the seeding stage (pyani_amd/csrc/pg_seed_plan.h), which the host planners and both seeding
kernels share, compiled for the host into a stand-alone program (tests/seed_plan/plan_check.cpp)."""
import subprocess

import pytest

from tests.conftest import ROOT

SRC = ROOT / "tests" / "seed_plan" / "plan_check.cpp"
CASES = 3 * 10 + 1   # S in {256, 512, 16384} x ten group sizes, and the 2^32 - 1 case


def _build_and_run(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, f"-I{ROOT / 'pyani_amd' / 'csrc'}", str(SRC), "-o", str(exe)],
                   check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.mark.parametrize("name,extra", [("plan_check", []), ("plan_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_passes_cover_every_entry_once(tmp_path, name, extra):
    """For n in {0, 1, H-1, H, H+1, 2H-1, 2H, 2H+1, 9000, 10^6} and S in {256, 512, 16384}: the passes cover [0, n) exactly once and in
    order, none holds more than H = S / 2 entries, P == 1 exactly when n <= H, n == 0 gives one empty pass; and n = 2^32 - 1 does
    not wrap.  Built a second time with -fsanitize=address,undefined (a stand-alone host program: it needs no preloading)."""
    out = _build_and_run(tmp_path, name, extra)
    assert out.returncode == 0 and "WRONG" not in out.stdout and out.stdout.count("ok ") == CASES, out.stdout + out.stderr
    assert f"{CASES} cases, 0 wrong" in out.stdout
