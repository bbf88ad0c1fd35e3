"""The index arithmetic of k_paths' per-wave path pool (csrc/path_pool.h: pop count, batch-due decision, push and pop
positions, capacity bound), driven on the CPU by tools/path_pool_check.cpp: one wave's round structure over passes of
random length with random finish patterns for 10^5 rounds.  The program asserts that the pool never exceeds its bound,
that every pushed entry is popped exactly once, that every slot is traced to its end once and that every pass
terminates; this test builds it with the host compiler and runs it.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which(os.environ.get("CXX", "g++"))


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("path_pool") / "path_pool_check")
    cmd = [CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "another_raytracer_amd", "csrc"),
           os.path.join(ROOT, "tools", "path_pool_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_pool_arithmetic_over_random_finish_patterns(check_bin, seed):
    r = subprocess.run([check_bin, "100000", str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    m = re.search(r"ok: (\d+) rounds, (\d+) passes, (\d+) batches, (\d+) entries pushed and popped, most entries at once (\d+) \(bound (\d+), capacity (\d+)\)",
                  r.stdout)
    assert m, r.stdout
    rounds, passes, batches, pushed, high, bound, cap = (int(x) for x in m.groups())
    assert rounds >= 100000 and passes > 1 and batches > passes
    assert pushed > 0  # the run did displace paths
    assert high <= bound <= cap
