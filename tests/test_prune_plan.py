"""LD pruning's host-side pieces (weightedld_amd/csrc/prune_plan.hpp: the rank
of a priority, sequential greedy with tags, the round rule) against a
restatement and under random asynchronous schedules
(tests/cpp/prune_plan_check.cpp, host only), plain and under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone host program)."""
import os
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_prune_plan_rounds_reach_greedy(tmp_path, san):
    exe = str(tmp_path / "prune_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *san,
                    "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "prune_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
