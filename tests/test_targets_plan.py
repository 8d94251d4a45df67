"""The target-site run's host-side plan (weightedld_amd/csrc/targets_plan.hpp:
list validation, the lower window limit and partner ranges, blocks of 16 sorted
targets with the permutation back to list positions, the work items and the
batch cuts) against brute force (tests/cpp/targets_plan_check.cpp, host only),
plain and under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone
host program, nothing preloaded)."""
import os
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_targets_plan_matches_brute_force(tmp_path, san):
    exe = str(tmp_path / "targets_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *san,
                    "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "targets_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
