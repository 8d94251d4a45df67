"""The banded Cholesky factorisation's host-side step list
(weightedld_amd/csrc/banded_chol_plan.hpp: per block row the panel's column
extent, its blocks, the trailing window's block list, the blocks the solves
walk, the launch count) against brute force
(tests/cpp/banded_chol_plan_check.cpp, host only), plain and under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone host program)."""
import os
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_banded_chol_plan_against_brute_force(tmp_path, san):
    exe = str(tmp_path / "banded_chol_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *san,
                    "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "banded_chol_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
