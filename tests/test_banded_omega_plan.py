"""The sweep scan's host-side plan (weightedld_amd/csrc/banded_omega_plan.hpp:
the chain pass's parallelogram tiling of a band's pair-sum table with its
clipping at both ends, at K < 64 and at K >= n, the candidate counts of a
split, and the splits of a scan from coordinates) against brute force over
every (n, K) with n <= 200 and K <= 140 (tests/cpp/banded_omega_plan_check.cpp,
host only), plain and under AddressSanitizer + UndefinedBehaviorSanitizer (a
stand-alone host program)."""
import os
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_banded_omega_plan_against_brute_force(tmp_path, san):
    exe = str(tmp_path / "banded_omega_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *san,
                    "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "banded_omega_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
