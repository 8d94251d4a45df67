"""The LD blocks' host-side pieces (weightedld_amd/csrc/blocks_plan.hpp: the
partition of the site axis from the break arrays under both rules, the merge
of break arrays by min / max, pass 2's tile list and id limits, the inverted
min key, the argument checks) against brute force straight from the
definitions (tests/cpp/blocks_plan_check.cpp, host only), plain and under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone host program)."""
import os
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_blocks_plan_against_brute_force(tmp_path, san):
    exe = str(tmp_path / "blocks_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *san,
                    "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "blocks_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
