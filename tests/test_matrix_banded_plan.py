"""The banded LD matrix's host-side pieces
(weightedld_amd/csrc/matrix_banded_plan.hpp: the argument validation, the
width a window needs, the tile list of a row range, the fill description, the
strip split of the host call and the pair count of a row range) against brute
force (tests/cpp/matrix_banded_plan_check.cpp, host only), plain and under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone host program)."""
import os
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_matrix_banded_plan_against_brute_force(tmp_path, san):
    exe = str(tmp_path / "matrix_banded_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *san,
                    "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "matrix_banded_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
