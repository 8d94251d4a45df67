"""The partitioned LD scores' host-side pieces (weightedld_amd/csrc/annot_plan.hpp:
the validation, the padded annotation image with its zero-chunk mask, the
self-term rule, the merge, the annotation-file reader and its merge-join)
against brute force (tests/cpp/annot_plan_check.cpp, host only), plain and
under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone host
program)."""
import os
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_annot_plan_against_brute_force(tmp_path, san):
    exe = str(tmp_path / "annot_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *san,
                    "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "annot_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
