"""The fp6 screen's quick test (WLD_OPT_FP6_QUICK), checked on the host by
tests/cpp/f6_quick_check.cpp: wherever f6q_lane_terms / f6q_skip
(pair_common.hpp) reject a lane's 16 pairs of a row block together, from one
numerator maximum and marginal bounds shared by the lane, r2_screen_terms_f6t
rejects every one of them, in f32, and each pair's numerator maximum is the
full test's bit for bit: on more than 10^6 lane tests built from small
alignments (weights on the 1/8 grid, the shared route for every e2m3 code,
adversarial columns, fixed and boundary thresholds) and on every lane of a
2,048 x 2,000 sample of bench.synth's distribution with C4's constants, where
at most 1/10 of the row blocks may fall through to the full test.  A
stand-alone program, plain and under AddressSanitizer +
UndefinedBehaviorSanitizer (host code only)."""
import os
import subprocess

import pytest

from conftest import REPO

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("san", [[], [x for f in SAN for x in ("-Xarch_host", f)] + ["-g"]],
                         ids=["plain", "asan_ubsan"])
def test_f6_quick_implies_full(tmp_path, san):
    exe = str(tmp_path / "f6_quick_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    *san, "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    "-x", "hip", os.path.join(REPO, "tests", "cpp", "f6_quick_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
