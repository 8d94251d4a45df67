"""The fp6 screen's three-sum test (WLD_OPT_FP6_THREE), checked on the host by
tests/cpp/f6_three_check.cpp: wherever r2_screen_terms_xy2_t (pair_common.hpp)
skips a pair from the three sums and the cap on the missing-by-missing one,
r2_screen_terms_xy2 on the true four sums, in f32, skips it too: on 10^7
random and adversarial tables at fixed and boundary thresholds, through
f6c_direct and, for every e2m3 code, through f6s_direct, and on every pair of a
512 x 2,000 sample of bench.synth's distribution with C4's constants, where at
most 1 pair in 10^4 may be left in doubt.  A stand-alone program, plain and
under AddressSanitizer + UndefinedBehaviorSanitizer (host code only)."""
import os
import subprocess

import pytest

from conftest import REPO

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("san", [[], [x for f in SAN for x in ("-Xarch_host", f)] + ["-g"]],
                         ids=["plain", "asan_ubsan"])
def test_f6_three_implies_four(tmp_path, san):
    exe = str(tmp_path / "f6_three_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    *san, "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    "-x", "hip", os.path.join(REPO, "tests", "cpp", "f6_three_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
