"""The fp6 screen's per-load site records, count units and one-sided quick test
(pair_common.hpp f6_row_rec / f6_col_rec, f6q_pair1), checked on the host by
tests/cpp/f6_quick_units_check.cpp: the records hold f6t_row's / f6t_col's
fields bit for bit; for every power-of-two weight code the quick test and the
three-sum test on the shared image's raw counts decide exactly as on the scaled
sums; and wherever the quick test on the one-sided cap skips a lane's 16 pairs,
r2_screen_terms_f6t skips every one of them, each pair's nt' being at least
f6q_pair's nt: on more than 10^6 lane tests built from small alignments and
on every lane of a 2,048 x 2,000 sample of bench.synth's distribution with
C4's constants, where at most 1/10 of the 1,984 row blocks may fall through to
the full test (the count is printed).  A stand-alone program, plain and under
AddressSanitizer + UndefinedBehaviorSanitizer (host code only)."""
import os
import subprocess

import pytest

from conftest import REPO

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("san", [[], [x for f in SAN for x in ("-Xarch_host", f)] + ["-g"]],
                         ids=["plain", "asan_ubsan"])
def test_f6_quick_units(tmp_path, san):
    exe = str(tmp_path / "f6_quick_units_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    *san, "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    "-x", "hip", os.path.join(REPO, "tests", "cpp", "f6_quick_units_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
