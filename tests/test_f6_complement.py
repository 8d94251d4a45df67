"""The fp6 screen's complement coding (pair_common.hpp f6c_direct: the direct
coding's accumulators restored exactly from the complement-coded ones and the
per-site marginals) and its weight-code scale rule (fp6_scale.hpp), checked
on the host by tests/cpp/f6_complement_check.cpp: a stand-alone program, plain
and under AddressSanitizer + UndefinedBehaviorSanitizer (host code only)."""
import os
import subprocess

import pytest

from conftest import REPO

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("san", [[], [x for f in SAN for x in ("-Xarch_host", f)] + ["-g"]],
                         ids=["plain", "asan_ubsan"])
def test_f6_complement_and_scale_rule(tmp_path, san):
    exe = str(tmp_path / "f6_complement_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    *san, "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    "-x", "hip", os.path.join(REPO, "tests", "cpp", "f6_complement_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
