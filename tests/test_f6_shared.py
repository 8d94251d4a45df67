"""The fp6 screen's shared code image (WLD_OPT_FP6_SHARED), checked on the host
by tests/cpp/f6_shared_check.cpp: the qualification (fp6_scale.hpp
fp6_shared_code: every weight code the same nonzero code), the two masks that
turn a shared-image dword into the fp4 A image's channels at the weights 2.0
and 1.0, the padded tail coded 0 (fp6_pack.hpp f6_pack_lane_shared), and the
restoration of the direct coding's sums from the count accumulators for every
e2m3 code (pair_common.hpp f6s_direct), bit for bit.  A stand-alone program,
plain and under AddressSanitizer + UndefinedBehaviorSanitizer (host code
only)."""
import os
import subprocess

import pytest

from conftest import REPO

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.parametrize("san", [[], [x for f in SAN for x in ("-Xarch_host", f)] + ["-g"]],
                         ids=["plain", "asan_ubsan"])
def test_f6_shared_qualification_masks_and_restoration(tmp_path, san):
    exe = str(tmp_path / "f6_shared_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    *san, "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    "-x", "hip", os.path.join(REPO, "tests", "cpp", "f6_shared_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
