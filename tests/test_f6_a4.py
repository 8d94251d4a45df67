"""The fp6 screen's fp4 A image (WLD_OPT_FP6_A4), checked on the host by
tests/cpp/f6_a4_check.cpp: the e2m3 -> e2m1 code map and the predicate that
lets a load take the image (fp6_scale.hpp), the weight sets the committed scale
rule puts on e2m1 values, and the lane packing of both A formats
(fp6_pack.hpp, the code frag6_kernel runs): same values at the same (site,
sequence), same block sums.  A stand-alone program, plain and under
AddressSanitizer + UndefinedBehaviorSanitizer (host code only)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
# tests/test_gpu_fp6_complement.py's "spread" weights at N = 130: 27 e2m3 codes under the scale rule
SPREAD_N, SPREAD_CODES = 130, 27


@pytest.mark.parametrize("san", [[], [x for f in SAN for x in ("-Xarch_host", f)] + ["-g"]],
                         ids=["plain", "asan_ubsan"])
def test_f6_a4_map_rule_and_packing(tmp_path, san):
    exe = str(tmp_path / "f6_a4_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall",
                    *san, "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    "-x", "hip", os.path.join(REPO, "tests", "cpp", "f6_a4_check.cpp"), "-o", exe], check=True)
    spread = str(tmp_path / "spread.f32")
    np.exp2(-4.0 * np.random.default_rng(5 + SPREAD_N).random(SPREAD_N)).astype(np.float32).tofile(spread)
    out = subprocess.run([exe, spread, str(SPREAD_CODES)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
