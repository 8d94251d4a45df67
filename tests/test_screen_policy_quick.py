"""The quick-test rule of the pair pass's screen policy
(weightedld_amd/csrc/screen_policy.hpp: WLD_OPT_FP6_QUICK, the sample run's
quarter of the row blocks, the learned threshold, lists without a sample),
checked by tests/cpp/screen_policy_quick_check.cpp, plain and under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone host program)."""
import os
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_screen_policy_quick_rule(tmp_path, san):
    exe = str(tmp_path / "screen_policy_quick_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", *san,
                    "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "screen_policy_quick_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
