"""The pair pass's screen policy (weightedld_amd/csrc/screen_policy.hpp: the
route of a pass, the sample run's precondition, what the auto policy learns,
what a route reports) against a frozen transcription of the logic it replaced
(tests/cpp/screen_policy_check.cpp, host only), plain and under
AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone host program)."""
import os
import subprocess

import pytest

from conftest import REPO


@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_screen_policy_equals_frozen_transcription(tmp_path, san):
    exe = str(tmp_path / "screen_policy_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", *san,
                    "-I", os.path.join(REPO, "weightedld_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "screen_policy_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
