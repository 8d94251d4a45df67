"""The CLI's --matrix-banded flag: the help text and the argument errors (it
needs --matrix-output, --matrix-format npy and a window, and takes no
--matrix-region), all raised before any GPU step (checkable without a device)
and before any output file is written."""
import os
import subprocess

import pytest

from conftest import CLI, FIXTURES

VCF = os.path.join(FIXTURES, "t7_1000genome.vcf")


def run(tmp_path, *args, pair=True):
    base = [CLI, "--vcf-input", VCF]
    if pair:
        base += ["--pair-output", str(tmp_path / "p.tsv")]
    return subprocess.run([*base, *args], capture_output=True, text=True, timeout=120)


def test_help_lists_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--matrix-banded" in r.stdout


@pytest.mark.parametrize("args,needle", [
    (["--matrix-banded"], "'--matrix-banded' needs '--matrix-output"),
    (["--matrix-banded", "--max-sites", "3"], "'--matrix-banded' needs '--matrix-output"),
    (["--matrix-banded", "--matrix-output", "b.npy", "--max-sites", "3"], "'--matrix-banded' needs '--matrix-format npy"),
    (["--matrix-banded", "--matrix-output", "b.npy", "--matrix-format", "tsv", "--max-sites", "3"],
     "'--matrix-banded' needs '--matrix-format npy"),
    (["--matrix-banded", "--matrix-output", "b.npy", "--matrix-format", "npy", "--max-sites", "3", "--matrix-region", "1:9"],
     "'--matrix-banded' cannot be used with '--matrix-region"),
    (["--matrix-banded", "--matrix-output", "b.npy", "--matrix-format", "npy"],
     "'--matrix-banded' needs '--max-distance or --max-sites"),
    (["--matrix-banded", "--matrix-output", "b.npy", "--matrix-format", "npy", "--max-sites", "3", "--devices", "0,0"],
     "'--matrix-output' cannot be used with '--devices"),
])
@pytest.mark.parametrize("pair", [True, False], ids=["with_pairs", "alone"])
def test_argument_errors(tmp_path, args, needle, pair):
    r = run(tmp_path, *args, pair=pair)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and needle in r.stderr, r.stderr
    assert "For more information try --help" in r.stderr
    assert not os.path.exists("b.npy") and not (tmp_path / "p.tsv").exists()
