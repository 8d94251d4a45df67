"""The CLI's --omega-* flags: the help text and the argument errors
(--omega-output needs --omega-max-side, every other --omega-* flag needs
--omega-output, bad values, no --devices), all raised before any GPU step
(checkable without a device) and before any output file is written."""
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


def test_help_lists_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--omega-output", "--omega-max-side", "--omega-grid", "--omega-min-side", "--omega-max-distance",
                 "--omega-eps"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args,needle", [
    (["--omega-output", "o.tsv"], "--omega-max-side <omega-max-side>"),
    (["--omega-max-side", "5"], "'--omega-max-side' needs '--omega-output"),
    (["--omega-grid", "5"], "'--omega-grid' needs '--omega-output"),
    (["--omega-eps", "0.1", "--omega-min-side", "3"], "'--omega-eps' needs '--omega-output"),
    (["--omega-output", "o.tsv", "--omega-max-side", "0"], "Invalid value for '--omega-max-side'"),
    (["--omega-output", "o.tsv", "--omega-max-side", "five"], "Invalid value for '--omega-max-side'"),
    (["--omega-output", "o.tsv", "--omega-max-side", "5", "--omega-min-side", "1"], "Invalid value for '--omega-min-side'"),
    (["--omega-output", "o.tsv", "--omega-max-side", "5", "--omega-grid", "-3"], "Invalid value for '--omega-grid'"),
    (["--omega-output", "o.tsv", "--omega-max-side", "5", "--omega-max-distance", "1e3"],
     "Invalid value for '--omega-max-distance'"),
    (["--omega-output", "o.tsv", "--omega-max-side", "5", "--omega-eps", "-1"], "Invalid value for '--omega-eps'"),
    (["--omega-output", "o.tsv", "--omega-max-side", "5", "--omega-eps", "nan"], "Invalid value for '--omega-eps'"),
    (["--omega-output", "o.tsv", "--omega-max-side", "5", "--omega-eps", "inf"], "Invalid value for '--omega-eps'"),
    (["--omega-output", "o.tsv", "--omega-max-side", "5", "--devices", "0,0"], "'--omega-output' cannot be used with '--devices"),
])
@pytest.mark.parametrize("pair", [True, False], ids=["with_pairs", "alone"])
def test_argument_errors(tmp_path, args, needle, pair):
    r = run(tmp_path, *args, pair=pair)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and needle in r.stderr, r.stderr
    assert "For more information try --help" in r.stderr
    assert not os.path.exists("o.tsv") and not (tmp_path / "p.tsv").exists()
