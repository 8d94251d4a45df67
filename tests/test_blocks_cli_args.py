"""The CLI's LD-block flags (--blocks-output, --blocks-r2, --blocks-dprime,
--blocks-rule, --blocks-min-sites): the help text and the argument errors, all
raised before any GPU step (checkable without a device)."""
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
    for flag in ("--blocks-output", "--blocks-r2", "--blocks-dprime", "--blocks-rule", "--blocks-min-sites"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args,needle", [
    (["--blocks-output", "b.tsv"], "--blocks-r2 <blocks-r2> or --blocks-dprime <blocks-dprime>"),  # no threshold
    (["--blocks-output", "b.tsv", "--blocks-r2", "0.5", "--blocks-dprime", "0.5"],
     "'--blocks-r2' cannot be used with '--blocks-dprime'"),                                       # both
    (["--blocks-output", "b.tsv", "--blocks-r2", "0.5", "--blocks-rule", "solid"], "Invalid value for '--blocks-rule'"),
    (["--blocks-output", "b.tsv", "--blocks-r2", "0.5", "--blocks-rule"], "--blocks-rule"),        # no value
    (["--blocks-output", "b.tsv", "--blocks-r2", "0.5", "--blocks-min-sites", "1"],
     "Invalid value for '--blocks-min-sites' (at least 2)"),
    (["--blocks-output", "b.tsv", "--blocks-r2", "0.5", "--blocks-min-sites", "0"],
     "Invalid value for '--blocks-min-sites' (at least 2)"),
    (["--blocks-output", "b.tsv", "--blocks-r2", "0.5", "--blocks-min-sites", "-2"],
     "Invalid value for '--blocks-min-sites' (at least 2)"),
    (["--blocks-output", "b.tsv", "--blocks-r2", "0.5", "--blocks-min-sites", "x"],
     "Invalid value for '--blocks-min-sites' (at least 2)"),
    (["--blocks-output", "b.tsv", "--blocks-r2", "0.5", "--blocks-min-sites", "99999999999999999999"],
     "Invalid value for '--blocks-min-sites'"),
    (["--blocks-output", "b.tsv", "--blocks-r2", "inf"], "Invalid value for '--blocks-r2' (a finite number)"),
    (["--blocks-output", "b.tsv", "--blocks-dprime", "nan"], "Invalid value for '--blocks-dprime' (a finite number)"),
    (["--blocks-r2", "0.5"], "'--blocks-r2' needs '--blocks-output"),                              # options without an output
    (["--blocks-dprime", "0.5"], "'--blocks-dprime' needs '--blocks-output"),
    (["--blocks-rule", "spine"], "'--blocks-rule' needs '--blocks-output"),
    (["--blocks-min-sites", "3"], "'--blocks-min-sites' needs '--blocks-output"),
])
@pytest.mark.parametrize("pair", [True, False], ids=["with_pairs", "alone"])
def test_argument_errors(tmp_path, args, needle, pair):
    r = run(tmp_path, *args, pair=pair)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and needle in r.stderr, r.stderr
    assert "For more information try --help" in r.stderr
    assert not (tmp_path / "b.tsv").exists() and not os.path.exists("b.tsv")


def test_invalid_threshold(tmp_path):
    r = run(tmp_path, "--blocks-output", str(tmp_path / "b.tsv"), "--blocks-r2", "abc")
    assert r.returncode == 1 and "blocks-r2" in r.stderr, r.stderr


def test_no_output_at_all_still_asks_for_the_pair_output(tmp_path):
    r = run(tmp_path, pair=False)
    assert r.returncode == 1 and "--pair-output <pair-output>" in r.stderr, r.stderr
