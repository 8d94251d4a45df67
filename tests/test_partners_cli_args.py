"""The CLI's best-partner flags (--partners-output, --partners-k,
--partners-r2): the help text and the argument errors, all raised before any
GPU step (checkable without a device)."""
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
    for flag in ("--partners-output", "--partners-k", "--partners-r2"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args,needle", [
    (["--partners-output", "b.tsv"], "--partners-k <partners-k>"),                              # missing K
    (["--partners-k", "4"], "'--partners-k' needs '--partners-output"),                         # K without an output
    (["--partners-r2", "0.3"], "'--partners-r2' needs '--partners-output"),
    (["--partners-output", "b.tsv", "--partners-k", "0"], "Invalid value for '--partners-k' (1 to 64)"),
    (["--partners-output", "b.tsv", "--partners-k", "65"], "Invalid value for '--partners-k' (1 to 64)"),
    (["--partners-output", "b.tsv", "--partners-k", "-3"], "Invalid value for '--partners-k' (1 to 64)"),
    (["--partners-output", "b.tsv", "--partners-k", "x"], "Invalid value for '--partners-k' (1 to 64)"),
    (["--partners-output", "b.tsv", "--partners-k", "99999999999999999999"], "Invalid value for '--partners-k'"),
    (["--partners-output", "b.tsv", "--partners-k"], "--partners-k"),                           # no value
])
@pytest.mark.parametrize("pair", [True, False], ids=["with_pairs", "alone"])
def test_argument_errors(tmp_path, args, needle, pair):
    r = run(tmp_path, *args, pair=pair)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and needle in r.stderr, r.stderr
    assert "For more information try --help" in r.stderr
    assert not (tmp_path / "b.tsv").exists() and not os.path.exists("b.tsv")


def test_invalid_threshold(tmp_path):
    r = run(tmp_path, "--partners-output", str(tmp_path / "b.tsv"), "--partners-k", "4", "--partners-r2", "abc")
    assert r.returncode == 1 and "partners-r2" in r.stderr, r.stderr


def test_no_output_at_all_still_asks_for_the_pair_output(tmp_path):
    r = run(tmp_path, pair=False)
    assert r.returncode == 1 and "--pair-output <pair-output>" in r.stderr, r.stderr
