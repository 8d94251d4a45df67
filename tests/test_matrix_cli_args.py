"""The CLI's LD-matrix flags (--matrix-output, --matrix-stat, --matrix-region,
--matrix-format, --matrix-zero-missing): the help text and the argument
errors, all raised before any GPU step (checkable without a device) and before
any output file is written."""
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
    for flag in ("--matrix-output", "--matrix-stat", "--matrix-region", "--matrix-format", "--matrix-zero-missing"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args,needle", [
    (["--matrix-stat", "r2"], "'--matrix-stat' needs '--matrix-output"),
    (["--matrix-region", "1:9"], "'--matrix-region' needs '--matrix-output"),
    (["--matrix-format", "npy"], "'--matrix-format' needs '--matrix-output"),
    (["--matrix-zero-missing"], "'--matrix-zero-missing' needs '--matrix-output"),
    (["--matrix-output", "m.tsv", "--matrix-stat", "rho"], "Invalid value for '--matrix-stat'"),
    (["--matrix-output", "m.tsv", "--matrix-stat", "R"], "Invalid value for '--matrix-stat'"),
    (["--matrix-output", "m.tsv", "--matrix-format", "csv"], "Invalid value for '--matrix-format'"),
    (["--matrix-output", "m.tsv", "--matrix-region", "9"], "Invalid value for '--matrix-region' (START:END)"),
    (["--matrix-output", "m.tsv", "--matrix-region", "9:3"], "Invalid value for '--matrix-region' (START:END)"),
    (["--matrix-output", "m.tsv", "--matrix-region", "a:3"], "Invalid value for '--matrix-region' (START:END)"),
    (["--matrix-output", "m.tsv", "--matrix-region", ":3"], "Invalid value for '--matrix-region' (START:END)"),
    (["--matrix-output", "m.tsv", "--matrix-region", "-1:3"], "--matrix-region"),
    (["--matrix-output", "m.tsv", "--devices", "0,0"], "'--matrix-output' cannot be used with '--devices"),
    (["--matrix-stat", "r", "--matrix-output"], "--matrix-output"),  # no value
])
@pytest.mark.parametrize("pair", [True, False], ids=["with_pairs", "alone"])
def test_argument_errors(tmp_path, args, needle, pair):
    r = run(tmp_path, *args, pair=pair)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and needle in r.stderr, r.stderr
    assert "For more information try --help" in r.stderr
    assert not os.path.exists("m.tsv") and not (tmp_path / "p.tsv").exists()


def test_matrix_output_alone_is_enough():
    """--matrix-output stands in for --pair-output: the missing-argument error is not raised
    (the run then ends at the input file, before any GPU step)."""
    r = subprocess.run([CLI, "--vcf-input", os.path.join(FIXTURES, "no_such.vcf"), "--matrix-output", "m.tsv"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "required arguments" not in r.stderr, r.stderr
    assert not os.path.exists("m.tsv")
