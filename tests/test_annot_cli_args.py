"""The CLI's partitioned-LD-score flags (--annot-input, --annot-score-output,
--annot-self): the help text, the argument errors and the annotation file's
format errors, all raised before any GPU step (checkable without a device)
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


def vcf_positions():
    """The parent index (POS) of every site the CLI loads from the fixture (host code only)."""
    import weightedld_amd as W
    v = W.read_vcf(VCF)
    return [v.parent_site_index(i) for i in range(v.n_sites())]


def test_help_lists_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--annot-input", "--annot-score-output", "--annot-self"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args,needle", [
    (["--annot-input", "a.tsv"], "'--annot-input' needs '--annot-score-output"),
    (["--annot-score-output", "l2.tsv"], "'--annot-score-output' needs '--annot-input"),
    (["--annot-self"], "'--annot-self' needs '--annot-input"),
    (["--annot-self", "--annot-input", "a.tsv"], "'--annot-input' needs '--annot-score-output"),
    (["--annot-self", "--annot-score-output", "l2.tsv"], "'--annot-score-output' needs '--annot-input"),
    (["--annot-score-output", "l2.tsv", "--annot-input"], "--annot-input"),  # no value
])
@pytest.mark.parametrize("pair", [True, False], ids=["with_pairs", "alone"])
def test_argument_errors(tmp_path, args, needle, pair):
    r = run(tmp_path, *args, pair=pair)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and needle in r.stderr, r.stderr
    assert "For more information try --help" in r.stderr
    assert not os.path.exists("l2.tsv") and not (tmp_path / "p.tsv").exists()


def names(n):
    return "site\t" + "\t".join("n%d" % k for k in range(n)) + "\n"


@pytest.mark.parametrize("text,needle", [
    (None, "cannot read"),                                    # no such file
    ("", "line 1"),                                           # empty
    ("pos\ta\n", "line 1"),                                   # not the header
    (names(129), "129 annotation columns; at most 128"),
    ("site\ta\tb\ta\n", "the name \"a\" appears twice"),
    ("site\ta\t\n", "line 1"),                                # an empty name
    ("site\ta\tb\n1\t2\n", "line 2"),                         # a short row
    ("site\ta\n1\t2\t3\n", "line 2"),                         # a long row
    ("site\ta\n1\t0.5\n2\tx\n", "line 3"),                    # not a number
    ("site\ta\n1\tnan\n", "not finite"),
    ("site\ta\n1\t1e60\n", "not finite"),
    ("site\ta\nrs1\t1\n", "line 2"),                          # not a site index
])
@pytest.mark.parametrize("pair", [True, False], ids=["with_pairs", "alone"])
def test_file_errors(tmp_path, text, needle, pair):
    path = tmp_path / "annot.tsv"
    if text is not None:
        path.write_text(text)
    out = tmp_path / "l2.tsv"
    r = run(tmp_path, "--annot-input", str(path), "--annot-score-output", str(out), "--annot-self", pair=pair)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and needle in r.stderr, r.stderr
    assert not out.exists() and not (tmp_path / "p.tsv").exists()


def test_128_names_pass_the_header_check_and_a_missing_site_is_named(tmp_path):
    """A well-formed file whose rows stop before the last site of interest:
    refused once the sites are known, still before any GPU step."""
    pos = vcf_positions()
    assert len(pos) > 2
    path, out = tmp_path / "annot.tsv", tmp_path / "l2.tsv"
    path.write_text(names(128) + "".join("%d\t%s\n" % (p, "\t".join(["1"] * 128)) for p in pos[:-1]))
    r = run(tmp_path, "--annot-input", str(path), "--annot-score-output", str(out))
    assert r.returncode == 1 and r.stderr.count("error: ") == 1, r.stderr
    assert "no row for site %d" % pos[-1] in r.stderr, r.stderr
    assert not out.exists() and not (tmp_path / "p.tsv").exists()
