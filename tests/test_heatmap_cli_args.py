"""The CLI's heat-map flags (--heatmap-output, --heatmap-cell-width,
--heatmap-cell-sites, --heatmap-region, --heatmap-stat): the help text and the
argument errors, all raised before any GPU step (checkable without a device)."""
import os
import subprocess

import pytest

from conftest import CLI, FIXTURES

VCF = os.path.join(FIXTURES, "t7_1000genome.vcf")


def run(tmp_path, *args, vcf=True):
    base = [CLI, "--vcf-input", VCF] if vcf else [CLI, "--fasta-input", os.path.join(FIXTURES, "example.fasta")]
    return subprocess.run([*base, "--pair-output", str(tmp_path / "p.tsv"), *args], capture_output=True, text=True,
                          timeout=120)


def test_help_lists_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--heatmap-output", "--heatmap-cell-width", "--heatmap-cell-sites", "--heatmap-region",
                 "--heatmap-stat"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args,needle", [
    (["--heatmap-output", "h.tsv"], "--heatmap-cell-width <heatmap-cell-width> or --heatmap-cell-sites"),  # no cell size
    (["--heatmap-output", "h.tsv", "--heatmap-cell-width", "100", "--heatmap-cell-sites", "4"],
     "'--heatmap-cell-width' cannot be used with '--heatmap-cell-sites'"),                              # both sizes
    (["--heatmap-cell-width", "100"], "'--heatmap-cell-width' needs '--heatmap-output"),                # a size, no output
    (["--heatmap-cell-sites", "4"], "'--heatmap-cell-sites' needs '--heatmap-output"),
    (["--heatmap-region", "1:9"], "'--heatmap-region' needs '--heatmap-output"),
    (["--heatmap-stat", "r2"], "'--heatmap-stat' needs '--heatmap-output"),
    (["--heatmap-output", "h.tsv", "--heatmap-cell-width", "0"], "Invalid value for '--heatmap-cell-width'"),
    (["--heatmap-output", "h.tsv", "--heatmap-cell-sites", "x"], "Invalid value for '--heatmap-cell-sites'"),
    (["--heatmap-output", "h.tsv", "--heatmap-cell-sites", "4", "--heatmap-stat", "d"],
     "Invalid value for '--heatmap-stat'"),
    (["--heatmap-output", "h.tsv", "--heatmap-cell-sites", "4", "--heatmap-region", "100"],
     "Invalid value for '--heatmap-region' (START:END)"),                                               # malformed regions
    (["--heatmap-output", "h.tsv", "--heatmap-cell-sites", "4", "--heatmap-region", "100:"], "(START:END)"),
    (["--heatmap-output", "h.tsv", "--heatmap-cell-sites", "4", "--heatmap-region", ":100"], "(START:END)"),
    (["--heatmap-output", "h.tsv", "--heatmap-cell-sites", "4", "--heatmap-region", "9:1"], "(START:END)"),
    (["--heatmap-output", "h.tsv", "--heatmap-cell-sites", "4", "--heatmap-region", "1-9"], "(START:END)"),
])
def test_argument_errors(tmp_path, args, needle):
    r = run(tmp_path, *args)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and needle in r.stderr, r.stderr
    assert "For more information try --help" in r.stderr


def test_too_many_cells_and_empty_regions(tmp_path):
    """Known once the input is read, still before any GPU step."""
    # the fixture with its last record moved 5,000 coordinates on
    lines = open(VCF).read().splitlines()
    rec = [i for i, line in enumerate(lines) if not line.startswith("#")]
    pos = [int(lines[i].split("\t")[1]) for i in rec]
    f = lines[rec[-1]].split("\t")
    f[1] = str(pos[0] + 5000)
    lines[rec[-1]] = "\t".join(f)
    wide = tmp_path / "wide.vcf"
    wide.write_text("\n".join(lines) + "\n")
    h = str(tmp_path / "h.tsv")
    r = subprocess.run([CLI, "--vcf-input", str(wide), "--pair-output", str(tmp_path / "p.tsv"), "--heatmap-output", h,
                        "--heatmap-cell-width", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "at most 4096" in r.stderr and "5001 cells" in r.stderr, r.stderr
    r = run(tmp_path, "--heatmap-output", h, "--heatmap-cell-width", "10", "--heatmap-region", "0:%d" % min(pos))
    assert r.returncode == 1 and "no site of interest is on a cell" in r.stderr, r.stderr
    assert not (tmp_path / "h.tsv").exists()
