"""`ska distance --no-table` at the command line: what it refuses, byte for byte and with no file created, and its help line.  No device is
needed: clap's refusals come before one is touched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
HINT = "\n\nFor more information, try '--help'.\n"
USAGE = "\n\nUsage: ska distance [OPTIONS] <SKF_FILE>"
OUTPUTS = [["--tree", "t.nwk"], ["--clusters", "c"], ["--tree", "t.nwk", "--clusters", "c", "--cluster-snps", "3"]]
OTHERS = [(["-o", "out.tsv"], "-o <OUTPUT>"), (["--max-snps", "3"], "--max-snps <N>"), (["--max-mismatches", "0.5"], "--max-mismatches <P>"),
          (["--closest", "2"], "--closest <K>"), (["--query", "a"], "--query <NAMES>"), (["--query-file", "q.txt"], "--query-file <FILE>"),
          (["--query-skf", "b.skf"], "--query-skf <FILE>"), (["--gpus", "2"], "--gpus <GPUS>")]


def _ska(*args, cwd):
    return subprocess.run([SKA, *args], cwd=cwd, capture_output=True, timeout=300)


def _refused(r, message, wd):
    assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", message), r.stderr
    assert sorted(os.listdir(wd)) == ["q.txt"]                                  # no file created


@pytest.fixture
def wd(tmp_path):
    (tmp_path / "q.txt").write_text("a\n")
    return str(tmp_path)


def test_help_names_the_option():
    out = _ska("distance", "--help", cwd=ROOT).stdout.decode()
    line = [ln for ln in out.splitlines() if ln.lstrip().startswith("--no-table")]
    assert len(line) == 1
    assert "(MI355X engine)" in line[0] and "graph.dot" in line[0] and "--max-snps" in line[0]
    assert out.index("--cluster-mismatches <P>") < out.index("--no-table") < out.index("--query <NAMES>")


def test_no_table_needs_a_tree_or_clusters(wd):
    r = _ska("distance", "x.skf", "--no-table", cwd=wd)
    _refused(r, "error: the following required arguments were not provided:\n  <--tree <FILE>|--clusters <PREFIX>>" + USAGE + HINT, wd)


@pytest.mark.parametrize("other, oarg", OTHERS, ids=[o[1].split()[0] for o in OTHERS])
def test_no_table_refuses_the_table_and_its_cuts(wd, other, oarg):
    for outputs in OUTPUTS:
        for args in (["--no-table", *outputs, *other], [*other, *outputs, "--no-table"]):            # --no-table is named first either way
            r = _ska("distance", "x.skf", *args, cwd=wd)
            _refused(r, f"error: the argument '--no-table' cannot be used with '{oarg}'" + USAGE + HINT, wd)
    r = _ska("distance", "x.skf", "--no-table", *other, cwd=wd)                                         # the conflict comes before the missing group
    _refused(r, f"error: the argument '--no-table' cannot be used with '{oarg}'" + USAGE + HINT, wd)


def test_the_cluster_options_are_checked_as_before(wd):
    r = _ska("distance", "x.skf", "--no-table", "--tree", "t.nwk", "--cluster-snps", "3", cwd=wd)
    _refused(r, "error: the following required arguments were not provided:\n  --clusters <PREFIX>" + USAGE + HINT, wd)
    r = _ska("distance", "x.skf", "--no-table", "--clusters", "c", "--cluster-snps", "-1", cwd=wd)
    _refused(r, "error: invalid value '-1' for '--cluster-snps <N>': Threshold must be zero or higher" + HINT, wd)


def test_other_subcommands_refuse_the_option(wd):
    r = _ska("align", "x.skf", "--no-table", cwd=wd)
    _refused(r, "error: unexpected argument '--no-table' found\n\nUsage: ska align [OPTIONS]" + HINT, wd)
