"""`ska markers` on the command line, as far as it goes without a device: its help lists every flag, and what it refuses it refuses in clap's
wording with exit code 2, without the banner and before a device is opened -- so this runs on the CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
USAGE = "ska markers [OPTIONS] --groups <FILE> -o <OUTPUT> <SKF_FILE>"
HINT = "\n\nFor more information, try '--help'.\n"
FLAGS = ["<SKF_FILE>", "--groups <FILE>", "-o <OUTPUT>", "--min-in <P>", "--max-out <Q>", "--min-group-size <N>", "--kind <KIND>", "--fasta",
         "[default: 1.0]", "[default: 0.0]", "[default: 1]", "[default: both]", "presence, allele, both", ".markers.tsv", ".markers.summary.tsv", ".markers.fa"]


def _run(*args):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=60)


def test_help_lists_every_flag():
    outs = set()
    for args in (("markers", "--help"), ("markers", "-h"), ("help", "markers"), ("markers", "x.skf", "--help")):
        r = _run(*args)
        assert r.returncode == 0 and r.stderr == "", (args, r.stderr)
        outs.add(r.stdout)
    assert len(outs) == 1
    out = outs.pop()
    assert out.split("\n")[2] == f"Usage: {USAGE}"
    for f in FLAGS + ["-v, --verbose", "-h, --help", "-V, --version"]:
        assert f in out, f
    assert "\n  markers " in _run("--help").stdout
    r = _run("markers", "--version")
    assert (r.returncode, r.stdout) == (0, "ska-markers 0.5.2\n")


def test_refusals_before_any_device():
    miss = "error: the following required arguments were not provided:\n  {}\n\nUsage: " + USAGE + HINT
    invalid = "error: invalid value '{}' for '{}': {}" + HINT
    prop = "Proportion must be between 0 and 1 (inclusive)"
    ok = ["markers", "x.skf", "--groups", "g.csv", "-o", "out"]
    cases = [
        (["markers"], miss.format("<SKF_FILE>")),
        (["markers", "x.skf", "-o", "out"], miss.format("--groups <FILE>")),
        (["markers", "x.skf", "--groups", "g.csv"], miss.format("-o <OUTPUT>")),
        (ok + ["--gpus", "2"], "error: the argument '--gpus <GPUS>' cannot be used with '--groups <FILE>'\n\nUsage: " + USAGE + HINT),
        (ok + ["--min-in", "1.5"], invalid.format("1.5", "--min-in <P>", prop)),
        (ok + ["--min-in", "-0.1"], invalid.format("-0.1", "--min-in <P>", prop)),
        (ok + ["--min-in", "nan"], invalid.format("nan", "--min-in <P>", prop)),
        (ok + ["--min-in", "half"], invalid.format("half", "--min-in <P>", "invalid float literal")),
        (ok + ["--max-out", "2"], invalid.format("2", "--max-out <Q>", prop)),
        (ok + ["--max-out", "-1e-9"], invalid.format("-1e-9", "--max-out <Q>", prop)),
        (ok + ["--max-out", "NaN"], invalid.format("NaN", "--max-out <Q>", prop)),
        (ok + ["--max-out", "0.1x"], invalid.format("0.1x", "--max-out <Q>", "invalid float literal")),
        (ok + ["--max-out", ""], invalid.format("", "--max-out <Q>", "cannot parse float from empty string")),
        (ok + ["--min-group-size", "0"], invalid.format("0", "--min-group-size <N>", "must be one or higher")),
        (ok + ["--min-group-size", "-3"], invalid.format("-3", "--min-group-size <N>", "invalid digit found in string")),
        (ok + ["--min-group-size", "two"], invalid.format("two", "--min-group-size <N>", "invalid digit found in string")),
        (ok + ["--kind", "snp"], "error: invalid value 'snp' for '--kind <KIND>'\n  [possible values: presence, allele, both]" + HINT),
        (ok + ["--kind", ""], "error: invalid value '' for '--kind <KIND>'\n  [possible values: presence, allele, both]" + HINT),
        (ok + ["y.skf"], "error: unexpected argument 'y.skf' found\n\nUsage: " + USAGE + HINT),
    ]
    for args, want in cases:
        r = _run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", want), (args, r.stderr)
    r = _run(*ok, "--min-freq", "0.5")
    assert r.returncode == 2 and r.stderr.startswith("error: unexpected argument '--min-freq' found\n") and "SKA:" not in r.stderr


def test_accepted_values_reach_the_banner():
    """the edge values that stand: the command goes on to its banner (and then fails on a box without a device or without the file)"""
    for extra in (["--min-in", "0", "--max-out", "1"], ["--min-in", "1.0", "--max-out", "0.0", "--kind", "allele", "--fasta", "--min-group-size", "+2"]):
        r = _run("markers", "/nonexistent/x.skf", "--groups", "/nonexistent/g.csv", "-o", "/nonexistent/out", *extra)
        assert r.returncode != 2 and r.stderr.startswith("SKA: Split K-mer Analysis"), (extra, r.stderr)
