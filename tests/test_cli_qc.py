"""`ska qc` on the command line, as far as it goes without a device: its help lists every flag, and what it refuses it refuses in clap's
wording with exit code 2, without the banner, before a device is opened and without writing a file -- so this runs on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
USAGE = "ska qc [OPTIONS] -o <OUTPUT> <SKF_FILE>"
HINT = "\n\nFor more information, try '--help'.\n"
FLAGS = ["<SKF_FILE>", "-o <OUTPUT>", "--min-freq <MIN_FREQ>", "--mad <M>", "[default: 0.9]", "[default: 5]", ".qc.tsv", ".qc.summary.tsv", ".qc.flagged.txt",
         "ska delete -f", "(MI355X engine)"]


def _run(*args, cwd=None):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=60, cwd=cwd)


def test_help_lists_every_flag():
    outs = set()
    for args in (("qc", "--help"), ("qc", "-h"), ("help", "qc"), ("qc", "x.skf", "--help")):
        r = _run(*args)
        assert r.returncode == 0 and r.stderr == "", (args, r.stderr)
        outs.add(r.stdout)
    assert len(outs) == 1
    out = outs.pop()
    assert out.split("\n")[2] == f"Usage: {USAGE}"
    for f in FLAGS + ["-v, --verbose", "-h, --help", "-V, --version"]:
        assert f in out, f
    assert "\n  qc " in _run("--help").stdout
    r = _run("qc", "--version")
    assert (r.returncode, r.stdout) == (0, "ska-qc 0.5.2\n")


def test_refusals_before_any_device(tmp_path):
    miss = "error: the following required arguments were not provided:\n  {}\n\nUsage: " + USAGE + HINT
    invalid = "error: invalid value '{}' for '{}': {}" + HINT
    conflict = "error: the argument '{}' cannot be used with '{}'\n\nUsage: " + USAGE + HINT
    freq = "Frequency must be between 0 and 1 (inclusive)"
    mad = "must be zero or higher"
    ok = ["qc", "x.skf", "-o", "out"]
    cases = [
        (["qc"], miss.format("<SKF_FILE>")),
        (["qc", "x.skf"], miss.format("-o <OUTPUT>")),
        (["qc", "-o", "out"], miss.format("<SKF_FILE>")),
        (ok + ["y.skf"], "error: unexpected argument 'y.skf' found\n\nUsage: " + USAGE + HINT),
        (ok + ["--gpus", "2"], conflict.format("--gpus <GPUS>", "<SKF_FILE>")),
        (["qc", "x.skf", "-o", ""], invalid.format("", "-o <OUTPUT>", "a value is required")),
        (ok + ["--min-freq", "1.5"], invalid.format("1.5", "--min-freq <MIN_FREQ>", freq)),
        (ok + ["--min-freq", "-0.1"], invalid.format("-0.1", "--min-freq <MIN_FREQ>", freq)),
        (ok + ["--min-freq", "most"], invalid.format("most", "--min-freq <MIN_FREQ>", "`most` isn't a valid frequency")),
        (ok + ["--mad", "-1"], invalid.format("-1", "--mad <M>", mad)),
        (ok + ["--mad", "-0.5"], invalid.format("-0.5", "--mad <M>", mad)),
        (ok + ["--mad", "NaN"], invalid.format("NaN", "--mad <M>", mad)),
        (ok + ["--mad", "five"], invalid.format("five", "--mad <M>", "invalid float literal")),
        (ok + ["--mad", ""], invalid.format("", "--mad <M>", "cannot parse float from empty string")),
    ]
    for args, want in cases:
        r = _run(*args, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", want), (args, r.stderr)
    for stray in (["--groups", "g.csv"], ["--filter", "no-const"], ["--threads", "2"], ["--permutations", "3"], ["--frobnicate"]):
        r = _run(*ok, *stray, cwd=tmp_path)
        assert r.returncode == 2 and r.stderr.startswith(f"error: unexpected argument '{stray[0]}' found\n") and "SKA:" not in r.stderr, (stray, r.stderr)
    assert list(tmp_path.iterdir()) == []                               # nothing is written on a refusal


def test_accepted_values_reach_the_banner(tmp_path):
    """the edge values that stand: the command goes on to its banner (and then fails on a box without a device or without the file)"""
    for extra in (["--min-freq", "0", "--mad", "0"], ["--min-freq", "1", "--mad", "2.5"], ["--mad", "1e3"], []):
        r = _run("qc", "/nonexistent/x.skf", "-o", str(tmp_path / "out"), *extra)
        assert r.returncode != 2 and r.stderr.startswith("SKA: Split K-mer Analysis"), (extra, r.stderr)
    assert list(tmp_path.iterdir()) == []
