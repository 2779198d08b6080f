"""`ska screen` on the command line, as far as it goes without a device: its help lists every flag, and what it refuses it refuses in clap's
wording with exit code 2, without the banner and before a device is opened -- so this runs on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
USAGE = "ska screen [OPTIONS] -o <OUTPUT> <SKF_FILE> <PANEL>"
HINT = "\n\nFor more information, try '--help'.\n"
FLAGS = ["<SKF_FILE>", "<PANEL>", "-o <OUTPUT>", "--min-cover <C>", "--min-identity <I>", "--matrix", "[default: 0.9]", "[default: 0]",
         ".screen.tsv", ".screen.summary.tsv", ".screen.matrix.tsv", "(MI355X engine)"]


def _run(*args):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=60)


def test_help_lists_every_flag():
    outs = set()
    for args in (("screen", "--help"), ("screen", "-h"), ("help", "screen"), ("screen", "x.skf", "--help")):
        r = _run(*args)
        assert r.returncode == 0 and r.stderr == "", (args, r.stderr)
        outs.add(r.stdout)
    assert len(outs) == 1
    out = outs.pop()
    assert out.split("\n")[2] == f"Usage: {USAGE}"
    for f in FLAGS + ["-v, --verbose", "-h, --help", "-V, --version"]:
        assert f in out, f
    top = _run("--help").stdout
    assert "\n  screen " in top and [l for l in top.splitlines() if l.startswith("  screen ")][0].split(None, 1)[1].startswith("(MI355X engine)")
    r = _run("screen", "--version")
    assert (r.returncode, r.stdout) == (0, "ska-screen 0.5.2\n")


def test_refusals_before_any_device():
    miss = "error: the following required arguments were not provided:\n  {}\n\nUsage: " + USAGE + HINT
    invalid = "error: invalid value '{}' for '{}': {}" + HINT
    conflict = "error: the argument '{}' cannot be used with '{}'\n\nUsage: " + USAGE + HINT
    prop = "Proportion must be between 0 and 1 (inclusive)"
    ok = ["screen", "x.skf", "panel.fa", "-o", "out"]
    cases = [
        (["screen"], miss.format("<SKF_FILE>\n  <PANEL>")),
        (["screen", "-o", "out"], miss.format("<SKF_FILE>\n  <PANEL>")),
        (["screen", "x.skf", "-o", "out"], miss.format("<PANEL>")),
        (["screen", "x.skf", "panel.fa"], miss.format("-o <OUTPUT>")),
        (ok + ["--gpus", "2"], conflict.format("--gpus <GPUS>", "<SKF_FILE>")),
        (["screen", "x.skf", "panel.fa", "-o", ""], invalid.format("", "-o <OUTPUT>", "a value is required")),
        (ok + ["--min-cover", "1.5"], invalid.format("1.5", "--min-cover <C>", prop)),
        (ok + ["--min-cover", "-0.1"], invalid.format("-0.1", "--min-cover <C>", prop)),
        (ok + ["--min-cover", "nan"], invalid.format("nan", "--min-cover <C>", prop)),
        (ok + ["--min-cover", "most"], invalid.format("most", "--min-cover <C>", "invalid float literal")),
        (ok + ["--min-cover", ""], invalid.format("", "--min-cover <C>", "cannot parse float from empty string")),
        (ok + ["--min-identity", "1.0001"], invalid.format("1.0001", "--min-identity <I>", prop)),
        (ok + ["--min-identity", "-1"], invalid.format("-1", "--min-identity <I>", prop)),
        (ok + ["--min-identity", "inf"], invalid.format("inf", "--min-identity <I>", prop)),
        (ok + ["--min-identity", "0x1"], invalid.format("0x1", "--min-identity <I>", "invalid float literal")),
        (ok + ["--min-identity", ""], invalid.format("", "--min-identity <I>", "cannot parse float from empty string")),
        (ok + ["second.fa"], "error: unexpected argument 'second.fa' found\n\nUsage: " + USAGE + HINT),
    ]
    for args, want in cases:
        r = _run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", want), (args, r.stderr)
    for stray in (["--groups", "g.csv"], ["--min-freq", "0.5"], ["--threads", "2"], ["--repeat-mask"]):
        r = _run(*ok, *stray)
        assert r.returncode == 2 and r.stderr.startswith(f"error: unexpected argument '{stray[0]}' found\n") and "SKA:" not in r.stderr


def test_accepted_values_reach_the_banner():
    """the edge values that stand: the command goes on to its banner (and then fails on a box without a device or without the file)"""
    for extra in (["--min-cover", "0", "--min-identity", "0"], ["--min-cover", "1", "--min-identity", "1", "--matrix"], ["--min-cover", "+0.5"],
                  ["--min-identity", "+0.5", "--matrix"], ["--min-cover", "1e-3", "--min-identity", "5E-1"]):
        r = _run("screen", "/nonexistent/x.skf", "/nonexistent/panel.fa", "-o", "/nonexistent/out", *extra)
        assert r.returncode != 2 and r.stderr.startswith("SKA: Split K-mer Analysis"), (extra, r.stderr)
