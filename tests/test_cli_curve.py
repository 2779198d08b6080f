"""`ska curve` on the command line, as far as it goes without a device: its help lists every flag, and what it refuses it refuses in clap's
wording with exit code 2, without the banner and before a device is opened -- so this runs on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
USAGE = "ska curve [OPTIONS] -o <OUTPUT> <SKF_FILE>"
HINT = "\n\nFor more information, try '--help'.\n"
FLAGS = ["<SKF_FILE>", "-o <OUTPUT>", "--permutations <P>", "--seed <N>", "--min-freq <MIN_FREQ>", "--order-file <FILE>", "--all-permutations",
         "[default: 20]", "[default: 1]", "[default: 0.9]", "1 to 10000", ".curve.tsv", ".curve.permutations.tsv"]


def _run(*args):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=60)


def test_help_lists_every_flag():
    outs = set()
    for args in (("curve", "--help"), ("curve", "-h"), ("help", "curve"), ("curve", "x.skf", "--help")):
        r = _run(*args)
        assert r.returncode == 0 and r.stderr == "", (args, r.stderr)
        outs.add(r.stdout)
    assert len(outs) == 1
    out = outs.pop()
    assert out.split("\n")[2] == f"Usage: {USAGE}"
    for f in FLAGS + ["-v, --verbose", "-h, --help", "-V, --version"]:
        assert f in out, f
    assert "\n  curve " in _run("--help").stdout
    r = _run("curve", "--version")
    assert (r.returncode, r.stdout) == (0, "ska-curve 0.5.2\n")


def test_refusals_before_any_device():
    miss = "error: the following required arguments were not provided:\n  {}\n\nUsage: " + USAGE + HINT
    invalid = "error: invalid value '{}' for '{}': {}" + HINT
    conflict = "error: the argument '{}' cannot be used with '{}'\n\nUsage: " + USAGE + HINT
    perms = "must be between 1 and 10000 (inclusive)"
    freq = "Frequency must be between 0 and 1 (inclusive)"
    ok = ["curve", "x.skf", "-o", "out"]
    cases = [
        (["curve"], miss.format("<SKF_FILE>")),
        (["curve", "x.skf"], miss.format("-o <OUTPUT>")),
        (ok + ["--gpus", "2"], conflict.format("--gpus <GPUS>", "<SKF_FILE>")),
        (ok + ["--order-file", "o.txt", "--permutations", "5"], conflict.format("--order-file <FILE>", "--permutations <P>")),
        (ok + ["--seed", "3", "--order-file", "o.txt"], conflict.format("--order-file <FILE>", "--seed <N>")),
        (ok + ["--order-file", ""], invalid.format("", "--order-file <FILE>", "a value is required")),
        (ok + ["--permutations", "0"], invalid.format("0", "--permutations <P>", perms)),
        (ok + ["--permutations", "10001"], invalid.format("10001", "--permutations <P>", perms)),
        (ok + ["--permutations", "-1"], invalid.format("-1", "--permutations <P>", "invalid digit found in string")),
        (ok + ["--permutations", "ten"], invalid.format("ten", "--permutations <P>", "invalid digit found in string")),
        (ok + ["--permutations", ""], invalid.format("", "--permutations <P>", "cannot parse integer from empty string")),
        (ok + ["--permutations", "99999999999999999999999"], invalid.format("99999999999999999999999", "--permutations <P>", "number too large to fit in target type")),
        (ok + ["--seed", "-5"], invalid.format("-5", "--seed <N>", "invalid digit found in string")),
        (ok + ["--seed", "1.5"], invalid.format("1.5", "--seed <N>", "invalid digit found in string")),
        (ok + ["--seed", "18446744073709551616"], invalid.format("18446744073709551616", "--seed <N>", "number too large to fit in target type")),
        (ok + ["--min-freq", "1.5"], invalid.format("1.5", "--min-freq <MIN_FREQ>", freq)),
        (ok + ["--min-freq", "-0.1"], invalid.format("-0.1", "--min-freq <MIN_FREQ>", freq)),
        (ok + ["--min-freq", "most"], invalid.format("most", "--min-freq <MIN_FREQ>", "`most` isn't a valid frequency")),
        (ok + ["y.skf"], "error: unexpected argument 'y.skf' found\n\nUsage: " + USAGE + HINT),
    ]
    for args, want in cases:
        r = _run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", want), (args, r.stderr)
    for stray in (["--groups", "g.csv"], ["--filter", "no-const"], ["--threads", "2"]):
        r = _run(*ok, *stray)
        assert r.returncode == 2 and r.stderr.startswith(f"error: unexpected argument '{stray[0]}' found\n") and "SKA:" not in r.stderr


def test_accepted_values_reach_the_banner():
    """the edge values that stand: the command goes on to its banner (and then fails on a box without a device or without the file)"""
    for extra in (["--permutations", "1", "--seed", "0", "--min-freq", "0"], ["--permutations", "10000", "--seed", "18446744073709551615", "--min-freq", "1", "--all-permutations"],
                  ["--order-file", "/nonexistent/order.txt", "--all-permutations"], ["--permutations", "+3"]):
        r = _run("curve", "/nonexistent/x.skf", "-o", "/nonexistent/out", *extra)
        assert r.returncode != 2 and r.stderr.startswith("SKA: Split K-mer Analysis"), (extra, r.stderr)
