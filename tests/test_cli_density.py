"""`ska density` on the command line, as far as it goes without a device: its help lists every flag and says that the defaults are a convention,
and what it refuses it refuses in clap's wording with exit code 2, without the banner and before a device is opened -- so this runs on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
USAGE = "ska density [OPTIONS] -o <OUTPUT> <REFERENCE> <SKF_FILE>"
HINT = "\n\nFor more information, try '--help'.\n"
FLAGS = ["<REFERENCE>", "<SKF_FILE>", "-o <OUTPUT>", "--window <W>", "--min-snps <T>", "--snps", "--masked-aln <FILE>", "[default: 1000]", "[default: 5]",
         ".density.regions.tsv", ".density.summary.tsv", ".density.bins.tsv", ".density.snps.tsv", "a convention, not a calibration", "(MI355X engine)"]


def _run(*args):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=60)


def test_help_lists_every_flag():
    outs = set()
    for args in (("density", "--help"), ("density", "-h"), ("help", "density"), ("density", "ref.fa", "--help")):
        r = _run(*args)
        assert r.returncode == 0 and r.stderr == "", (args, r.stderr)
        outs.add(r.stdout)
    assert len(outs) == 1
    out = outs.pop()
    assert out.split("\n")[2] == f"Usage: {USAGE}"
    for f in FLAGS + ["-v, --verbose", "-h, --help", "-V, --version"]:
        assert f in out, f
    assert out.count("a convention, not a calibration") == 2                  # --window and --min-snps
    top = _run("--help").stdout
    assert "\n  density " in top and [l for l in top.splitlines() if l.startswith("  density ")][0].split(None, 1)[1].startswith("(MI355X engine)")
    r = _run("density", "--version")
    assert (r.returncode, r.stdout) == (0, "ska-density 0.5.2\n")


def test_refusals_before_any_device():
    miss = "error: the following required arguments were not provided:\n  {}\n\nUsage: " + USAGE + HINT
    invalid = "error: invalid value '{}' for '{}': {}" + HINT
    conflict = "error: the argument '{}' cannot be used with '{}'\n\nUsage: " + USAGE + HINT
    window, snps = "must be between 1 and 2147483648 (inclusive)", "must be between 2 and 65535 (inclusive)"
    ok = ["density", "ref.fa", "x.skf", "-o", "out"]
    cases = [
        (["density"], miss.format("<REFERENCE>\n  <SKF_FILE>")),
        (["density", "-o", "out"], miss.format("<REFERENCE>\n  <SKF_FILE>")),
        (["density", "ref.fa", "-o", "out"], miss.format("<SKF_FILE>")),
        (["density", "ref.fa", "x.skf"], miss.format("-o <OUTPUT>")),
        (ok + ["--gpus", "2"], conflict.format("--gpus <GPUS>", "<SKF_FILE>")),
        (["density", "ref.fa", "x.skf", "-o", ""], invalid.format("", "-o <OUTPUT>", "a value is required")),
        (ok + ["--masked-aln", ""], invalid.format("", "--masked-aln <FILE>", "a value is required")),
        (ok + ["--window", "0"], invalid.format("0", "--window <W>", window)),
        (ok + ["--window", "2147483649"], invalid.format("2147483649", "--window <W>", window)),
        (ok + ["--window", "-5"], invalid.format("-5", "--window <W>", "invalid digit found in string")),
        (ok + ["--window", "1e3"], invalid.format("1e3", "--window <W>", "invalid digit found in string")),
        (ok + ["--window", ""], invalid.format("", "--window <W>", "cannot parse integer from empty string")),
        (ok + ["--window", "99999999999999999999999"], invalid.format("99999999999999999999999", "--window <W>", "number too large to fit in target type")),
        (ok + ["--min-snps", "1"], invalid.format("1", "--min-snps <T>", snps)),
        (ok + ["--min-snps", "0"], invalid.format("0", "--min-snps <T>", snps)),
        (ok + ["--min-snps", "65536"], invalid.format("65536", "--min-snps <T>", snps)),
        (ok + ["--min-snps", "five"], invalid.format("five", "--min-snps <T>", "invalid digit found in string")),
        (ok + ["--min-snps", ""], invalid.format("", "--min-snps <T>", "cannot parse integer from empty string")),
        (ok + ["second.skf"], "error: unexpected argument 'second.skf' found\n\nUsage: " + USAGE + HINT),
    ]
    for args, want in cases:
        r = _run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", want), (args, r.stderr)
    for stray in (["--groups", "g.csv"], ["--min-freq", "0.5"], ["--threads", "2"], ["--repeat-mask"], ["--max-snps", "3"]):
        r = _run(*ok, *stray)
        assert r.returncode == 2 and r.stderr.startswith(f"error: unexpected argument '{stray[0]}' found\n") and "SKA:" not in r.stderr


def test_accepted_values_reach_the_banner():
    """the edge values that stand: the command goes on to its banner (and then fails on a box without a device or without the file)"""
    for extra in (["--window", "1", "--min-snps", "2"], ["--window", "2147483648", "--min-snps", "65535", "--snps"], ["--window", "+500"],
                  ["--snps", "--masked-aln", "/nonexistent/masked.aln"]):
        r = _run("density", "/nonexistent/ref.fa", "/nonexistent/x.skf", "-o", "/nonexistent/out", *extra)
        assert r.returncode != 2 and r.stderr.startswith("SKA: Split K-mer Analysis"), (extra, r.stderr)
