"""`ska mask` on the command line, as far as it goes without a device: its help lists every flag, and what it refuses it refuses in clap's
wording with exit code 2, without the banner and before a device is opened -- so this runs on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
USAGE = "ska mask [OPTIONS] -o <OUTPUT> <--regions <FILE>|--dense|--bed <FILE>> <REFERENCE> <SKF_FILE>"
HINT = "\n\nFor more information, try '--help'.\n"
FLAGS = ["<REFERENCE>", "<SKF_FILE>", "-o <OUTPUT>", "--regions <FILE>", "--dense", "--window <W>", "--min-snps <T>", "--bed <FILE>", "--summary <PREFIX>",
         "[default: 1000]", "[default: 5]", ".density.regions.tsv", ".mask.summary.tsv", "never overwritten", "0-based start, exclusive end", "1-based, inclusive",
         "(MI355X engine)"]


def _run(*args):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=60)


def test_help_lists_every_flag():
    outs = set()
    for args in (("mask", "--help"), ("mask", "-h"), ("help", "mask"), ("mask", "ref.fa", "--help")):
        r = _run(*args)
        assert r.returncode == 0 and r.stderr == "", (args, r.stderr)
        outs.add(r.stdout)
    assert len(outs) == 1
    out = outs.pop()
    assert out.split("\n")[2] == f"Usage: {USAGE}"
    for f in FLAGS + ["-v, --verbose", "-h, --help", "-V, --version"]:
        assert f in out, f
    assert out.count("a convention, not a calibration") == 2                  # --window and --min-snps, as `ska density` says it
    top = _run("--help").stdout
    assert "\n  mask " in top and [l for l in top.splitlines() if l.startswith("  mask ")][0].split(None, 1)[1].startswith("(MI355X engine)")
    assert "\n  density " in top                                              # (the command it completes is still listed)
    r = _run("mask", "--version")
    assert (r.returncode, r.stdout) == (0, "ska-mask 0.5.2\n")


def test_refusals_before_any_device():
    miss = "error: the following required arguments were not provided:\n  {}\n\nUsage: " + USAGE + HINT
    invalid = "error: invalid value '{}' for '{}': {}" + HINT
    conflict = "error: the argument '{}' cannot be used with '{}'\n\nUsage: " + USAGE + HINT
    window, snps = "must be between 1 and 2147483648 (inclusive)", "must be between 2 and 65535 (inclusive)"
    base = ["mask", "ref.fa", "x.skf", "-o", "out.skf"]
    ok = base + ["--dense"]
    cases = [
        (["mask"], miss.format("<REFERENCE>\n  <SKF_FILE>")),
        (["mask", "-o", "out.skf", "--dense"], miss.format("<REFERENCE>\n  <SKF_FILE>")),
        (["mask", "ref.fa", "-o", "out.skf", "--dense"], miss.format("<SKF_FILE>")),
        (["mask", "ref.fa", "x.skf", "--dense"], miss.format("-o <OUTPUT>")),
        (base, miss.format("<--regions <FILE>|--dense|--bed <FILE>>")),
        (base + ["--summary", "p"], miss.format("<--regions <FILE>|--dense|--bed <FILE>>")),
        (ok + ["--gpus", "2"], conflict.format("--gpus <GPUS>", "<SKF_FILE>")),
        (ok + ["--regions", "r.tsv"], conflict.format("--regions <FILE>", "--dense")),
        (base + ["--regions", "r.tsv", "--window", "500"], miss.format("--dense")),
        (base + ["--bed", "b.bed", "--min-snps", "3"], miss.format("--dense")),
        (["mask", "ref.fa", "x.skf", "-o", "", "--dense"], invalid.format("", "-o <OUTPUT>", "a value is required")),
        (base + ["--regions", ""], invalid.format("", "--regions <FILE>", "a value is required")),
        (ok + ["--bed", ""], invalid.format("", "--bed <FILE>", "a value is required")),
        (ok + ["--summary", ""], invalid.format("", "--summary <PREFIX>", "a value is required")),
        (ok + ["--window", "0"], invalid.format("0", "--window <W>", window)),
        (ok + ["--window", "2147483649"], invalid.format("2147483649", "--window <W>", window)),
        (ok + ["--window", "-5"], invalid.format("-5", "--window <W>", "invalid digit found in string")),
        (ok + ["--window", ""], invalid.format("", "--window <W>", "cannot parse integer from empty string")),
        (ok + ["--window", "99999999999999999999999"], invalid.format("99999999999999999999999", "--window <W>", "number too large to fit in target type")),
        (ok + ["--min-snps", "1"], invalid.format("1", "--min-snps <T>", snps)),
        (ok + ["--min-snps", "65536"], invalid.format("65536", "--min-snps <T>", snps)),
        (ok + ["--min-snps", "five"], invalid.format("five", "--min-snps <T>", "invalid digit found in string")),
        (ok + ["second.skf"], "error: unexpected argument 'second.skf' found\n\nUsage: " + USAGE + HINT),
    ]
    for args, want in cases:
        r = _run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", want), (args, r.stderr)
    for stray in (["--snps"], ["--masked-aln", "m.aln"], ["--min-freq", "0.5"], ["--threads", "2"], ["--reverse"], ["--repeat-mask"]):
        r = _run(*ok, *stray)
        assert r.returncode == 2 and r.stderr.startswith(f"error: unexpected argument '{stray[0]}' found\n") and "SKA:" not in r.stderr


def test_accepted_values_reach_the_banner():
    """the combinations that stand: the command goes on to its banner (and then fails on a box without a device or without the file)"""
    for extra in (["--dense"], ["--dense", "--window", "1", "--min-snps", "2"], ["--dense", "--window", "2147483648", "--min-snps", "65535", "--bed", "/nonexistent/b.bed"],
                  ["--regions", "/nonexistent/r.tsv"], ["--bed", "/nonexistent/b.bed"], ["--regions", "/nonexistent/r.tsv", "--bed", "/nonexistent/b.bed", "--summary", "/nonexistent/p"]):
        r = _run("mask", "/nonexistent/ref.fa", "/nonexistent/x.skf", "-o", "/nonexistent/out.skf", *extra)
        assert r.returncode != 2 and r.stderr.startswith("SKA: Split K-mer Analysis"), (extra, r.stderr)
