"""`ska lo` on the command line (cli.rs:395-425): its help, its place in the top-level help, and clap's refusals -- exit code 2,
clap's wording, no banner, no device touched -- so this runs on the CPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
pytestmark = pytest.mark.skipif(not os.path.exists(SKA), reason="ska executable not built")


def _run(*args):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=60)


def test_lo_help_lists_every_flag_and_default():
    outs = set()
    for args in (("lo", "--help"), ("lo", "-h"), ("help", "lo"), ("lo", "x.skf", "out", "--help")):
        r = _run(*args)
        assert r.returncode == 0 and r.stderr == "", (args, r.stderr)
        outs.add(r.stdout)
    assert len(outs) == 1
    out = outs.pop()
    assert out.startswith("Finds 'left out' SNPs and INDELs using a graph\n\nUsage: ska lo [OPTIONS] <INPUT_SKF> <OUTPUT>\n")
    for want in ("<INPUT_SKF>", "<OUTPUT>", "-r, --reference <REFERENCE>", "-m, --missing <MISSING>", "-d, --depth <DEPTH>",
                 "-n, --indel-kmers <INDEL_KMERS>", "--threads <THREADS>", "[default: 0.1]", "[default: 4]", "[default: 2]", "[default: 1]",
                 "\ninput:\n", "\noutput:\n", "\ngraph traversal:\n", "\nother:\n", "-v, --verbose"):
        assert want in out, want


def test_top_level_help_lists_lo():
    r = _run("--help")
    assert r.returncode == 0
    assert "\n  lo        Finds 'left out' SNPs and INDELs using a graph\n" in r.stdout


@pytest.mark.parametrize("args,message", [
    ((), "error: the following required arguments were not provided:\n  <INPUT_SKF>\n  <OUTPUT>\n"),
    (("in.skf",), "error: the following required arguments were not provided:\n  <OUTPUT>\n"),
    (("in.skf", "out", "-m", "abc"), "error: invalid value 'abc' for '--missing <MISSING>': invalid float literal\n"),
    (("in.skf", "out", "--missing", "0.x"), "error: invalid value '0.x' for '--missing <MISSING>': invalid float literal\n"),
    (("in.skf", "out", "-d", "1.5"), "error: invalid value '1.5' for '--depth <DEPTH>': invalid digit found in string\n"),
    (("in.skf", "out", "--depth", "-1"), "error: invalid value '-1' for '--depth <DEPTH>': invalid digit found in string\n"),
    (("in.skf", "out", "-n", "two"), "error: invalid value 'two' for '--indel-kmers <INDEL_KMERS>': invalid digit found in string\n"),
    (("in.skf", "out", "--threads", "0"), "error: invalid value '0' for '--threads <THREADS>': Threads must be one or higher\n"),
    (("in.skf", "out", "--min-freq", "0.5"), "error: unexpected argument '--min-freq' found\n"),
])
def test_lo_refusals_in_clap_wording(args, message):
    r = _run("lo", *args)
    assert r.returncode == 2, r.stderr
    assert r.stdout == ""
    assert r.stderr.startswith(message), r.stderr
    assert "SKA: Split K-mer Analysis" not in r.stderr
    assert "For more information, try '--help'." in r.stderr


def test_lo_accepts_rust_float_forms():
    # these parse as f32 in Rust, so clap lets them through: the command then fails later on the missing input file (not with exit 2)
    for v in ("0.1", ".5", "1e-1", "inf", "5."):
        r = _run("lo", os.path.join(ROOT, "does_not_exist.skf"), "out", "-m", v)
        assert "invalid value" not in r.stderr, (v, r.stderr)
