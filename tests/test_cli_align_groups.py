"""`ska align --groups / --min-group-size / --samples / --samples-file`: what is refused before a device is opened (exit code 2, clap's
wording, no banner), and skh_read_groups -- the groups file reader, which touches no device -- through skx_engine.read_groups.  Runs on
the CPU."""
import os
import subprocess

import pytest

import skx_engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
USAGE = "ska align [OPTIONS] <INPUT>..."
TAIL = "\n\nFor more information, try '--help'.\n"


def _run(*args, env=None):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=60, env=env)


def _conflict(x, y):
    return f"error: the argument '{x}' cannot be used with '{y}'\n\nUsage: {USAGE}{TAIL}"


def _missing(what):
    return f"error: the following required arguments were not provided:\n  {what}\n\nUsage: {USAGE}{TAIL}"


def _invalid(value, arg, why):
    return f"error: invalid value '{value}' for '{arg}': {why}{TAIL}"


@pytest.mark.skipif(not os.path.exists(SKA), reason="ska executable not built")
def test_refusals_before_any_device(tmp_path):
    empty = tmp_path / "empty.txt"
    empty.write_text("\n\n")
    cases = [
        (["align", "x.skf", "--groups", "g.csv"], _missing("-o <OUTPUT>")),
        (["align", "x.skf", "--groups", "g.csv", "-o", "p", "--samples", "a,b"], _conflict("--groups <FILE>", "--samples <NAMES>")),
        (["align", "x.skf", "--groups", "g.csv", "-o", "p", "--samples-file", "f"], _conflict("--groups <FILE>", "--samples-file <FILE>")),
        (["align", "x.skf", "--samples", "a", "--samples-file", "f"], _conflict("--samples <NAMES>", "--samples-file <FILE>")),
        (["align", "x.skf", "--min-group-size", "3"], _missing("--groups <FILE>")),
        (["align", "x.skf", "--groups", "g.csv", "-o", "p", "--min-group-size", "0"], _invalid("0", "--min-group-size <N>", "must be one or higher")),
        (["align", "x.skf", "--groups", "g.csv", "-o", "p", "--min-group-size", "two"], _invalid("two", "--min-group-size <N>", "invalid digit found in string")),
        (["align", "x.skf", "--groups", "g.csv", "-o", "p", "--min-group-size", "-1"], _invalid("-1", "--min-group-size <N>", "invalid digit found in string")),
        (["align", "x.skf", "--groups", "g.csv", "-o", "p", "--min-group-size", ""], _invalid("", "--min-group-size <N>", "cannot parse integer from empty string")),
        (["align", "a.fa", "b.fa", "--groups", "g.csv", "-o", "p", "--gpus", "2"], _conflict("--groups <FILE>", "--gpus <GPUS>")),
        (["align", "a.fa", "b.fa", "--groups", "g.csv", "-o", "p", "--min-group-size", "3", "--gpus", "2"], _conflict("--groups <FILE>", "--gpus <GPUS>")),
        (["align", "a.fa", "b.fa", "--samples", "a", "--gpus", "2"], _conflict("--samples <NAMES>", "--gpus <GPUS>")),
        (["align", "a.fa", "b.fa", "--samples-file", "f", "--gpus", "2"], _conflict("--samples-file <FILE>", "--gpus <GPUS>")),
        (["align", "x.skf", "--groups", "", "-o", "p"], _invalid("", "--groups <FILE>", "a value is required")),
        (["align", "x.skf", "--samples", ",,"], _invalid(",,", "--samples <NAMES>", "no sample names given")),
        (["align", "x.skf", "--samples-file", str(empty)], _invalid(str(empty), "--samples-file <FILE>", "no sample names given")),
    ]
    for args, want in cases:
        r = _run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", want), (args, r.stderr)
    # a rank of a sharded job (SKX_WORLD in the environment) is refused like --gpus
    r = _run("align", "a.fa", "b.fa", "--samples", "a", env=dict(os.environ, SKX_WORLD="2", SKX_RANK="0"))
    assert (r.returncode, r.stdout, r.stderr) == (2, "", _conflict("--samples <NAMES>", "--gpus <GPUS>"))
    # what was refused before is refused as before
    r = _run("align", "x.skf", "--bogus")
    assert r.returncode == 2 and r.stderr == f"error: unexpected argument '--bogus' found\n\nUsage: ska align [OPTIONS]{TAIL}"
    r = _run("distance", "x.skf", "--groups", "g.csv")
    assert r.returncode == 2 and r.stderr.startswith("error: unexpected argument '--groups' found\n")


@pytest.mark.skipif(not os.path.exists(SKA), reason="ska executable not built")
def test_help_names_the_new_options():
    out = _run("align", "--help").stdout
    for flag in ("--groups <FILE>", "--min-group-size <N>", "--samples <NAMES>", "--samples-file <FILE>"):
        line = [l for l in out.splitlines() if l.strip().startswith(flag)]
        assert line, flag
    assert out.count("(MI355X engine)") == 5 and "[default: 2]" in out          # --gpus and the four new ones


def test_read_groups_takes_clusters_csv_as_written(tmp_path):
    names = ["plain", "with,comma", 'with"quote', "line\nbreak", "cr\rinside", "tail"]
    labels = [0, 1, 0, 3, 1, 5]                                           # labels[i] = the lowest sample of i's cluster
    text = E.clusters_csv(names, labels)
    assert text.startswith("id,Cluster__autocolour\n") and '"with,comma"' in text and '"with""quote"' in text
    p = tmp_path / "x.clusters.csv"
    p.write_text(text, newline="")
    groups = E.read_groups(str(p))
    # clusters numbered from 1 by size descending (ties: lowest sample), rows by cluster then sample
    assert groups == [("1", ["plain", 'with"quote']), ("2", ["with,comma", "cr\rinside"]), ("3", ["line\nbreak"]), ("4", ["tail"])]
    assert sorted(n for _, g in groups for n in g) == sorted(names)


def test_read_groups_separators_line_ends_and_order(tmp_path):
    p = tmp_path / "g.tsv"
    p.write_bytes(b"b\tsecond\r\n\r\na\tfirst\r\nna,me\tsecond\r\n\nc\tfirst")      # tabs, CRLF, blank lines, no final line break
    assert E.read_groups(str(p)) == [("second", ["b", "na,me"]), ("first", ["a", "c"])]
    p.write_text("id,Cluster__autocolour\nx,7\ny,7\nid,Cluster__autocolour\n")    # the header is skipped where it comes first only
    assert E.read_groups(str(p)) == [("7", ["x", "y"]), ("Cluster__autocolour", ["id"])]
    p.write_text('x,7\n"q""1",8\n"tab\tin",7\n')                                 # no header; a quoted tab is no separator
    assert E.read_groups(str(p)) == [("7", ["x", "tab\tin"]), ("8", ['q"1'])]
    p.write_text("")
    assert E.read_groups(str(p)) == []


@pytest.mark.parametrize("text,line,why", [
    ("a,1\nb\n", 2, "two fields are required (sample name, group label), found 1"),
    ("a,1\n\nb,2,3\n", 3, "two fields are required (sample name, group label), found 3"),
    ("id,Cluster__autocolour\n,1\n", 2, "the sample name is empty"),
    ("a,1\r\nb,\r\n", 2, "the group label is empty"),
    ("a\tx/y\n", 1, "the group label cannot be part of a file name"),
    ("a,1\nb,.\n", 2, "the group label cannot be part of a file name"),
    ("a,1\nb,..\n", 2, "the group label cannot be part of a file name"),
    ("a,1\nb,l\0l\n", 2, "the group label cannot be part of a file name"),
    ('"multi\nline",1\nb,2\n"multi\nline",3\n', 4, 'sample "multi\nline" is listed twice (first on line 1)'),
    ("a,1\nb,2\nc,1\nb,1\n", 4, 'sample "b" is listed twice (first on line 2)'),
    ('a,1\n"open,2\nb,3\n', 2, "a quoted field is not closed"),
    ('"a"x,1\n', 1, "text follows a closing quote"),
], ids=["one-field", "three-fields", "empty-name", "empty-label", "slash", "dot", "dotdot", "nul", "twice-quoted", "twice", "open-quote", "after-quote"])
def test_read_groups_refusals_name_the_line(tmp_path, text, line, why):
    p = tmp_path / "bad.csv"
    p.write_bytes(text.encode())
    with pytest.raises(E.EngineError) as ei:
        E.read_groups(str(p))
    assert ei.value.code == E.EINVAL
    assert f"groups file {p}: line {line}: {why}" in str(ei.value), str(ei.value)


def test_read_groups_missing_file(tmp_path):
    with pytest.raises(E.EngineError) as ei:
        E.read_groups(str(tmp_path / "nothing.csv"))
    assert ei.value.code == E.EIO and "Unable to open groups file" in str(ei.value)
