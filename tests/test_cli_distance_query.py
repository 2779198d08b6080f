"""`ska distance --query / --query-file / --query-skf` (the executable).  The output is defined from the full table: the header, then exactly
the lines of `ska distance` (same other flags) that name a query sample, in the table's order and text -- so the goldens of the full table
are the reference here.  The refusals and the help need no device and run everywhere."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
GOLD = os.path.join(ROOT, "tests", "golden")
HINT = "\n\nFor more information, try '--help'.\n"


def _ska(*args, cwd, ok=True):
    r = subprocess.run([SKA, *args], cwd=cwd, capture_output=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-1500:].decode(errors="replace")
    return r


def _fin(name):
    return os.path.join(GOLD, "input", name)


def _golden(name):
    return open(os.path.join(GOLD, "correct", name), "rb").read()


def _restrict(table, queries):
    """the header and the lines of a full table in which Sample1 or Sample2 is a query"""
    lines = table.decode().splitlines(keepends=True)
    qs = set(queries)
    return "".join([lines[0]] + [ln for ln in lines[1:] if ln.split("\t")[0] in qs or ln.split("\t")[1] in qs]).encode()


def _names(table):
    seen = []
    for ln in table.decode().splitlines()[1:]:
        for n in ln.split("\t")[:2]:
            if n not in seen:
                seen.append(n)
    return seen


# ---------------------------------------------------------------------------------------------- no device needed
QUERY_OPTS = [("--query", "--query <NAMES>", "a"), ("--query-file", "--query-file <FILE>", "q.txt"), ("--query-skf", "--query-skf <FILE>", "b.skf")]


@pytest.mark.parametrize("flag, arg, value", QUERY_OPTS)
def test_query_refuses_what_needs_the_whole_table(tmp_path, flag, arg, value):
    (tmp_path / "q.txt").write_text("a\n")
    conflict = "error: the argument '{}' cannot be used with '{}'\n\nUsage: ska distance [OPTIONS] <SKF_FILE>" + HINT
    for other, oarg in ((["--tree", "t.nwk"], "--tree <FILE>"), (["--clusters", "c"], "--clusters <PREFIX>"), (["--gpus", "2"], "--gpus <GPUS>")):
        r = _ska("distance", "x.skf", flag, value, *other, cwd=str(tmp_path), ok=False)
        assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", conflict.format(arg, oarg)), (flag, other, r.stderr)
    assert not os.path.exists(tmp_path / "t.nwk")


def test_empty_query_and_missing_query_file(tmp_path):
    wd = str(tmp_path)
    r = _ska("distance", "x.skf", "--query", "", cwd=wd, ok=False)
    assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", "error: invalid value '' for '--query <NAMES>': a value is required" + HINT)
    r = _ska("distance", "x.skf", "--query", ",,", cwd=wd, ok=False)
    assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", "error: invalid value ',,' for '--query <NAMES>': no sample names given" + HINT)
    r = _ska("distance", "x.skf", "--query-file", "nothing_here.txt", cwd=wd, ok=False)
    assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", "error: Unable to open file_list\n")
    (tmp_path / "blank.txt").write_text("\n\n")
    r = _ska("distance", "x.skf", "--query-file", "blank.txt", cwd=wd, ok=False)
    assert (r.returncode, r.stdout) == (2, b"") and "no sample names given" in r.stderr.decode()
    # the options belong to `ska distance` alone
    r = _ska("align", "x.skf", "--query", "a", cwd=wd, ok=False)
    assert (r.returncode, r.stderr.decode()) == (2, "error: unexpected argument '--query' found\n\nUsage: ska align [OPTIONS]" + HINT)


def test_help_lists_the_query_options():
    out = _ska("distance", "--help", cwd=ROOT).stdout.decode()
    for f in ("--query <NAMES>", "--query-file <FILE>", "--query-skf <FILE>"):
        assert f in out, f
    assert "Usage: ska distance [OPTIONS] <SKF_FILE>" in out
    assert out.index("--cluster-mismatches <P>") < out.index("--query <NAMES>") < out.index("-v, --verbose")


# ---------------------------------------------------------------------------------------------- goldens
MULTIDIST = [("multidist.stdout", []), ("multidist.minfreq.stdout", ["--min-freq", "0.9"]), ("multidist.ambig.stdout", ["--allow-ambiguous"])]


@pytest.mark.gpu
@pytest.mark.parametrize("golden, flags", MULTIDIST, ids=[g for g, _ in MULTIDIST])
def test_multidist_goldens(tmp_path, golden, flags):
    wd, src, table = str(tmp_path), _fin("multidist.skf"), _golden(golden)
    names = _names(table)
    assert len(names) == 6
    for query in [[n] for n in names] + [[names[0], names[-1]], names]:
        want = _restrict(table, query)
        rest = 6 - len(query)
        assert len(want.splitlines()) == 1 + 15 - rest * (rest - 1) // 2                 # every pair but those of two other samples
        r = _ska("distance", src, "--query", ",".join(query), *flags, cwd=wd)
        assert r.stdout == want, query
    # -o, --query-file (a blank line in it), and the union of the two options with a repeat
    query = [names[4], names[1]]
    want = _restrict(table, query)
    (tmp_path / "q.txt").write_text(f"{names[4]}\n\n{names[1]}\n")
    r = _ska("distance", src, "--query-file", "q.txt", "-o", "out.tsv", *flags, cwd=wd)
    assert r.stdout == b"" and open(os.path.join(wd, "out.tsv"), "rb").read() == want
    r = _ska("distance", src, "--query", ",".join(query), "-o", "out2.tsv", *flags, cwd=wd)
    assert r.stdout == b"" and open(os.path.join(wd, "out2.tsv"), "rb").read() == want
    r = _ska("distance", src, "--query-file", "q.txt", "--query", f"{names[4]},{names[2]}", *flags, cwd=wd)
    assert r.stdout == _restrict(table, query + [names[2]])
    assert want != table and _restrict(table, names) == table


@pytest.mark.gpu
def test_wide_keys_golden(tmp_path):
    table = _golden("merge_k41.dist.stdout")
    names = _names(table)
    for query in [[n] for n in names] + [names]:
        assert _ska("distance", _fin("merge_k41.skf"), "--query", ",".join(query), cwd=str(tmp_path)).stdout == _restrict(table, query)


# ---------------------------------------------------------------------------------------------- --query-skf
@pytest.mark.gpu
def test_query_skf_of_two_built_files(tmp_path):
    wd = str(tmp_path)
    _ska("build", "-k", "17", "-o", "one", _fin("test_1.fa"), cwd=wd)
    _ska("build", "-k", "17", "-o", "two", _fin("test_2.fa"), cwd=wd)
    r = _ska("distance", "one.skf", "--query-skf", "two.skf", cwd=wd)
    assert r.stdout == _golden("merge.dist.stdout")
    assert not [f for f in os.listdir(wd) if f not in ("one.skf", "two.skf")]          # the merge happens in memory
    # a file of another k: `ska merge`'s refusal, message and status
    _ska("build", "-k", "21", "-o", "other", _fin("test_2.fa"), cwd=wd)
    m = _ska("merge", "one.skf", "other.skf", "-o", "never", cwd=wd, ok=False)
    q = _ska("distance", "one.skf", "--query-skf", "other.skf", cwd=wd, ok=False)
    assert m.returncode != 0 and q.returncode == m.returncode and q.stdout == b""
    err = [ln for ln in m.stderr.decode().splitlines() if ln.startswith("error:")]
    assert err and err == [ln for ln in q.stderr.decode().splitlines() if ln.startswith("error:")]


@pytest.mark.gpu
@pytest.mark.parametrize("golden, flags", MULTIDIST, ids=[g for g, _ in MULTIDIST])
def test_query_skf_of_a_split_array(tmp_path, golden, flags):
    wd, src, table = str(tmp_path), _fin("multidist.skf"), _golden(golden)
    names = _names(table)
    assert _ska("distance", src, *flags, cwd=wd).stdout == table
    two = [names[1], names[4]]
    _ska("delete", "-s", src, "-o", "four", *two, cwd=wd)
    _ska("delete", "-s", src, "-o", "two", *[n for n in names if n not in two], cwd=wd)
    _ska("merge", "four.skf", "two.skf", "-o", "merged", cwd=wd)
    full = _ska("distance", "merged.skf", *flags, cwd=wd).stdout
    assert _names(full) == [n for n in names if n not in two] + two
    r = _ska("distance", "four.skf", "--query-skf", "two.skf", *flags, cwd=wd)
    assert r.stdout == _restrict(full, two) and len(r.stdout.splitlines()) == 1 + 4 * 2 + 1
    # with a named sample of the first file on top
    r = _ska("distance", "four.skf", "--query-skf", "two.skf", "--query", names[0], *flags, cwd=wd)
    assert r.stdout == _restrict(full, two + [names[0]])


# ---------------------------------------------------------------------------------------------- errors
@pytest.mark.gpu
def test_unknown_name(tmp_path):
    table = _golden("multidist.stdout")
    r = _ska("distance", _fin("multidist.skf"), "--query", f"{_names(table)[0]},no_such_sample", cwd=str(tmp_path), ok=False)
    d = _ska("delete", "-s", _fin("multidist.skf"), "-o", "d", "no_such_sample", cwd=str(tmp_path), ok=False)
    assert r.returncode == d.returncode != 0 and r.stdout == b""
    assert 'Could not find sample(s): {"no_such_sample"}' in r.stderr.decode()
