"""`ska distance (--max-snps | --max-mismatches | --closest | --mst) --sites PREFIX [--sites-max N]` at the command line: the refusals and the help
need no device and run everywhere; with one, PREFIX.sites.tsv is the model's (tests/sites_model.py) on the array the engine loads, and the
table's lines are those without --sites."""
import os
import subprocess

import numpy as np
import pytest

import sites_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
GOLD = os.path.join(ROOT, "tests", "golden")
HINT = "\n\nFor more information, try '--help'.\n"
USAGE = "\n\nUsage: ska distance [OPTIONS] <SKF_FILE>"


def _ska(*args, cwd, ok=True):
    r = subprocess.run([SKA, *[str(a) for a in args]], cwd=cwd, capture_output=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-1500:].decode(errors="replace")
    return r


def _fin(name):
    return os.path.join(GOLD, "input", name)


def _refused(r, message, cwd):
    assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", message), r.stderr
    assert sorted(os.listdir(cwd)) == ["q.txt"]                                            # no file created


@pytest.fixture
def wd(tmp_path):
    (tmp_path / "q.txt").write_text("a\n")
    return str(tmp_path)


# ---------------------------------------------------------------------------------------------- no device needed
SELECTING = [["--max-snps", "5"], ["--max-mismatches", "0.5"], ["--closest", "2"], ["--mst"]]
OTHERS = [(["--allow-ambiguous"], "--allow-ambiguous"), (["--no-table"], "--no-table"), (["--query", "a"], "--query <NAMES>"),
          (["--query-file", "q.txt"], "--query-file <FILE>"), (["--query-skf", "b.skf"], "--query-skf <FILE>"), (["--gpus", "2"], "--gpus <GPUS>")]


def test_help_lists_the_two_options_after_no_table():
    out = _ska("distance", "--help", cwd=ROOT).stdout.decode()
    lines = out.splitlines()
    at = [n for n, ln in enumerate(lines) if ln.lstrip().startswith("--no-table  ")]
    assert len(at) == 1
    for n, head in enumerate(("--sites <PREFIX>  ", "--sites-max <N>  ")):
        ln = lines[at[0] + 1 + n].lstrip()
        assert ln.startswith(head) and "(MI355X engine)" in ln, ln
    assert lines[at[0] + 3].lstrip().startswith("--query <NAMES>")
    assert "<PREFIX>.sites.tsv" in lines[at[0] + 1] and "[default: 134217728]" in lines[at[0] + 2] and 134217728 == 1 << 27


@pytest.mark.parametrize("other, oarg", OTHERS, ids=[o[1].split()[0] for o in OTHERS])
def test_the_sites_refuse_what_has_no_selected_lines_of_one_device(wd, other, oarg):
    for sel in SELECTING:
        for args in ([*sel, "--sites", "p", *other], [*other, "--sites", "p", *sel], ["--sites", "p", "--sites-max", "10", *other, *sel]):
            r = _ska("distance", "x.skf", *args, cwd=wd, ok=False)
            _refused(r, f"error: the argument '--sites <PREFIX>' cannot be used with '{oarg}'" + USAGE + HINT, wd)


def test_the_sites_need_a_selection_and_the_limit_needs_the_sites(wd):
    missing = "error: the following required arguments were not provided:\n  {}" + USAGE + HINT
    for args in (["--sites", "p"], ["--sites", "p", "--sites-max", "10"], ["--sites-max", "10", "--sites", "p", "-o", "t.tsv"], ["--sites", "p", "--tree", "t.nwk"]):
        r = _ska("distance", "x.skf", *args, cwd=wd, ok=False)
        _refused(r, missing.format("<--max-snps <N>|--max-mismatches <P>|--closest <K>|--mst>"), wd)
    for sel in ([], *SELECTING):
        for args in ([*sel, "--sites-max", "10"], ["--sites-max", "10", *sel]):
            r = _ska("distance", "x.skf", *args, cwd=wd, ok=False)
            _refused(r, missing.format("--sites <PREFIX>"), wd)


BAD_MAX = [("", "cannot parse integer from empty string"), ("ten", "invalid digit found in string"), ("1e6", "invalid digit found in string"),
           ("-5", "invalid digit found in string"), ("1.5", "invalid digit found in string"), ("0", "must be one or higher"),
           ("99999999999999999999", "number too large to fit in target type")]


@pytest.mark.parametrize("value, why", BAD_MAX, ids=[b[0] or "empty" for b in BAD_MAX])
def test_bad_values(wd, value, why):
    for args in (["--max-snps", "5", "--sites", "p", "--sites-max", value], ["--sites-max", value, "--sites", "p", "--mst"]):
        r = _ska("distance", "x.skf", *args, cwd=wd, ok=False)
        _refused(r, f"error: invalid value '{value}' for '--sites-max <N>': {why}" + HINT, wd)
    for args in (["--max-snps", "5", "--sites", ""], ["--sites", "", "--closest", "1"]):
        r = _ska("distance", "x.skf", *args, cwd=wd, ok=False)
        _refused(r, "error: invalid value '' for '--sites <PREFIX>': a value is required" + HINT, wd)


def test_the_ladder_is_cut_from_another_load(wd):
    for args in (["--mst", "--mst-clusters", "lad", "--sites", "p"], ["--sites", "p", "--mst-clusters", "lad", "--mst"]):
        r = _ska("distance", "x.skf", *args, cwd=wd, ok=False)
        _refused(r, "error: the argument '--sites <PREFIX>' cannot be used with '--mst-clusters <PREFIX>'" + USAGE + HINT, wd)


@pytest.mark.parametrize("args", (["--sites", "p"], ["--sites-max", "3"]), ids=lambda a: a[0])
def test_other_subcommands_refuse_the_options(wd, args):
    r = _ska("align", "x.skf", *args, cwd=wd, ok=False)
    _refused(r, f"error: unexpected argument '{args[0]}' found\n\nUsage: ska align [OPTIONS]" + HINT, wd)


def test_accepted_values_reach_the_banner(wd):
    """what stands goes on to the banner (and then fails on a box without a device, or for want of the file)"""
    for args in (["--max-snps", "5", "--sites", "p"], ["--sites", "p", "--mst", "--max-mismatches", "0.5", "--sites-max", "+7"],
                 ["--closest", "1", "--sites", "p", "--sites-max", "18446744073709551615", "-o", "t.tsv", "--min-freq", "0.5"]):
        r = _ska("distance", _fin("multidist.skf"), *args, cwd=wd, ok=False)
        assert r.returncode != 2 and r.stderr.decode().startswith("SKA: Split K-mer Analysis"), (args, r.stderr)


# ---------------------------------------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def _loaded(E, skf):
    """the array as the command loads it -- a file's rows in the file's order, which the oracle's load keeps: names, k, the rows' split k-mers, the
    matrix, the rows' counts"""
    import ora
    oa = ora.Array.load(_fin(skf))
    keys, var, counts = oa.export()
    arr = E.Array.load(_fin(skf))
    assert arr.names == oa.names and arr.nrows == len(var)
    rec, rkeys, _ = arr.pair_sites(SM.all_pairs(len(oa.names)), keys=True)
    assert len(rec) and np.array_equal(rkeys, keys[rec["row"].astype(np.int64)]), "a record's row is not the file's row"
    return oa.names, oa.k, keys, var, counts


def _pairs_of(names, table):
    return [(names.index(f[0]), names.index(f[1])) for f in (ln.split("\t") for ln in table.splitlines()[1:])]


def _model_text(loaded, table, min_freq=0.0):
    names, k, keys, var, counts = loaded
    pairs = _pairs_of(names, table)
    recs = SM.sites(var, SM.sweep_flags(var, min_freq, counts), pairs)
    # the model's own link to the table: a line's Distance is its number of sites
    assert [float(n) for n in SM.counts_of(recs, len(pairs))] == [float(ln.split("\t")[2]) for ln in table.splitlines()[1:]]
    return SM.sites_text(names, keys, k, pairs, recs), len(recs)


RUNS = [("multidist.skf", ["--max-snps", "5"], 0.0), ("multidist.skf", ["--max-mismatches", "0.6"], 0.0), ("multidist.skf", ["--max-snps", "5", "--min-freq", "0.5"], 0.5),
        ("merge_k41.skf", ["--max-snps", "1000"], 0.0), ("multidist.skf", ["--mst"], 0.0), ("multidist.skf", ["--closest", "1"], 0.0),
        ("multidist.skf", ["--mst", "--max-mismatches", "0.6"], 0.0), ("multidist.skf", ["--closest", "1", "--max-snps", "1"], 0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("skf, flags, min_freq", RUNS, ids=[r[0].split(".")[0] + " " + " ".join(r[1]) for r in RUNS])
def test_the_file_is_the_models_and_the_table_is_unchanged(E, tmp_path, skf, flags, min_freq):
    wd = str(tmp_path)
    plain = _ska("distance", _fin(skf), *flags, cwd=wd).stdout.decode()
    r = _ska("distance", _fin(skf), *flags, "--sites", "p", cwd=wd)
    assert r.stdout.decode() == plain                                                      # byte for byte the output without --sites
    assert sorted(os.listdir(wd)) == ["p.sites.tsv"]
    want, n = _model_text(_loaded(E, skf), plain, min_freq)
    assert open(os.path.join(wd, "p.sites.tsv")).read() == want                            # the sites of exactly the printed lines, in their order
    if flags in (["--max-snps", "5"], ["--max-snps", "1000"], ["--max-mismatches", "0.6"]):
        assert n > 0, "a run that lists nothing shows nothing"
    r = _ska("distance", _fin(skf), *flags, "--sites", "p", "-o", "t.tsv", cwd=wd)
    assert r.stdout == b"" and open(os.path.join(wd, "t.tsv")).read() == plain and open(os.path.join(wd, "p.sites.tsv")).read() == want


@pytest.mark.gpu
def test_the_limit_refuses_after_the_table(E, tmp_path):
    wd, src = str(tmp_path), _fin("multidist.skf")
    plain = _ska("distance", src, "--max-snps", "5", cwd=wd).stdout.decode()
    want, n = _model_text(_loaded(E, "multidist.skf"), plain)
    assert n > 1
    r = _ska("distance", src, "--max-snps", "5", "--sites", "p", "--sites-max", n, "-v", cwd=wd)
    assert r.stdout.decode() == plain and open(os.path.join(wd, "p.sites.tsv")).read() == want
    assert f"Sites: {n} records of {len(plain.splitlines()) - 1} lines".encode() in r.stderr
    os.remove(os.path.join(wd, "p.sites.tsv"))
    r = _ska("distance", src, "--max-snps", "5", "--sites", "p", "--sites-max", n - 1, cwd=wd, ok=False)
    assert r.returncode == 101 and r.stdout.decode() == plain                              # the table's lines were written first
    assert r.stderr.decode().endswith(f"error: pair sites: {n} records; the limit is {n - 1}\n")
    assert os.listdir(wd) == []
    r = _ska("distance", src, "--max-snps", "5", "--sites", "p", "--sites-max", n - 1, "-o", "t.tsv", cwd=wd, ok=False)
    assert r.returncode == 101 and r.stdout == b"" and open(os.path.join(wd, "t.tsv")).read() == plain and os.listdir(wd) == ["t.tsv"]
