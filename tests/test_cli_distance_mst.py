"""`ska distance --mst [--mst-clusters PREFIX [--levels ...]]` at the command line: the lines of the table's minimum spanning forest as the
model (tests/mst_model.py) picks them from the golden tables' text, and the ladder's CSV.  The refusals and the help need no device and
run everywhere."""
import os
import subprocess

import pytest

from mst_model import levels, mst, mst_text
from select_model import table_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
GOLD = os.path.join(ROOT, "tests", "golden")
HINT = "\n\nFor more information, try '--help'.\n"
USAGE = "\n\nUsage: ska distance [OPTIONS] <SKF_FILE>"


def _ska(*args, cwd, ok=True):
    r = subprocess.run([SKA, *args], cwd=cwd, capture_output=True, timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-1500:].decode(errors="replace")
    return r


def _fin(name):
    return os.path.join(GOLD, "input", name)


def _golden(name):
    return open(os.path.join(GOLD, "correct", name)).read()


def _refused(r, message, cwd):
    assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", message), r.stderr
    assert sorted(os.listdir(cwd)) == ["q.txt"]                                            # no file created


# ---------------------------------------------------------------------------------------------- no device needed
MST_OPTS = [("--mst", ""), ("--mst-clusters", "<PREFIX>"), ("--levels", "<L1,L2,...>")]
OTHERS = [(["--tree", "t.nwk"], "--tree <FILE>"), (["--clusters", "c"], "--clusters <PREFIX>"), (["--cluster-snps", "3"], "--cluster-snps <N>"),
          (["--cluster-mismatches", "0.5"], "--cluster-mismatches <P>"), (["--no-table"], "--no-table"), (["--gpus", "2"], "--gpus <GPUS>"),
          (["--query", "a"], "--query <NAMES>"), (["--query-file", "q.txt"], "--query-file <FILE>"), (["--query-skf", "b.skf"], "--query-skf <FILE>")]


@pytest.fixture
def wd(tmp_path):
    (tmp_path / "q.txt").write_text("a\n")
    return str(tmp_path)


def test_help_lists_the_forest_options_after_closest():
    out = _ska("distance", "--help", cwd=ROOT).stdout.decode()
    lines = out.splitlines()
    at = [n for n, ln in enumerate(lines) if ln.lstrip().startswith("--closest <K>")]
    assert len(at) == 1
    for n, (flag, value) in enumerate(MST_OPTS):
        ln = lines[at[0] + 1 + n].lstrip()
        assert ln.startswith((flag + " " + value).strip() + "  ") and "(MI355X engine)" in ln, ln
    assert lines[at[0] + 4].lstrip().startswith("-v, --verbose")
    assert "[default: 250,100,50,25,10,5,0]" in lines[at[0] + 3]


@pytest.mark.parametrize("other, oarg", OTHERS, ids=[o[1].split()[0] for o in OTHERS])
def test_the_forest_refuses_what_needs_the_table_or_several_devices(wd, other, oarg):
    for args in (["--mst", *other], [*other, "--mst"], ["--mst", "--mst-clusters", "p", *other]):          # --mst is named first either way
        r = _ska("distance", "x.skf", *args, cwd=wd, ok=False)
        _refused(r, f"error: the argument '--mst' cannot be used with '{oarg}'" + USAGE + HINT, wd)


def test_another_selection_option_is_named_first(wd):
    for args in (["--mst", "--closest", "2"], ["--closest", "2", "--mst"], ["--max-snps", "3", "--closest", "2", "--mst"]):
        r = _ska("distance", "x.skf", *args, cwd=wd, ok=False)
        _refused(r, "error: the argument '--closest <K>' cannot be used with '--mst'" + USAGE + HINT, wd)
    # the existing order holds where a threshold meets what it has always been refused with
    r = _ska("distance", "x.skf", "--mst", "--max-snps", "3", "--tree", "t.nwk", cwd=wd, ok=False)
    _refused(r, "error: the argument '--max-snps <N>' cannot be used with '--tree <FILE>'" + USAGE + HINT, wd)
    r = _ska("distance", "x.skf", "--mst", "--closest", "2", "--query", "a", cwd=wd, ok=False)
    _refused(r, "error: the argument '--closest <K>' cannot be used with '--query <NAMES>'" + USAGE + HINT, wd)
    r = _ska("distance", "x.skf", "--mst", "--no-table", "--max-mismatches", "0.5", cwd=wd, ok=False)
    _refused(r, "error: the argument '--no-table' cannot be used with '--max-mismatches <P>'" + USAGE + HINT, wd)


MISSING = [(["--mst-clusters", "p"], "--mst"), (["--levels", "5,0"], "--mst\n  --mst-clusters <PREFIX>"), (["--mst-clusters", "p", "--levels", "5,0"], "--mst"),
           (["--mst", "--levels", "5,0"], "--mst-clusters <PREFIX>"), (["--mst", "--max-snps", "3", "--levels", "5"], "--mst-clusters <PREFIX>")]


@pytest.mark.parametrize("args, missing", MISSING, ids=[" ".join(m[0]) for m in MISSING])
def test_the_ladder_needs_the_forest(wd, args, missing):
    r = _ska("distance", "x.skf", *args, cwd=wd, ok=False)
    _refused(r, f"error: the following required arguments were not provided:\n  {missing}" + USAGE + HINT, wd)


BAD_LEVELS = [("", "cannot parse float from empty string"), ("5,,0", "cannot parse float from empty string"), ("5,0,", "cannot parse float from empty string"),
              ("five", "invalid float literal"), ("5;0", "invalid float literal"), ("5, 0", "invalid float literal"), ("0x10", "invalid float literal"),
              ("-1", "a level must be zero or more"), ("5,nan", "a level must be zero or more"), ("5,0,5.0", "a level is given twice"), ("0,-0", "a level is given twice"),
              (",".join(str(n) for n in range(17)), "at most 16 levels")]


@pytest.mark.parametrize("value, why", BAD_LEVELS, ids=[b[0] or "empty" for b in BAD_LEVELS])
def test_bad_levels(wd, value, why):
    r = _ska("distance", "x.skf", "--mst", "--mst-clusters", "p", "--levels", value, cwd=wd, ok=False)
    _refused(r, f"error: invalid value '{value}' for '--levels <L1,L2,...>': {why}" + HINT, wd)
    r = _ska("distance", "x.skf", "--mst", "--mst-clusters", "", cwd=wd, ok=False)
    _refused(r, "error: invalid value '' for '--mst-clusters <PREFIX>': a value is required" + HINT, wd)


def test_bad_thresholds_are_refused_as_without_the_forest(wd):
    r = _ska("distance", "x.skf", "--mst", "--max-snps", "-1", cwd=wd, ok=False)
    _refused(r, "error: invalid value '-1' for '--max-snps <N>': must be zero or more" + HINT, wd)
    r = _ska("distance", "x.skf", "--mst", "--max-mismatches", "1.5", cwd=wd, ok=False)
    _refused(r, "error: invalid value '1.5' for '--max-mismatches <P>': Proportion must be between 0 and 1 (inclusive)" + HINT, wd)


@pytest.mark.parametrize("args", (["--mst"], ["--mst-clusters", "p"], ["--levels", "1"]), ids=lambda a: a[0])
def test_other_subcommands_refuse_the_options(wd, args):
    r = _ska("align", "x.skf", *args, cwd=wd, ok=False)
    _refused(r, f"error: unexpected argument '{args[0]}' found\n\nUsage: ska align [OPTIONS]" + HINT, wd)


# ---------------------------------------------------------------------------------------------- goldens
def _printed_values_decide(text, criteria):
    """the model reads the table's text, the engine compares the doubles behind it: the two agree when no printed value sits on a threshold
    unless it is exact (a distance without --allow-ambiguous is an integer; a proportion printed as 0 or 1 has no mismatch / no match)"""
    for ln in text.splitlines()[1:]:
        f = ln.split("\t")
        if "max_mismatches" in criteria and float(f[3]) == criteria["max_mismatches"]:
            assert (f[3] == "1.00000" and f[4] == "0") or (f[3] == "0.00000" and f[5] == "0"), ln
        if "max_snps" in criteria and float(f[2]) == criteria["max_snps"]:
            assert f[2].endswith(".00"), ln


def _flags(criteria):
    names = {"max_snps": "--max-snps", "max_mismatches": "--max-mismatches"}
    return [x for k, v in criteria.items() for x in (names[k], str(v))]


CRITERIA = [{}, {"max_snps": 0}, {"max_snps": 1}, {"max_mismatches": 0.5}, {"max_mismatches": 0.6}, {"max_snps": 1, "max_mismatches": 0.6}, {"max_snps": 1000, "max_mismatches": 1}]
TABLES = [("multidist.skf", "multidist.stdout", []), ("multidist.skf", "multidist.minfreq.stdout", ["--min-freq", "0.9"]),
          ("multidist.skf", "multidist.ambig.stdout", ["--allow-ambiguous"]), ("merge_k41.skf", "merge_k41.dist.stdout", [])]


@pytest.mark.gpu
@pytest.mark.parametrize("skf, golden, flags", TABLES, ids=[t[1] for t in TABLES])
def test_the_forest_of_the_golden_tables(tmp_path, skf, golden, flags):
    text = _golden(golden)
    sizes = set()
    for criteria in CRITERIA:
        if "--allow-ambiguous" in flags and criteria.get("max_snps") in (0, 1):
            criteria = {**criteria, "max_snps": criteria["max_snps"] + 0.49}                   # between the printed values: multiples of 1/36 keep 0.01 away
        _printed_values_decide(text, criteria)
        r = _ska("distance", _fin(skf), "--mst", *_flags(criteria), *flags, cwd=str(tmp_path))
        assert r.stdout.decode() == mst_text(text, **criteria), criteria
        sizes.add(len(r.stdout.splitlines()))
    if golden == "multidist.stdout":
        assert max(sizes) == 6 and len(sizes) > 1                                              # six samples: a tree of five lines, less under a threshold


@pytest.mark.gpu
def test_the_worked_case_the_output_file_and_the_ladder(tmp_path):
    wd, src, text = str(tmp_path), _fin("multidist.skf"), _golden("multidist.stdout")
    out = _ska("distance", src, "--mst", cwd=wd).stdout.decode()
    # the distance-0 lines in the table's order, each taken while it still joins two trees: N_test_2 by its first such line, not by its second
    # (ambig_test_2), test_2 by its first (ambig_test_1)
    assert [ln.split("\t")[:2] for ln in out.splitlines()[1:]] == [["N_test_1", "ambig_test_1"], ["N_test_1", "ambig_test_2"], ["N_test_1", "test_1"],
                                                                    ["N_test_2", "ambig_test_1"], ["ambig_test_1", "test_2"]]
    r = _ska("distance", src, "--mst", "-o", "out.tsv", "-v", cwd=wd)
    assert r.stdout == b"" and open(os.path.join(wd, "out.tsv")).read() == out
    assert b"Spanning forest of 5 lines in 1 trees from 15 candidate pairs: 1 bands of 6 samples, count buffer of 4608 bytes, at most " in r.stderr
    names, D, M, _ = table_arrays(text)
    for extra, ladder in ((["--levels", "2,1,0"], [2, 1, 0]), ([], [250, 100, 50, 25, 10, 5, 0]), (["--levels", "0.5"], [0.5])):
        r = _ska("distance", src, "--mst", "--mst-clusters", "lad", *extra, cwd=wd)
        assert r.stdout.decode() == out
        columns, csv = levels(D, M, mst(D, M), ladder, names)
        assert open(os.path.join(wd, "lad.levels.csv")).read() == csv
    assert csv.splitlines()[:2] == ["id,snps_0.5,address", "N_test_1,1,1"] and columns[0] == [1] * 6          # every line of this forest is a 0.00
    # under a threshold the ladder is the forest's of the lines kept
    crit = {"max_mismatches": 0.6}
    r = _ska("distance", src, "--mst", "--max-mismatches", "0.6", "--mst-clusters", "lad", "--levels", "2,1,0", "-o", "kept.tsv", cwd=wd)
    assert open(os.path.join(wd, "kept.tsv")).read() == mst_text(text, **crit)
    columns, csv = levels(D, M, mst(D, M, **crit), [2, 1, 0], names)
    assert columns == [[1, 1, 2, 2, 1, 1], [1, 1, 2, 2, 1, 1], [1, 2, 3, 3, 1, 4]] and open(os.path.join(wd, "lad.levels.csv")).read() == csv
