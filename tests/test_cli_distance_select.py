"""`ska distance --max-snps / --max-mismatches / --closest` at the command line: the lines of the table the selection model
(tests/select_model.py) keeps, from the golden tables' text.  The refusals and the help need no device and run everywhere."""
import os
import subprocess

import pytest

from select_model import select_text, table_arrays

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


# ---------------------------------------------------------------------------------------------- no device needed
SELECT_OPTS = [("--max-snps", "--max-snps <N>", "3"), ("--max-mismatches", "--max-mismatches <P>", "0.5"), ("--closest", "--closest <K>", "2")]
OTHERS = [(["--tree", "t.nwk"], "--tree <FILE>"), (["--clusters", "c"], "--clusters <PREFIX>"), (["--gpus", "2"], "--gpus <GPUS>"),
          (["--query", "a"], "--query <NAMES>"), (["--query-file", "q.txt"], "--query-file <FILE>"), (["--query-skf", "b.skf"], "--query-skf <FILE>")]


def _refused(r, message):
    assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", message), r.stderr


def test_help_lists_the_selection_options_after_the_query_options():
    out = _ska("distance", "--help", cwd=ROOT).stdout.decode()
    lines = out.splitlines()
    at = [n for n, ln in enumerate(lines) if ln.lstrip().startswith("--query-skf <FILE>")]
    assert len(at) == 1
    for n, (_, arg, _) in enumerate(SELECT_OPTS):
        ln = lines[at[0] + 1 + n].lstrip()
        assert ln.startswith(arg) and "(MI355X engine)" in ln, ln
    assert out.index("--closest <K>") < out.index("-v, --verbose")


@pytest.mark.parametrize("flag, arg, value", SELECT_OPTS)
def test_selection_refuses_what_needs_the_whole_table(tmp_path, flag, arg, value):
    (tmp_path / "q.txt").write_text("a\n")
    for other, oarg in OTHERS:
        for args in ([flag, value, *other], [*other, flag, value]):                          # the selection option is named first either way
            r = _ska("distance", "x.skf", *args, cwd=str(tmp_path), ok=False)
            _refused(r, f"error: the argument '{arg}' cannot be used with '{oarg}'" + USAGE + HINT)
    assert not os.path.exists(tmp_path / "t.nwk")


def test_the_earliest_selection_option_is_named(tmp_path):
    wd = str(tmp_path)
    r = _ska("distance", "x.skf", "--closest", "1", "--max-mismatches", "0.5", "--max-snps", "2", "--tree", "t", cwd=wd, ok=False)
    _refused(r, "error: the argument '--max-snps <N>' cannot be used with '--tree <FILE>'" + USAGE + HINT)
    r = _ska("distance", "x.skf", "--closest", "1", "--max-mismatches", "0.5", "--query", "a", "--clusters", "c", cwd=wd, ok=False)
    _refused(r, "error: the argument '--max-mismatches <P>' cannot be used with '--clusters <PREFIX>'" + USAGE + HINT)


BAD_VALUES = [("--max-snps", "--max-snps <N>", "many", "invalid float literal"), ("--max-snps", "--max-snps <N>", "-1", "must be zero or more"),
              ("--max-mismatches", "--max-mismatches <P>", "half", "invalid float literal"),
              ("--max-mismatches", "--max-mismatches <P>", "1.5", "Proportion must be between 0 and 1 (inclusive)"),
              ("--max-mismatches", "--max-mismatches <P>", "-0.1", "Proportion must be between 0 and 1 (inclusive)"),
              ("--closest", "--closest <K>", "1.5", "invalid digit found in string"), ("--closest", "--closest <K>", "few", "invalid digit found in string"),
              ("--closest", "--closest <K>", "0", "must be one or higher")]


@pytest.mark.parametrize("flag, arg, value, why", BAD_VALUES, ids=[f"{b[0]}={b[2]}" for b in BAD_VALUES])
def test_bad_values(tmp_path, flag, arg, value, why):
    r = _ska("distance", "x.skf", flag, value, cwd=str(tmp_path), ok=False)
    _refused(r, f"error: invalid value '{value}' for '{arg}': {why}" + HINT)


@pytest.mark.parametrize("flag, arg, why", [("--max-snps", "--max-snps <N>", "cannot parse float from empty string"),
                                            ("--max-mismatches", "--max-mismatches <P>", "cannot parse float from empty string"),
                                            ("--closest", "--closest <K>", "cannot parse integer from empty string")])
def test_empty_values(tmp_path, flag, arg, why):
    r = _ska("distance", "x.skf", flag, "", cwd=str(tmp_path), ok=False)
    _refused(r, f"error: invalid value '' for '{arg}': {why}" + HINT)


def test_other_subcommands_refuse_the_options(tmp_path):
    r = _ska("align", "x.skf", "--closest", "1", cwd=str(tmp_path), ok=False)
    assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", "error: unexpected argument '--closest' found\n\nUsage: ska align [OPTIONS]" + HINT)


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
    names = {"max_snps": "--max-snps", "max_mismatches": "--max-mismatches", "closest": "--closest"}
    return [x for k, v in criteria.items() for x in (names[k], str(v))]


GROUPS = {
    "max-snps": [{"max_snps": v} for v in (0, 1, 2, 1000)],
    "max-mismatches": [{"max_mismatches": v} for v in (0, 0.3, 0.6, 1)],
    "closest": [{"closest": v} for v in (1, 2, 5, 7)],
    "combined": [{"max_snps": 1, "max_mismatches": 0.6}, {"closest": 1, "max_mismatches": 0.6}, {"closest": 2, "max_snps": 1},
                 {"closest": 5, "max_snps": 2, "max_mismatches": 1}],
}
TABLES = [("multidist.skf", "multidist.stdout", []), ("multidist.skf", "multidist.minfreq.stdout", ["--min-freq", "0.9"]),
          ("merge_k41.skf", "merge_k41.dist.stdout", [])]


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("skf, golden, flags", TABLES, ids=[t[1] for t in TABLES])
def test_selection_of_the_golden_tables(tmp_path, skf, golden, flags, group):
    text = _golden(golden)
    for criteria in GROUPS[group]:
        _printed_values_decide(text, criteria)
        r = _ska("distance", _fin(skf), *_flags(criteria), *flags, cwd=str(tmp_path))
        assert r.stdout.decode() == select_text(text, **criteria), criteria


@pytest.mark.gpu
def test_the_worked_cases_and_the_output_file(tmp_path):
    wd, src, text = str(tmp_path), _fin("multidist.skf"), _golden("multidist.stdout")
    for args, n_lines in ((["--max-mismatches", "0.6"], 7), (["--max-mismatches", "0.6", "--max-snps", "1"], 5), (["--closest", "1", "--max-mismatches", "0.6"], 4)):
        out = _ska("distance", src, *args, cwd=wd).stdout.decode()
        assert len(out.splitlines()) == 1 + n_lines, args
    assert [ln.split("\t")[:2] for ln in out.splitlines()[1:]] == [["N_test_1", "test_1"], ["N_test_1", "test_2"], ["N_test_2", "test_1"],
                                                                    ["ambig_test_1", "ambig_test_2"]]
    r = _ska("distance", src, "--closest", "1", "--max-mismatches", "0.6", "-o", "out.tsv", cwd=wd)
    assert r.stdout == b"" and open(os.path.join(wd, "out.tsv")).read() == out
    # every pair passes: the table itself
    assert _ska("distance", src, "--max-snps", "1000", "--max-mismatches", "1", "--closest", "5", cwd=wd).stdout.decode() == text


@pytest.mark.gpu
def test_allow_ambiguous_thresholds_between_the_printed_values(tmp_path):
    """--allow-ambiguous distances are multiples of 1/36, none of which lies within 0.01 of n + 0.49: the two printed decimals decide"""
    text = _golden("multidist.ambig.stdout")
    _, D, _, _ = table_arrays(text)
    kept = set()
    for n in (0, 1, 2, 1000):
        criteria = {"max_snps": n + 0.49}
        r = _ska("distance", _fin("multidist.skf"), "--allow-ambiguous", *_flags(criteria), cwd=str(tmp_path))
        assert r.stdout.decode() == select_text(text, **criteria), criteria
        kept.add(len(r.stdout.splitlines()))
    assert len(kept) > 1 and max(kept) == 16                                           # the thresholds bite differently, the last keeps all
    criteria = {"max_snps": 1.49, "max_mismatches": 0.6}
    _printed_values_decide(text, {"max_mismatches": 0.6})
    r = _ska("distance", _fin("multidist.skf"), "--allow-ambiguous", *_flags(criteria), cwd=str(tmp_path))
    assert r.stdout.decode() == select_text(text, **criteria)
