"""tests/sites_model.py (the model the GPU tests of `ska distance --sites` compare against) held against the oracle and the committed distance
tables: the number of sites of a pair is the pair's Distance, the NoConst stage never removes a site row, and two wrong variants of the model
differ from it on these very inputs.  CPU only."""
import functools
import os

import numpy as np
import pytest

import ora
import sites_model as SM
from select_model import table_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["merge.skf", "merge_k9.skf", "merge_k41.skf", "multidist.skf"]
MIN_FREQS = [0.0, 0.5, 1.0]
# the committed filter-ambiguous tables: (fixture, min_freq) -> file under tests/golden/correct (merge_k9.dist.stdout is the --allow-ambiguous one)
GOLDENS = {("merge.skf", 0.0): "merge.dist.stdout", ("merge_k9.skf", 0.0): "merge_k9_no_ambig.dist.stdout", ("merge_k9.skf", 1.0): "merge_k9_min_freq.dist.stdout",
           ("merge_k41.skf", 0.0): "merge_k41.dist.stdout", ("multidist.skf", 0.0): "multidist.stdout", ("multidist.skf", 0.9): "multidist.minfreq.stdout"}


def _path(fixture):
    return os.path.join(HERE, "golden", "input", fixture)


@functools.lru_cache(maxsize=None)
def _export(fixture):
    a = ora.Array.load(_path(fixture))
    keys, var, counts = a.export()
    return a.names, keys, var, counts


def _oracle_distances(fixture, min_freq):
    """generic_modes::distance as the oracle's distance_tsv chains it, the doubles instead of their text"""
    a = ora.Array.load(_path(fixture))
    if min_freq * a.nsamples >= 1.0:
        a.apply_filters(min_freq, False, ora.FILTER_NONE)
    constant = a.apply_filters(0.0, False, ora.FILTER_NO_CONST)
    return a.distance(float(constant), True)["distance"]


def _model_counts(fixture, min_freq, **wrong):
    names, _, var, counts = _export(fixture)
    pairs = SM.all_pairs(len(names))
    keep = SM.sweep_flags(var, min_freq, counts, use_threshold=not wrong.get("ignore_threshold", False))
    recs = SM.sites(var, keep, pairs, count_ambiguous=wrong.get("count_ambiguous", False))
    # sorted by (pair, row), every (pair, row) once
    word = (recs["pair"].astype(np.int64) << 40) | recs["row"].astype(np.int64)
    assert (np.diff(word) > 0).all()
    return SM.counts_of(recs, len(pairs)), recs


@pytest.mark.parametrize("min_freq", MIN_FREQS)
@pytest.mark.parametrize("fixture", FIXTURES)
def test_counts_are_the_oracles_distances(fixture, min_freq):
    got, _ = _model_counts(fixture, min_freq)
    want = _oracle_distances(fixture, min_freq)
    assert len(got) == len(want) > 0
    assert np.array_equal(got.astype(np.float64), want), (fixture, min_freq)


@pytest.mark.parametrize("fixture,min_freq", sorted(GOLDENS))
def test_counts_are_the_committed_tables(fixture, min_freq):
    text = open(os.path.join(HERE, "golden", "correct", GOLDENS[(fixture, min_freq)])).read()
    names, D, _, _ = table_arrays(text)
    assert names == _export(fixture)[0]
    got, _ = _model_counts(fixture, min_freq)
    want = [D[i][j] for i, j in SM.all_pairs(len(names))]
    assert [float(x) for x in got] == want
    if GOLDENS[(fixture, min_freq)] == "multidist.stdout":
        assert set(want) == {0.0, 1.0, 2.0}


@pytest.mark.parametrize("fixture", FIXTURES)
def test_noconst_never_removes_a_site_row(fixture):
    names, keys, var, counts = _export(fixture)
    assert len(keys) == len(var)
    a = ora.Array.load(_path(fixture))
    a.filter(0, False, ora.FILTER_NO_CONST, False, False, True)             # update_kmers: the keys stay in step with the rows
    kept = {(int(k["hi"]), int(k["lo"])) for k in a.export()[0]}
    assert 0 < len(kept) <= len(keys)
    assert fixture not in ("merge.skf", "merge_k9.skf") or len(kept) < len(keys)                      # the stage removes something there
    flags = SM.no_const_flags(var)
    assert {(int(k["hi"]), int(k["lo"])) for k in keys[flags]} == kept       # the model's NoConst is the oracle's
    recs = SM.sites(var, np.ones(len(var), bool), SM.all_pairs(len(names)))  # the sites of every row, swept or not
    assert len(recs) > 0
    assert all((int(k["hi"]), int(k["lo"])) in kept for k in keys[np.unique(recs["row"]).astype(np.int64)])


def test_wrong_variants_differ_on_these_inputs():
    """a model that counts ambiguous cells, and one that ignores the frequency threshold, are told apart by the fixtures the tests above use"""
    ambiguous = [f for f in FIXTURES if not np.array_equal(_model_counts(f, 0.0)[0], _model_counts(f, 0.0, count_ambiguous=True)[0])]
    assert "multidist.skf" in ambiguous
    blind = [(f, m) for f in FIXTURES for m in (0.5, 1.0) if not np.array_equal(_model_counts(f, m)[0], _model_counts(f, m, ignore_threshold=True)[0])]
    assert blind
    for f, m in blind:                                                       # and the oracle sides with the model
        assert np.array_equal(_model_counts(f, m)[0].astype(np.float64), _oracle_distances(f, m))


def test_text_of_a_worked_example():
    var = np.array([[ord(c) for c in row] for row in ["ACA", "AAA", "A-C", "RCA", "TTG", "CA-"]], np.uint8)
    keep = SM.sweep_flags(var, 0.0)
    assert keep.tolist() == [True, False, True, True, True, True]
    recs = SM.sites(var, keep, [(1, 2), (0, 1), (0, 2)])
    assert [(int(r["pair"]), int(r["row"]), chr(r["base_i"]), chr(r["base_j"])) for r in recs] == [
        (0, 0, "C", "A"), (0, 3, "C", "A"), (0, 4, "T", "G"), (1, 0, "A", "C"), (1, 5, "C", "A"), (2, 2, "A", "C"), (2, 4, "T", "G")]
    assert SM.sweep_flags(var, 1.0).tolist() == [True, False, False, True, True, False]        # rows 2 and 5 hold two of three samples
    keys = np.zeros(6, ora.KEY_DT)
    keys["lo"] = [0b0001_1011, 0, 0b1110_0100, 0, 0, 0]                      # k = 5: two bases an arm
    text = SM.sites_text(["x", "y", "z"], keys, 5, [(1, 2), (0, 2)], SM.sites(var, keep, [(1, 2), (0, 2)])[[0, 3]])
    assert text == SM.HEADER + "y\tz\tAC\tTG\tC\tA\nx\tz\tGT\tCA\tA\tC\n"
