"""tests/qc_model.py (the model `ska qc` is held to on the GPU) against what it must equal: the oracle's alignments, its delete_samples and its
distances on the `tiny` and `k31` cases of subset_model, a cell-by-cell restatement, a hand-worked example and curve_model at t = S.  Four wrong
variants of the model (ties for major to the highest code, private without the unamb >= 2 gate, floor for ceil in the threshold, ambiguous cells
counted into c[b]) must fail these checks.  The flag rule is worked by hand, and the host-only writer skh_qc_text is held to the model's three
texts: it needs no device.  CPU only.

One sentence of the feature's description does not follow from its own rule and is not asserted: "S = 2 gives no flags by the rule itself".
By the rule as stated med is place (S - 1) // 2 = 0 of the sorted values, the smaller one, and mad is place 0 of the sorted |x - med|, which is
0, so d = 1 and the larger value is high as soon as it is more than M above the smaller.  test_rule_at_one_and_two_samples asserts the rule."""
import math

import numpy as np
import pytest

import curve_model as CM
import ora
import qc_model as Q
import subset_model as M

Opts = M.Opts
FREQS = (0.0, 0.5, 0.9, 1.0)
CASES = ("tiny", "k31")


def _lines(aln):
    return [np.frombuffer(l, np.uint8) for l in aln.split(b"\n")[1::2]]


def _oracle_alignment(case, f):
    """the oracle's `ska align --min-freq f --filter no-filter`: one line of letters per sample"""
    return _lines(M._oracle_array(case).align(filter_type=ora.FILTER_NONE, min_freq=f))


def _letters(line, other_than):
    return int((~np.isin(line, np.frombuffer(other_than, np.uint8))).sum())


def _check_alignment_counts(case, **wrong):
    var = M.oracle_export(case)
    got, _ = Q.sample_qc(var, 0.0, **wrong)
    lines = _oracle_alignment(case, 0.0)
    assert len(lines) == var.shape[1]
    assert [int(x) for x in got["kmers"]] == [_letters(l, b"-") for l in lines], case
    assert [int(x) for x in got["ambiguous"]] == [_letters(l, b"ACGT-") for l in lines], case
    assert got["ambiguous"].sum() > 0
    for f in FREQS:
        got, info = Q.sample_qc(var, f, **wrong)
        lines = _oracle_alignment(case, f)
        assert [int(x) for x in got["core_present"]] == [_letters(l, b"-") for l in lines], (case, f)
        assert int(info["core_rows"]) == len(lines[0]) - (int((Q.CODE[var] == 0).all(axis=1).sum()) if f == 0.0 else 0), (case, f)


@pytest.mark.parametrize("case", CASES)
def test_kmers_ambiguous_and_core_present_are_the_oracles_alignments(case):
    _check_alignment_counts(case)
    var = M.oracle_export(case)
    core = [int(Q.sample_qc(var, f)[1]["core_rows"]) for f in FREQS]
    assert core[0] > core[1] > 0 and core[1] >= core[-1]                 # the frequencies tell rows apart


@pytest.mark.parametrize("case", CASES)
def test_singletons_are_the_rows_the_oracles_delete_removes(case):
    var = M.oracle_export(case)
    S = var.shape[1]
    got, info = Q.sample_qc(var, 0.9)
    opts = Opts((0.0, False, 0, False, True))
    _, everybody, _ = M.oracle_chain(case, tuple(range(S)), opts)
    assert everybody == int(info["rows_present"])
    for s in range(S):
        _, left, _ = M.oracle_chain(case, tuple(x for x in range(S) if x != s), opts)
        assert int(got["singletons"][s]) == everybody - left, (case, s)
        assert left == M.model(var, [x for x in range(S) if x != s], opts)[1]["rows_present"]
    assert got["singletons"].sum() > 0


def _oracle_distance(case, i, j):
    """generic_modes::distance of the two samples left after the oracle's delete_samples of the others, ambiguous bases filtered"""
    a = M._oracle_array(case)
    names = M.names_of(case)
    a.delete_samples([n for x, n in enumerate(names) if x not in (i, j)])
    constant = a.apply_filters(0.0, False, ora.FILTER_NO_CONST)
    return float(a.distance(float(constant), True)["distance"][0])


def _check_pairs(**wrong):
    var = M.oracle_export("tiny")
    S = var.shape[1]
    assert S == 6
    seen = 0
    for i in range(S):
        for j in range(i + 1, S):
            got, _ = Q.sample_qc(var[:, [i, j]], 0.0, **wrong)
            d = _oracle_distance("tiny", i, j)
            assert float(got["private_alleles"][0]) == float(got["private_alleles"][1]) == d, (i, j)
            seen += d > 0
    assert seen > 0


def test_private_alleles_of_two_samples_are_the_oracles_distance():
    _check_pairs()


# ---- a hand-worked example: 8 rows x 4 samples at min_freq 0.7, thr = ceil(2.8) = 3 ----
HAND = np.array([list(r.encode()) for r in (
    "AACC",      # A and C tie: major A, samples 2 and 3 minor; nobody private (c = 2, 2)
    "TTGG",      # T and G tie: major T, samples 2 and 3 minor
    "NRYM",      # ambiguous cells only: core, no major, nobody private or minor
    "--G-",      # one cell: a singleton of sample 2, not core; c[G] = 1 but unamb = 1: not private
    "ARNN",      # a plain base alone among ambiguous cells: c[A] = 1, unamb = 1: not private; core
    "AAC-",      # n = 3, exactly the threshold: core; sample 2 private (c[C] = 1, unamb = 3) and minor
    "A-C-",      # n = 2: not core (core with floor: thr = 2); samples 0 and 2 private, nobody minor
    "----",      # no cell present
)], np.uint8)
HAND_F = 0.7
#              kmers  ambiguous  singletons  core_present  private_alleles  minor_alleles
HAND_WANT = [[6, 1, 0, 5, 1, 0],
             [5, 2, 0, 5, 0, 0],
             [7, 2, 1, 5, 2, 3],
             [4, 2, 0, 4, 0, 2]]
HAND_INFO = [8, 7, 5, 3, 3]                                               # rows, rows_present, core_rows, core_variant_rows, threshold


def _hand(**wrong):
    got = Q.as_lists(*Q.sample_qc(HAND, HAND_F, **wrong))
    assert got == (HAND_WANT, HAND_INFO), got


def test_hand_worked_example():
    _hand()
    assert Q.sample_qc_slow(HAND, HAND_F) == (HAND_WANT, HAND_INFO)
    assert Q.threshold(4, 0.7) == 3 and Q.threshold(4, 0.75) == 3 and Q.threshold(4, 0.0) == 1 and Q.threshold(13, 0.9) == 12 and Q.threshold(10, 1e-9) == 1


def test_cell_by_cell_restatement_on_random_matrices():
    rng = np.random.default_rng(8)
    letters = np.frombuffer(b"-ACGTMRWSYKVHDBN\0", np.uint8)
    for U, S in ((40, 7), (9, 1), (25, 12), (0, 3), (30, 2)):
        var = letters[rng.integers(0, len(letters), size=(U, S))]
        var[rng.random((U, S)) < 0.4] = ord("-")
        var[: U // 3] = np.where(rng.random((U // 3, S)) < 0.8, np.uint8(ord("A")), var[: U // 3])      # rows with a clear major base
        for f in (0.0, 1e-9, 0.5, 0.9, 1.0):
            assert Q.as_lists(*Q.sample_qc(var, f)) == Q.sample_qc_slow(var, f), (U, S, f)


def _check_against_curve(case, **wrong):
    var = M.oracle_export(case)
    S = var.shape[1]
    for f in (0.0, 0.5, 0.6, 0.9, 1.0):
        _, info = Q.sample_qc(var, f, **wrong)
        last = CM.curve(var, [np.arange(S)], f)[0, -1]
        assert (int(info["rows_present"]), int(info["core_rows"]), int(info["core_variant_rows"])) == (int(last[0]), int(last[1]), int(last[3])), (case, f)
        assert int(info["threshold"]) == int(CM.thresholds(S, f)[-1]) and int(info["rows"]) == len(var)


@pytest.mark.parametrize("case", CASES)
def test_totals_are_curves_last_step(case):
    _check_against_curve(case)
    assert int(Q.sample_qc(M.oracle_export(case), 0.5)[1]["core_variant_rows"]) > 0


WRONG = {"ties_to_highest": dict(ties_to_highest=True), "private_ungated": dict(private_ungated=True), "floor": dict(rounding=math.floor),
         "ambiguous_are_bases": dict(ambiguous_are_bases=True)}


@pytest.mark.parametrize("name", sorted(WRONG))
def test_wrong_variants_are_caught(name):
    wrong = WRONG[name]
    with pytest.raises(AssertionError):
        _hand(**wrong)
    if name == "floor":                                                  # 13 x 0.9 = 11.7: the oracle's alignments and curve differ too
        with pytest.raises(AssertionError):
            _check_alignment_counts("k31", **wrong)
        with pytest.raises(AssertionError):
            _check_against_curve("k31", **wrong)
    if name == "ambiguous_are_bases":
        with pytest.raises(AssertionError):
            _check_against_curve("k31", **wrong)


# ---- the flag rule ----
def _records(S, **columns):
    r = np.zeros(S, Q.SAMPLE_DT)
    for k, v in columns.items():
        r[k] = v
    return r


def _info(core_rows=0, rows=0):
    i = np.zeros(1, Q.INFO_DT)[0]
    i["core_rows"], i["rows"], i["rows_present"], i["threshold"] = core_rows, rows, rows, 1
    return i


def test_rule_at_one_and_two_samples():
    per, stats = Q.flags(_records(1, kmers=[10**12], ambiguous=[7]), _info())
    assert per == [[]] and stats["kmers"] == (10**12, 10**12, 10**12, 0, 0)
    # two samples: med is the smaller value, mad 0, d = 1 -- the larger is high once it is more than M above, the smaller is never low
    assert Q.flags(_records(2, kmers=[100, 105]), _info(), 5.0)[0] == [[], []]
    assert Q.flags(_records(2, kmers=[100, 106]), _info(), 5.0)[0] == [[], ["high_kmers"]]
    assert Q.flags(_records(2, kmers=[106, 100]), _info(), 5.0)[0] == [["high_kmers"], []]
    assert Q.flags(_records(2, kmers=[100, 100]), _info(), 0.0)[0] == [[], []]
    assert Q.flags(_records(0), _info())[0] == []


def test_mad_zero_falls_back_to_one():
    x = [50] * 9 + [55, 56, 44, 45]
    side, st = Q.outliers(x, 5.0, both_sides=True)
    assert st == (44, 50, 56, 0) and side == [None] * 9 + [None, "high", "low", None]
    assert Q.outliers(x, 5.0, both_sides=False)[0][11] is None
    # and a mad above one scales the bound: with two values far above 0..8 med is 5 and mad 3
    side, st = Q.outliers(list(range(9)) + [14, 15], 5.0, both_sides=True)
    assert st == (0, 5, 15, 3) and side == [None] * 11
    side, _ = Q.outliers(list(range(9)) + [20, 21], 5.0, both_sides=True)
    assert side == [None] * 9 + [None, "high"]                                         # med 5, mad 3: 20 - 5 = 15 is not above 15, 21 - 5 is


def test_one_planted_outlier_per_metric_and_nobody_else():
    S = 11
    rng = np.random.default_rng(5)
    # every column within one of its centre: mad <= 1, so d = 1 and no deviation (<= 2) is above M = 5
    base = dict(kmers=5000 + rng.integers(-1, 2, S), ambiguous=30 + rng.integers(-1, 2, S), singletons=10 + rng.integers(-1, 2, S),
                core_present=4000 - rng.integers(0, 3, S), private_alleles=8 + rng.integers(-1, 2, S), minor_alleles=40 + rng.integers(-1, 2, S))
    info = _info(core_rows=4010, rows=6000)
    assert Q.flags(_records(S, **base), info)[0] == [[] for _ in range(S)]
    plants = (("kmers", 9000, "high_kmers"), ("kmers", 900, "low_kmers"), ("ambiguous", 900, "ambiguous"), ("singletons", 2000, "singletons"),
              ("core_present", 1000, "core_missing"), ("private_alleles", 500, "private_alleles"), ("minor_alleles", 700, "minor_alleles"))
    for at, (column, value, flag) in enumerate(plants):
        cols = {k: v.copy() for k, v in base.items()}
        cols[column][at] = value
        per, stats = Q.flags(_records(S, **cols), info)
        assert per == [[flag] if s == at else [] for s in range(S)], (column, per)
        assert sum(st[4] for st in stats.values()) == 1
    cols = {k: v.copy() for k, v in base.items()}                                       # several at once: the order of the flags is FLAGS'
    cols["minor_alleles"][3], cols["kmers"][3], cols["ambiguous"][3] = 700, 9000, 900
    assert Q.flags(_records(S, **cols), info)[0][3] == ["high_kmers", "ambiguous", "minor_alleles"]
    cols["core_present"][4] = 5000                                                      # made-up: above core_rows -> core_missing 0, no flag
    assert Q.metric_values(_records(S, **cols), info)["core_missing"][4] == 0


# ---- the texts ----
def test_texts_by_hand():
    samples, info = Q.sample_qc(HAND, HAND_F)
    t = Q.texts(samples, ["a", "b", "c", "d"], info, 1.0)
    assert t[".qc.tsv"] == ("sample\tkmers\tambiguous\tsingletons\tcore_present\tcore_missing\tprivate_alleles\tminor_alleles\tflags\n"
                            "a\t6\t1\t0\t5\t0\t1\t0\t-\n"
                            "b\t5\t2\t0\t5\t0\t0\t0\t-\n"
                            "c\t7\t2\t1\t5\t0\t2\t3\thigh_kmers,private_alleles,minor_alleles\n"     # kmers: med 5, mad 1: 2 > 1; private and minor: med 0, mad 0: 2 > 1, 3 > 1
                            "d\t4\t2\t0\t4\t1\t0\t2\tminor_alleles\n")                    # kmers: 1 below, not more; core_missing: 1 is not above 1; minor: 2 > 1
    assert t[".qc.summary.tsv"] == ("samples\t4\nrows\t8\nrows_present\t7\ncore_rows\t5\ncore_variant_rows\t3\nthreshold\t3\n"
                                    "metric\tmin\tmedian\tmax\tmad\tflagged\n"
                                    "kmers\t4\t5\t7\t1\t1\nambiguous\t1\t2\t2\t0\t0\nsingletons\t0\t0\t1\t0\t0\ncore_missing\t0\t0\t1\t0\t0\n"
                                    "private_alleles\t0\t0\t2\t0\t1\nminor_alleles\t0\t0\t3\t0\t2\n")
    assert t[".qc.flagged.txt"] == "c\nd\n"
    assert Q.texts(samples, ["a", "b", "c", "d"], info, 100.0)[".qc.flagged.txt"] == ""


def test_host_writer_equals_the_model():
    import skx_engine as E
    rng = np.random.default_rng(0)
    which = {".qc.tsv": E.QC_SAMPLES_TEXT, ".qc.summary.tsv": E.QC_SUMMARY_TEXT, ".qc.flagged.txt": E.QC_FLAGGED_TEXT}
    samples, info = Q.sample_qc(HAND, HAND_F)
    for suffix, text in Q.texts(samples, ["a", "b", "c", "d"], info, 1.0).items():
        assert E.qc_text(which[suffix], samples, ["a", "b", "c", "d"], info, 1.0) == text, suffix
    for S, top, M_ in ((0, 10, 5.0), (1, 10, 5.0), (2, 50, 5.0), (7, 40, 0.0), (30, 1 << 40, 3.5), (64, 1 << 63, 5.0), (200, 100, 1.0), (33, 5, 0.5)):
        samples = np.zeros(S, Q.SAMPLE_DT)
        for f in Q.COUNTS:
            samples[f] = rng.integers(0, top, size=S, dtype=np.uint64) if rng.random() < 0.7 else rng.integers(top // 2, top // 2 + 3, size=S, dtype=np.uint64)
        if S > 3:
            samples["kmers"][S // 2] = top * 2 - 1                       # (below 2^64; above 2^32 for the large tops)
        info = np.zeros(1, Q.INFO_DT)[0]
        info["rows"], info["rows_present"], info["core_rows"], info["core_variant_rows"], info["threshold"] = top, top - 1, int(top // 2 + 1), 3, max(1, S)
        names = [f"sample {i} x" if i % 5 == 0 else f"n{i}" for i in range(S)]
        want = Q.texts(samples, names, info, M_)
        for suffix, text in want.items():
            assert E.qc_text(which[suffix], samples, names, info, M_) == text, (S, suffix)
    big = np.zeros(3, Q.SAMPLE_DT)
    big["kmers"] = [(1 << 33) + 5, (1 << 33) + 6, (1 << 34)]
    text = E.qc_text(E.QC_SAMPLES_TEXT, big, ["a", "b", "c"], np.zeros(1, Q.INFO_DT)[0])
    assert text.splitlines()[3] == f"c\t{1 << 34}\t0\t0\t0\t0\t0\t0\thigh_kmers"
    for bad in (float("nan"), -1.0):
        with pytest.raises(E.EngineError) as ei:
            E.qc_text(E.QC_SAMPLES_TEXT, big, ["a", "b", "c"], np.zeros(1, Q.INFO_DT)[0], bad)
        assert ei.value.code == E.EINVAL
    with pytest.raises(E.EngineError):
        E.qc_text(3, big, ["a", "b", "c"], np.zeros(1, Q.INFO_DT)[0])
