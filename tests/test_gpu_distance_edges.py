"""The distance entry points at the edges of their plane builder (`-m gpu`): no row at all, and kept-row counts on either side of a 64-row
plane word and of the 4 096-row flag group of launch_build_planes_keep, for the single plane set and for the clean / dirty split of
--allow-ambiguous.  Every other distance fixture has at least 1 100 rows and 70 samples and reaches none of these.

Arrays are handed over by the caller (Array.from_host; the oracle's from the same rows): S = 5, k = 9, rows of four kinds in a seeded order --
clean variable (A/C/G/T and '-', two different bases at least), dirty variable (one two-base IUPAC code at least, beside two different
bases), constant (one base in every sample: the NoConst filter removes them and they become the constant) and sparse (one or two present
samples: a min_freq of 0.6 drops them; without a frequency filter they are variable rows, '-' being a symbol of its own to NoConst,
merge_ska_array.rs:322-334, so the arrays swept with min_freq 0.0 are built without them and hold the same kept rows).  Only two-base codes:
every term the oracle adds to a distance is then a multiple of 1/4, its row-by-row float64 sum is exact, and the tables can be compared byte
for byte.  Expected tables are the oracle's: its filters, then its distance with its constant."""
import functools
import math

import numpy as np
import pytest

import ora
from conftest import set_knob

pytestmark = pytest.mark.gpu
S, K = 5, 9
NAMES = [f"s{i}" for i in range(S)]
# (clean, dirty) kept rows; None = an array without any row (the other (0, 0) form: every row constant)
COUNTS = [(0, 0), None, (1, 0), (0, 1), (64, 0), (65, 0), (64, 65), (4096, 1), (4097, 0)]
CASES = [(c, n_const) for c in COUNTS for n_const in (0, 3) if not (c is None and n_const) and not (c == (0, 0) and not n_const)]
IDS = ["no-rows" if c is None else f"{c[0]}-{c[1]}-const{n}" for c, n in CASES]
N_SPARSE = 3
CODES = b"RYSWKM"
BASES = b"ACGT"


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


@functools.lru_cache(maxsize=None)
def rows_of(counts, n_const, sparse, n_samples=S):
    """-> (keys, cells [U, n_samples]) of the recipe; sparse: with the N_SPARSE sparse rows among them"""
    if counts is None:
        return np.zeros(0, ora.KEY_DT), np.zeros((0, n_samples), np.uint8)
    clean, dirty = counts
    rng = np.random.default_rng(1000 * clean + 10 * dirty + n_const)
    rows = []
    for kind, n in (("clean", clean), ("dirty", dirty), ("const", n_const), ("sparse", N_SPARSE if sparse else 0)):
        for r in range(n):
            row = np.full(n_samples, ord("-"), np.uint8)
            if kind == "const":
                row[:] = BASES[r % 4]
            elif kind == "sparse":
                row[rng.choice(n_samples, 1 + r % 2, replace=False)] = BASES[r % 4]
            else:
                present = rng.permutation(n_samples)[: max(int(rng.integers(3, 6)), 3) if n_samples >= 3 else n_samples]
                row[present] = rng.choice(np.frombuffer(BASES, np.uint8), len(present))
                two = rng.choice(4, 2, replace=False)
                row[present[0]] = BASES[two[0]]
                if len(present) > 1:
                    row[present[1]] = BASES[two[1]]                          # two different bases: variable whatever else is drawn
                elif kind == "clean":
                    row[present[0]] = BASES[r % 4]                            # (one sample: nothing to differ from)
                if kind == "dirty":
                    row[present[-1]] = CODES[int(rng.integers(len(CODES)))]
            rows.append(row)
    cells = np.array(rows, np.uint8).reshape(len(rows), n_samples)[rng.permutation(len(rows))]
    keys = np.zeros(len(cells), ora.KEY_DT)
    keys["lo"] = np.sort(rng.choice(4 ** (K - 1), len(cells), replace=False))
    return keys, cells


def is_dirty(cells):
    return ~np.isin(cells, np.frombuffer(BASES + b"-", np.uint8)).all(axis=1)


@functools.lru_cache(maxsize=None)
def expected(counts, n_const, min_freq, filt, n_samples=S):
    """the oracle's side, computed once: -> (table, constant, rows used, kept cells)"""
    keys, cells = rows_of(counts, n_const, min_freq > 0.0, n_samples)
    oa = ora.Array.from_rows(K, True, NAMES[:n_samples], keys, cells)
    if min_freq * n_samples >= 1.0:
        oa.filter(math.ceil(n_samples * min_freq), False, ora.FILTER_NONE, False, False, False)
    oc = oa.filter(0, False, ora.FILTER_NO_CONST, False, False, False)
    table = oa.distance(oc, filt)
    table.setflags(write=False)
    return table, oc, oa.nrows, oa.export()[1]


def engine_array(E, counts, n_const, min_freq, n_samples=S):
    keys, cells = rows_of(counts, n_const, min_freq > 0.0, n_samples)
    return E.Array.from_host(K, True, NAMES[:n_samples], keys, cells)


def filtered(E, counts, n_const, min_freq, n_samples=S):
    """the engine's own two filters, as generic_modes::distance applies them -> (array, constant)"""
    arr = engine_array(E, counts, n_const, min_freq, n_samples)
    if min_freq * n_samples >= 1.0:
        arr.filter(math.ceil(n_samples * min_freq), False, E.FILTER_NONE, False, False, False)
    return arr, arr.filter(0, False, E.FILTER_NO_CONST, False, False, False)


def pair_index(i, j, n=S):
    return i * n - i * (i + 1) // 2 + j - i - 1


def same(got, want):
    return got.tobytes() == np.ascontiguousarray(want).tobytes()


def query_rows(table, query, n=S):
    out = np.zeros((len(query), n), table.dtype)
    for q, x in enumerate(query):
        for j in range(n):
            if j != x:
                out[q, j] = table[pair_index(min(x, j), max(x, j), n)]
    return out


def thresholds(table):
    """cluster thresholds that split the table's pairs where they can: the median distance, every mismatch proportion"""
    return (float(np.median(table["distance"])) if len(table) else 10.0), 1.0


def labels_hold(E, labels, table, n=S):
    cs, cm = thresholds(table)
    return E.clusters_csv(NAMES[:n], labels) == E.distance_clusters(NAMES[:n], table, cs, cm)[0]


@pytest.mark.parametrize("min_freq", [0.0, 0.6])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_preconditions(case, min_freq):
    """on the oracle's side: each case has the kept clean rows, kept dirty rows and removed constant rows it is named for"""
    counts, n_const = case
    _, constant, rows_used, kept = expected(counts, n_const, min_freq, True)
    clean, dirty = counts or (0, 0)
    assert constant == n_const and rows_used == clean + dirty == len(kept)
    assert int(is_dirty(kept).sum()) == dirty
    if counts is not None:
        _, cells = rows_of(counts, n_const, min_freq > 0.0)
        assert len(cells) == clean + dirty + n_const + (N_SPARSE if min_freq else 0)
    if counts == (0, 0):
        assert n_const and len(rows_of(counts, n_const, False)[1]) == n_const          # every row constant: everything is filtered away


def test_no_row_entries_follow_the_rule():
    """merge_ska_array.rs:596-631 on no rows: distance 0, mismatch proportion 0, the constant as the match count, no mismatch"""
    for counts, n_const in ((None, 0), ((0, 0), 3)):
        for filt in (True, False):
            table = expected(counts, n_const, 0.0, filt)[0]
            want = np.zeros(S * (S - 1) // 2, ora.DIST_DT)
            want["match_count"] = n_const
            assert same(table, want)


@pytest.mark.parametrize("min_freq", [0.0, 0.6])
@pytest.mark.parametrize("filt", [True, False])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filtering_entry_points(E, case, filt, min_freq):
    """the entry points that apply the two filters themselves, on the array as handed over"""
    counts, n_const = case
    table, constant, rows_used, _ = expected(counts, n_const, min_freq, filt)
    arr = engine_array(E, counts, n_const, min_freq)
    got, c, r = arr.distance_filtered(min_freq, filt)
    assert same(got, table) and (c, r) == (constant, rows_used)
    for query in ([3], [4, 0]):
        got, c, r = arr.distance_query_filtered(query, min_freq, filt)
        assert same(got, query_rows(table, query)) and (c, r) == (constant, rows_used), query
    pairs, c, r, _ = arr.distance_select(min_freq, filt, max_snps=float(table["distance"].max()) + 1.0)
    assert [(int(p["i"]), int(p["j"])) for p in pairs] == [(i, j) for i in range(S) for j in range(i + 1, S)]
    assert same(pairs["d"], table) and (c, r) == (constant, rows_used)
    pairs, c, r, _ = arr.distance_select(min_freq, filt, closest=1)
    assert len(pairs) >= (S + 1) // 2 and (c, r) == (constant, rows_used)               # every sample is in a pair
    assert same(pairs["d"], table[[pair_index(int(p["i"]), int(p["j"])) for p in pairs]])
    cs, cm = thresholds(table)
    for band_rows in (0, 2):
        labels, _, c, r, _ = arr.distance_banded(min_freq, filt, cluster_snps=cs, cluster_mismatches=cm, band_rows=band_rows)
        assert labels_hold(E, labels, table) and (c, r) == (constant, rows_used), band_rows


@pytest.mark.parametrize("min_freq", [0.0, 0.6])
@pytest.mark.parametrize("filt", [True, False])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_prefiltered_entry_points(E, case, filt, min_freq):
    """the entry points that sweep every row, after the engine's own filter, with its constant"""
    counts, n_const = case
    table, constant, rows_used, _ = expected(counts, n_const, min_freq, filt)
    arr, c = filtered(E, counts, n_const, min_freq)
    assert c == constant and arr.nrows == rows_used
    assert same(arr.distance(c, filt), table)
    for query in ([3], [4, 0]):
        assert same(arr.distance_query(query, c, filt), query_rows(table, query)), query
    pairs, _ = arr.distance_select_prefiltered(c, filt, max_snps=float(table["distance"].max()) + 1.0)
    assert same(pairs["d"], table) and len(pairs) == len(table)
    cs, cm = thresholds(table)
    for band_rows in (0, 2):
        labels, _, _ = arr.distance_banded_prefiltered(c, filt, cluster_snps=cs, cluster_mismatches=cm, band_rows=band_rows)
        assert labels_hold(E, labels, table), band_rows
    ptr, wpr, n_planes = arr.distance_planes(filt)
    assert wpr == max((rows_used + 63) // 64, 1) and n_planes == (4 if filt else 8)
    bands = [E.planes_distance(ptr, S, wpr, filt, c, lo, hi, ctx=arr.ctx) for lo, hi in ((0, 2), (2, 5))]
    assert same(np.concatenate(bands), table)


def test_stale_row_mask_falls_back_to_the_twelve_class_sweep(E, monkeypatch):
    """SKX_KNOBS=stale_row_mask: every kept row is passed off as clean, the check of the 4-plane set finds the dirty ones and all rows go
    through the twelve-class sweep -- the same --allow-ambiguous table"""
    set_knob(monkeypatch, "stale_row_mask", 1)
    for min_freq in (0.0, 0.6):
        table, constant, rows_used, _ = expected((64, 65), 3, min_freq, False)
        got, c, r = engine_array(E, (64, 65), 3, min_freq).distance_filtered(min_freq, False)
        assert same(got, table) and (c, r) == (constant, rows_used)
        arr, c = filtered(E, (64, 65), 3, min_freq)
        assert same(arr.distance(c, False), table)


@pytest.mark.parametrize("filt", [True, False])
@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_samples(E, n, filt):
    """S = 1 and S = 2 at 65 kept rows: every entry point returns, the query form leaves its zeroed self entry, the labels are the table's"""
    table, constant, rows_used, _ = expected((65, 0), 3, 0.0, filt, n)
    assert len(table) == n * (n - 1) // 2 and rows_used == (65 if n > 1 else 0)        # (one sample: every row is constant)
    arr = engine_array(E, (65, 0), 3, 0.0, n)
    got, c, r = arr.distance_filtered(0.0, filt)
    assert same(got, table) and (n == 1 or (c, r) == (constant, rows_used))
    got, _, _ = arr.distance_query_filtered([n - 1], 0.0, filt)
    assert same(got, query_rows(table, [n - 1], n)) and not any(got[0, n - 1].tolist())
    pairs, _, _, _ = arr.distance_select(0.0, filt, max_snps=1e9)
    assert same(pairs["d"], table)
    assert len(arr.distance_select(0.0, filt, closest=1)[0]) == len(table)
    cs, cm = thresholds(table)
    labels = arr.distance_banded(0.0, filt, cluster_snps=cs, cluster_mismatches=cm)[0]
    assert labels.tolist() in ([0], [0, 0], [0, 1]) and labels_hold(E, labels, table, n)
    pre, c = filtered(E, (65, 0), 3, 0.0, n)
    assert same(pre.distance(c, filt), table)
    assert same(pre.distance_query([0], c, filt), query_rows(table, [0], n))
    assert same(pre.distance_select_prefiltered(c, filt, max_snps=1e9)[0]["d"], table)
    assert pre.distance_banded_prefiltered(c, filt, cluster_snps=cs, cluster_mismatches=cm)[0].tolist() == labels.tolist()
    ptr, wpr, _ = pre.distance_planes(filt)
    assert same(E.planes_distance(ptr, n, wpr, filt, c, 0, n, ctx=pre.ctx), table)
