"""skx_array_pair_sites (`-m gpu`), through skx_engine.py, against tests/sites_model.py (held against the oracle and the committed tables by
tests/test_sites_model.py on the CPU).  Arrays made with Array.from_host from rows given in ascending key order keep that order, so the records
must be the model's one for one: pair, row, the two bases, the split k-mer.  Arrays of another provenance (a loaded file, a lazily held build)
have a row order of their own: there a record is identified by (pair, split k-mer), and the device's own order -- ascending (pair, row), every
one once -- is checked besides.  Every random case asserts that the model itself lists something, so an engine that returns nothing cannot pass."""
import os

import numpy as np
import pytest
from conftest import set_knob

import sites_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b"ACGT", np.uint8)
AMBIG = np.frombuffer(b"MRWSYKVHDBN", np.uint8)


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def _matrix(S, U, seed, differ=0.2, gaps=0.1, ambiguous=0.05):
    """a base per row, a share of the cells another base, gaps and IUPAC codes (N among them) -> (ascending keys, [U, S] cells)"""
    rng = np.random.default_rng(seed)
    lo = np.unique(rng.integers(1 << 33, 1 << 59, size=U + 64, dtype=np.uint64))[:U]
    assert len(lo) == U
    var = np.repeat(ACGT[rng.integers(0, 4, size=(U, 1))], S, axis=1)
    hit = rng.random((U, S)) < differ
    var[hit] = ACGT[rng.integers(0, 4, size=int(hit.sum()))]
    var[rng.random((U, S)) < gaps] = ord("-")
    hit = rng.random((U, S)) < ambiguous
    var[hit] = AMBIG[rng.integers(0, len(AMBIG), size=int(hit.sum()))]
    return lo, var


def _from_host(E, lo, var, k=31):
    keys = np.zeros(len(lo), E.KEY_DT)
    keys["lo"] = lo
    return E.Array.from_host(k, True, [f"s{i:03d}" for i in range(var.shape[1])], keys, var), keys


def _check(arr, keys, var, pairs, min_freq=0.0, want_keys=True, nonempty=True, where=None):
    """one call against the model, record for record -> the records"""
    pairs = [tuple(p) for p in pairs]
    rec, rkeys, counts = arr.pair_sites(pairs, min_freq=min_freq, keys=want_keys)
    want = SM.sites(var, SM.sweep_flags(var, min_freq), pairs)
    where = (where, min_freq, len(rec), len(want))
    if nonempty:
        assert len(want) > 0, where
    assert len(rec) == len(want), where
    for f in ("pair", "row", "base_i", "base_j"):
        assert np.array_equal(rec[f], want[f]), (where, f)
    assert not rec["reserved"].any(), where
    assert np.array_equal(counts.astype(np.int64), SM.counts_of(want, len(pairs))), where
    if want_keys:
        assert np.array_equal(rkeys, keys[want["row"].astype(np.int64)]), where
    else:
        assert rkeys is None
    return rec


# ---- row edges: the lane's 16 rows, the wave's 1 024, the chunk's 4 096 ----
@pytest.mark.parametrize("S", [2, 3, 65])
@pytest.mark.parametrize("U", [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_row_edges(E, U, S):
    lo, var = _matrix(S, U, 1000 * S + U)
    if U:                                                               # the last row is a site of the last pair whatever the draw
        var[U - 1, :] = ord("A")
        var[U - 1, S - 1] = ord("C")
    arr, keys = _from_host(E, lo, var)
    pairs = SM.all_pairs(S) if S < 65 else [(0, 64), (63, 64), (1, 2), (31, 33), (0, 1), (62, 64)]
    rec = _check(arr, keys, var, pairs, nonempty=U >= 16, where=(U, S))
    if U:
        assert int(rec["row"].max()) == U - 1
    if U >= 16:
        _check(arr, keys, var, pairs[::-1], min_freq=0.7, where=(U, S, "min_freq"))
    assert all(np.array_equal(x, y) for x, y in zip(arr.export()[:2], (keys, var)))          # the array keeps its content


# ---- pair edges ----
@pytest.fixture(scope="module")
def small(E):
    lo, var = _matrix(9, 5000, 77)
    var[:, 4] = var[:, 2]                                               # two identical samples
    arr, keys = _from_host(E, lo, var)
    return arr, keys, var


def test_no_pair(small):
    arr, keys, var = small
    rec, rkeys, counts = arr.pair_sites(np.zeros((0, 2), np.uint32))
    assert len(rec) == 0 and len(rkeys) == 0 and len(counts) == 0


def test_every_pair(small):
    arr, keys, var = small
    _check(arr, keys, var, SM.all_pairs(9))


def test_one_pair_twice_and_descending_order(small):
    arr, keys, var = small
    rec = _check(arr, keys, var, [(1, 5), (0, 3), (1, 5)])
    runs = [rec[rec["pair"] == p] for p in range(3)]
    assert len(runs[0]) > 0 and np.array_equal(runs[0]["row"], runs[2]["row"])                # two runs of records
    _check(arr, keys, var, SM.all_pairs(9)[::-1])


def test_identical_samples_give_nothing_and_harm_nobody(small):
    arr, keys, var = small
    rec = _check(arr, keys, var, [(1, 2), (2, 4), (3, 4)])
    assert (rec["pair"] == 1).sum() == 0 and (rec["pair"] == 0).sum() > 0 and (rec["pair"] == 2).sum() > 0


def test_more_pairs_than_a_grid_dimension(E):
    S, U = 375, 130
    lo, var = _matrix(S, U, 375)
    arr, keys = _from_host(E, lo, var)
    pairs = SM.all_pairs(S)
    assert len(pairs) == 70125 > 65535
    _check(arr, keys, var, pairs)


# ---- content edges ----
def test_a_pair_that_differs_at_every_row(E):
    U = 70000
    lo, var = _matrix(3, U, 3)
    var[:, 0], var[:, 2] = ord("A"), ord("G")
    arr, keys = _from_host(E, lo, var)
    rec = _check(arr, keys, var, [(0, 1), (0, 2), (1, 2)])
    assert (rec["pair"] == 1).sum() == U > 1 << 16


@pytest.mark.parametrize("cell", ["-", "N"])
def test_a_column_of_one_letter(E, cell):
    lo, var = _matrix(5, 4500, ord(cell))
    var[:, 1] = ord(cell)
    arr, keys = _from_host(E, lo, var)
    rec = _check(arr, keys, var, SM.all_pairs(5))
    assert not np.isin(rec["pair"], [0, 4, 5, 6]).any()                 # (0, 1), (1, 2), (1, 3), (1, 4): nothing to compare


def test_frequency_threshold(E):
    S, U = 10, 4200
    lo, var = _matrix(S, U, 10, gaps=0.0)
    planted = np.arange(0, U, 7)
    var[planted] = ord("-")                                             # four samples present, and the pair (0, 1) differs
    var[planted, 0], var[planted, 1], var[planted, 2], var[planted, 3] = ord("A"), ord("C"), ord("A"), ord("A")
    arr, keys = _from_host(E, lo, var)
    all_rows = _check(arr, keys, var, [(0, 1), (2, 5)], min_freq=0.0)
    half = _check(arr, keys, var, [(0, 1), (2, 5)], min_freq=0.5)
    assert np.isin(planted, all_rows["row"][all_rows["pair"] == 0]).all()
    assert not np.isin(half["row"], planted).any() and len(half) > 0
    _check(arr, keys, var, [(0, 1), (2, 5)], min_freq=0.05)             # below one sample: no threshold (0.05 * 10 < 1)
    _check(arr, keys, var, [(0, 1), (2, 5)], min_freq=1.0, nonempty=False)


# ---- counts against the engine's own distances ----
@pytest.mark.parametrize("min_freq", [0.0, 0.6])
def test_counts_are_the_engines_distances(small, min_freq):
    arr, keys, var = small
    pairs, _, _, _ = arr.distance_select(min_freq=min_freq, max_snps=1e18)
    assert len(pairs) == 36
    ij = np.stack([pairs["i"], pairs["j"]], axis=1)
    _, _, counts = arr.pair_sites(ij, min_freq=min_freq, keys=False)
    assert np.array_equal(counts.astype(np.float64), pairs["d"]["distance"]) and counts.sum() > 0


# ---- max_records ----
def test_max_records(small, E):
    arr, keys, var = small
    pairs = [(0, 1), (2, 4), (5, 8)]
    want = SM.sites(var, SM.sweep_flags(var, 0.0), pairs)
    total = len(want)
    assert total > 1
    rec, _, _ = arr.pair_sites(pairs, max_records=total)
    assert len(rec) == total
    with pytest.raises(E.EngineError) as ei:
        arr.pair_sites(pairs, max_records=total - 1)
    assert ei.value.code == E.ENOMEM and f"pair sites: {total} records; the limit is {total - 1}" in str(ei.value)
    assert np.array_equal(ei.value.counts.astype(np.int64), SM.counts_of(want, 3)) and ei.value.records is None       # counts filled, *records NULL


# ---- the refusals ----
def test_refusals(small, E):
    arr, keys, var = small
    bad = [dict(ij=[(1, 1)]), dict(ij=[(3, 2)]), dict(ij=[(0, 1), (0, 9)]), dict(ij=[(9, 10)]), dict(ij=[(0, 1)], min_freq=-0.1), dict(ij=[(0, 1)], min_freq=1.01),
           dict(ij=[(0, 1)], min_freq=float("nan"))]
    for kw in bad:
        with pytest.raises(E.EngineError) as ei:
            arr.pair_sites(**kw)
        assert ei.value.code == E.EINVAL and "] pair sites:" in str(ei.value), (kw, str(ei.value))
    assert all(np.array_equal(x, y) for x, y in zip(arr.export()[:2], (keys, var)))


# ---- provenance ----
def _check_by_key(arr, pairs, min_freq=0.0, want_keys=True):
    """an array with a row order of its own: the model works on the export (rows ascending by split k-mer), a record is identified by its key"""
    rec, rkeys, counts = arr.pair_sites(pairs, min_freq=min_freq, keys=want_keys)
    ekeys, var, ecounts = arr.export()
    want = SM.sites(var, SM.sweep_flags(var, min_freq, ecounts), pairs)
    assert len(rec) == len(want) > 0
    assert np.array_equal(counts.astype(np.int64), SM.counts_of(want, len(pairs)))
    word = (rec["pair"].astype(np.int64) << 40) | rec["row"].astype(np.int64)
    assert (np.diff(word) > 0).all() and (rec["row"] < len(var)).all() and not rec["reserved"].any()
    if not want_keys:
        assert rkeys is None
        for p in range(len(pairs)):                                     # rows and bases only: the pairs of bases, as multisets
            g, w = rec[rec["pair"] == p], want[want["pair"] == p]
            assert sorted(zip(g["base_i"].tolist(), g["base_j"].tolist())) == sorted(zip(w["base_i"].tolist(), w["base_j"].tolist()))
        return rec
    o = np.lexsort((rkeys["lo"], rkeys["hi"], rec["pair"]))
    for f in ("pair", "base_i", "base_j"):
        assert np.array_equal(rec[f][o], want[f]), f
    assert np.array_equal(rkeys[o], ekeys[want["row"].astype(np.int64)])
    return rec


def test_a_loaded_file_with_128_bit_keys(E):
    arr = E.Array.load(os.path.join(ROOT, "tests", "golden", "input", "merge_k41.skf"))
    assert arr.k_bits == 128
    rec = _check_by_key(arr, [(0, 1)])
    assert len(rec) == 1                                                # the committed table's Distance


def test_a_loaded_file_with_six_samples(E):
    arr = E.Array.load(os.path.join(ROOT, "tests", "golden", "input", "multidist.skf"))
    _check_by_key(arr, SM.all_pairs(6))
    _check_by_key(arr, SM.all_pairs(6)[::-1], min_freq=0.5)


@pytest.mark.parametrize("k", [31, 41])
def test_a_lazily_held_build(E, tmp_path, k):
    rng = np.random.default_rng(k)
    anc = ACGT[rng.integers(0, 4, size=20000)]
    inputs = []
    for i in range(5):
        s = anc.copy()
        pos = rng.integers(0, len(s), size=60)
        s[pos] = ACGT[rng.integers(0, 4, size=60)]
        p = tmp_path / f"s{i}.fa"
        p.write_bytes(b">c\n" + s[: len(s) * (5 - i % 2) // 5].tobytes() + b"\n")
        inputs.append((f"s{i}", str(p), None))
    arr = E.Array.build(inputs, k=k, threads=2)
    pairs = SM.all_pairs(5)
    first = arr.pair_sites(pairs, min_freq=0.5)                         # on the array as the build left it: materialised by the call
    _check_by_key(arr, pairs, min_freq=0.5)
    again = arr.pair_sites(pairs, min_freq=0.5)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))


def test_an_array_without_split_kmers(E, tmp_path, monkeypatch):
    """skx_array_load_filtered steps over the file's split k-mer list: rows and bases only, and the keys are refused"""
    lo, var = _matrix(4, 20000, 4)
    full, keys = _from_host(E, lo, var)
    path = str(tmp_path / "k.skf")
    set_knob(monkeypatch, "skf_device", "1")
    full.save(path)
    arr, removed, _ = E.Array.load_filtered(path, 0.0, False, E.FILTER_NONE, False, False)      # nothing removed: the file's rows, in its order, but no keys
    assert removed == 0 and arr.nrows == len(var)
    with pytest.raises(E.EngineError):
        arr.export()
    pairs = SM.all_pairs(4)
    with pytest.raises(E.EngineError) as ei:
        arr.pair_sites(pairs, keys=True)
    assert ei.value.code == E.EINVAL and "] pair sites:" in str(ei.value)
    _check(arr, keys, var, pairs, want_keys=False)
    _check(arr, keys, var, pairs[::-1], min_freq=0.75, want_keys=False)
