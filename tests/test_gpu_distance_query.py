"""skx_array_distance_query / skx_array_distance_query_filtered / skh_distance_query_tsv (`-m gpu`), through skx_engine.py against the
oracle's table.  The shapes sit on the edges of the kernels involved: 64-slot tiles of the 4-plane pair sweep and 32-slot tiles of the
8-plane one (S = 70: one full tile and a ragged one, S = 130: two and a ragged one), 8 samples per workgroup of the plane builders (query
counts on both sides of 8 and of the tile sides), 8 plane words per staging step (at least 1 100 kept rows: more than two steps).  Every
number is compared as the table prints it, the suite's bar for distances."""
import math

import numpy as np
import pytest
from conftest import set_knob

import ora

pytestmark = pytest.mark.gpu

FMT = "%s\t%s\t%.2f\t%.5f\t%d\t%d"           # the table's line (VariantDist's Display, merge_ska_array.rs:57-65)
HEADER = "Sample1\tSample2\tDistance\tMismatches (proportion)\tMatch count\tMismatch count"
MIN_FREQS = (0.0, 0.6)


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def _samples(S, seed):
    """one ancestor, point mutations per sample, every other sample truncated (missing rows: the tail is held by half of the samples, below
    a min_freq of 0.6); each sample's second record is a copy of one of its own windows with a few bases changed, so the k-mers whose middle
    base those are carry an ambiguity code in that sample"""
    rng = np.random.default_rng(seed)
    L = 8000
    anc = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L)
    out = []
    for i in range(S):
        s = anc.copy()
        for p in rng.integers(600, L, size=40):                     # (the first 600 bases stay as they are in every sample: constant rows at any k)
            s[p] = b"ACGT"[rng.integers(0, 4)]
        if i % 2:
            s = s[: int(L * 0.7) - 11 * i]
        w0 = int(rng.integers(600, 4000))
        win = s[w0:w0 + 600].copy()
        for p in range(60, len(win), 90):
            win[p] = b"ACGT"[(b"ACGT".index(int(win[p])) + 1 + int(rng.integers(0, 3))) % 4]
        out.append([s.tobytes(), win.tobytes()])
    return out


def _build(E, samples, k):
    names = [f"s{i}" for i in range(len(samples))]
    return E.DictSet.build([E.record_stream(r) for r in samples], k, True).merge(names)


def _oracle_tables(samples, k):
    """{(min_freq, filt_ambig): {(name1, name2): line}} and the tables' line order"""
    names = [f"s{i}" for i in range(len(samples))]
    dicts = []
    for recs in samples:
        d = ora.Dict.new(k, True)
        for r in recs:
            d.add_record(r)
        dicts.append(d)
    tables = {}
    for mf in MIN_FREQS:
        for filt in (True, False):
            text = ora.Array.from_dicts(dicts, names).distance_tsv(min_freq=mf, filt_ambig=filt).decode()
            lines = text.splitlines()
            assert lines[0] == HEADER and len(lines) == 1 + len(names) * (len(names) - 1) // 2
            tables[(mf, filt)] = lines[1:]
    return tables


def _query_sets(S, seed):
    """spread over the whole index range, the last sample in each, in no particular order"""
    rng = np.random.default_rng(seed)
    sets = [[S - 1], [0, S - 1]]
    for q in (7, 9, 33, 65):
        sets.append(sorted(set(np.rint(np.linspace(0, S - 1, q)).astype(int).tolist())))
        assert len(sets[-1]) == q and sets[-1][-1] == S - 1 and sets[-1][0] == 0
    sets.append([i for i in range(S) if i != S // 3])
    sets.append(list(range(S)))
    assert [len(x) for x in sets] == [1, 2, 7, 9, 33, 65, S - 1, S]
    return [[int(x) for x in rng.permutation(s)] for s in sets]


def _lines(names, query, out):
    """{(name_i, name_j) with i < j: the table's line} of a query result"""
    got = {}
    for q, row in zip(query, out):
        assert row[q].tobytes() == bytes(out.dtype.itemsize), "the entry of the query against itself is zeroed"
        for j in range(len(names)):
            if j == q:
                continue
            a, b = min(q, j), max(q, j)
            line = FMT % (names[a], names[b], row["distance"][j], row["mismatch_prop"][j], row["match_count"][j], row["mismatch_count"][j])
            assert got.setdefault((a, b), line) == line, "a pair of two queries is the same from both sides"
    return got


def _expected(table, S, query):
    """the oracle's lines that name a query, keyed like _lines (the table is in pair order: first sample ascending, then second)"""
    qs, want, n = set(query), {}, 0
    for i in range(S):
        for j in range(i + 1, S):
            if i in qs or j in qs:
                want[(i, j)] = table[n]
            n += 1
    return want


@pytest.fixture(scope="module", params=[(70, 9), (70, 41), (130, 9), (130, 41)], ids=lambda p: f"S{p[0]}-k{p[1]}")
def case(request, E):
    S, k = request.param
    samples = _samples(S, 1000 * S + k)
    return {"S": S, "k": k, "samples": samples, "tables": _oracle_tables(samples, k), "arr": _build(E, samples, k), "sets": _query_sets(S, S + k),
            "names": [f"s{i}" for i in range(S)]}


def _hand_filtered(E, case, mf):
    """generic_modes::distance's two filters applied to a copy of the array -> (array, constant sites)"""
    a = _build(E, case["samples"], case["k"])
    if mf * case["S"] >= 1.0:
        a.filter(math.ceil(case["S"] * mf), False, E.FILTER_NONE, False, False, True)
    return a, a.filter(0, False, E.FILTER_NO_CONST, False, False, True)


def test_preconditions(E, case):
    """the inputs reach what the comparison is meant to cover: enough kept rows for several staging steps, both filters biting, and for the
    --allow-ambiguous sweep kept rows with and without an ambiguous cell (the 4-plane and the 8-plane half of the split)"""
    arr, used = case["arr"], {}
    for mf in MIN_FREQS:
        _, _, rows = arr.distance_query_filtered([0], mf, True)
        hand, _ = _hand_filtered(E, case, mf)
        _, var, _ = hand.export()
        assert rows == var.shape[0] >= 1100
        amb = ~np.isin(var, np.frombuffer(b"-ACGT", np.uint8)).reshape(var.shape)
        assert amb.any(axis=1).any() and (~amb.any(axis=1)).any()
        used[mf] = rows
        hand.free()
    assert used[0.6] < used[0.0] < arr.nrows


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_query_rows_equal_the_oracles_lines(E, case, filt):
    arr, S, names = case["arr"], case["S"], case["names"]
    for mf in MIN_FREQS:
        table = case["tables"][(mf, filt)]
        for query in case["sets"]:
            out, _, rows = arr.distance_query_filtered(query, mf, filt)
            assert out.shape == (len(query), S) and rows >= 1100
            got, want = _lines(names, query, out), _expected(table, S, query)
            assert got.keys() == want.keys()
            bad = [(p, got[p], want[p]) for p in want if got[p] != want[p]]
            assert not bad, (mf, len(query), len(bad), bad[:3])


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_query_tsv_of_a_file(E, case, filt, tmp_path):
    """skh_distance_query_tsv: the header and the oracle's lines that name a query, in the table's order"""
    arr, S, names = case["arr"], case["S"], case["names"]
    path = str(tmp_path / "q.skf")
    arr.save(path)
    for mf in MIN_FREQS:
        table = case["tables"][(mf, filt)]
        for query in (case["sets"][2], case["sets"][5]):
            text = arr.ctx.distance_query_tsv(path, [names[q] for q in query] + [names[query[0]]], min_freq=mf, filt_ambig=filt).decode()
            want = _expected(table, S, query)
            assert text == "\n".join([HEADER] + [want[p] for p in sorted(want)]) + "\n", (mf, len(query))


def test_hand_filtered_array_gives_the_same_rows(E, case):
    arr = case["arr"]
    for mf in MIN_FREQS:
        hand, constant = _hand_filtered(E, case, mf)
        for filt in (True, False):
            for query in (case["sets"][1], case["sets"][4]):
                want, c, _ = arr.distance_query_filtered(query, mf, filt)
                assert c == constant
                assert hand.distance_query(query, constant, filt).tobytes() == want.tobytes(), (mf, filt, len(query))
        hand.free()


def test_all_rows_through_the_twelve_class_sweep(E, case, monkeypatch):
    """SKX_KNOBS=stale_row_mask: the row statistics are taken to claim that no kept row holds an ambiguous cell, the check of the 4-plane
    planes finds that they do, and every row goes through the 8-plane sweep -- same numbers"""
    arr = case["arr"]
    queries = (case["sets"][3], case["sets"][6])
    want = [arr.distance_query_filtered(q, 0.6, False)[0].tobytes() for q in queries]
    set_knob(monkeypatch, "stale_row_mask", 1)
    assert [arr.distance_query_filtered(q, 0.6, False)[0].tobytes() for q in queries] == want


def test_repeatable_and_the_array_stays(E, case):
    arr, query = case["arr"], case["sets"][4]
    before = arr.export()
    for filt in (True, False):
        a = arr.distance_query_filtered(query, 0.6, filt)[0].tobytes()
        assert arr.distance_query_filtered(query, 0.6, filt)[0].tobytes() == a
        b = arr.distance_query(query, 3.0, filt).tobytes()
        assert arr.distance_query(query, 3.0, filt).tobytes() == b
    assert all(np.array_equal(x, y) for x, y in zip(arr.export(), before))


def test_refusals(E, case):
    arr, S = case["arr"], case["S"]
    for bad in ([S], [-1], [0, S - 1, 0], []):
        for call in (lambda q: arr.distance_query(q), lambda q: arr.distance_query_filtered(q)):
            with pytest.raises(E.EngineError) as e:
                call(bad)
            assert e.value.code == E.EINVAL and "distance query" in str(e.value), (bad, str(e.value))
