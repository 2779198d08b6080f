"""skx_array_distance_mst / skh_distance_mst_tsv / skh_mst_levels_csv (`-m gpu`), through skx_engine.py, against the forest model
(tests/mst_model.py) applied to the float64 values of the full table (Array.distance_filtered on the same array, whose printed form the
existing tests pin to the oracle).  The shapes sit on the pair sweep's tile edges (64-slot tiles of the 4-plane sweep, 32-slot tiles of the
8-plane one: S = 70 and 130), the samples come in clades with duplicate founders, so that distance-0 ties are everywhere and the
(distance, i, j) rule decides, and the thresholds are values of the table itself.  What is compared: the set of (i, j), their ascending
order, and every pair's skx_dist byte for byte against the table's entry."""
import math

import numpy as np
import pytest
from conftest import set_knob

from mst_model import boruvka, candidates, components, kruskal, levels, mst, mst_streamed

pytestmark = pytest.mark.gpu

FMT = "%s\t%s\t%.2f\t%.5f\t%d\t%d"
HEADER = "Sample1\tSample2\tDistance\tMismatches (proportion)\tMatch count\tMismatch count"
MIN_FREQS = (0.0, 0.6)
BAND = 64
PLANTED = (65, 66, 10, 30, 68)        # where the fourth clade sits after the shuffle (samples)
# (S, k, bases a sample, seed): at k = 9 a shorter sequence, because two of its 9-mers meet in a split k-mer by chance about L^2 / 65 536 times
# and every such cell is an ambiguous one; the seeds are ones at which every table meets test_preconditions
SHAPES = [(70, 9, 2400, 70011), (130, 9, 2400, 130010), (70, 41, 6000, 70042)]


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def samples(S, seed, L=6000, n_lineage=60, n_founder=8):
    """one ancestor, two lineages 60 point mutations away from it each (in the part every sample keeps), and in them, alternating, clades of
    five consecutive samples: a founder (the lineage with 8 mutations), members 0 and 1 equal to it (duplicates: distance 0, ties wherever a clade is joined), members
    2-4 with 1-3 mutations of their own.  Every third sample is truncated (missing rows, the tail below a min_freq of 0.6); each sample's
    second record is a window of itself with a base changed every 90 (the ambiguous cells).  The order is then shuffled with a seeded
    permutation, so that the members of a clade sit in different bands of the pair matrix, and the fourth clade is moved to the places 65,
    66 (its two copies of the founder), 10, 30 and 68: the first band (i < 64) joins 65 and 66 through lines that the second band's line
    between the two displaces.
    Lines within a clade, between clades of a lineage and between lineages are three scales of distance: the 30 % quantile lies below the
    third, and a single band needs a round for each."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    anc = rng.choice(acgt, size=L)

    shared = int(L * 0.7) - L // 900 * S                           # what the shortest sample still has

    def mutate(s, n, end=L):
        for p in rng.integers(600, end, size=n):                   # (the first 600 bases stay: constant rows at any k)
            s[p] = b"ACGT"[(b"ACGT".index(int(s[p])) + 1 + int(rng.integers(0, 3))) % 4]

    lineage = [anc.copy(), anc.copy()]
    for s in lineage:
        mutate(s, n_lineage, shared)
    out, founder = [], None
    for i in range(S):
        if i % 5 == 0:
            founder = lineage[(i // 5) % 2].copy()
            mutate(founder, n_founder)
        s = founder.copy()
        if i % 5 >= 2:
            mutate(s, i % 5 - 1)
        if i % 3 == 0:
            s = s[: int(L * 0.7) - L // 900 * i]
        w0 = int(rng.integers(600, len(s) - 400))
        win = s[w0:w0 + 400].copy()
        for p in range(60, len(win), 90):
            win[p] = b"ACGT"[(b"ACGT".index(int(win[p])) + 1 + int(rng.integers(0, 3))) % 4]
        out.append([s.tobytes(), win.tobytes()])
    order = [int(p) for p in np.random.default_rng(S).permutation(S)]
    for member, place in zip(range(15, 20), PLANTED):
        at = order.index(member)
        order[at], order[place] = order[place], order[at]
    return [out[p] for p in order]


def _pair_index(S, i, j):
    return i * (2 * S - i - 1) // 2 + (j - i - 1)


def _matrices(table, S):
    D, M = np.zeros((S, S)), np.zeros((S, S))
    iu = np.triu_indices(S, 1)                                      # row-major (i < j): the table's order
    D[iu], M[iu] = table["distance"], table["mismatch_prop"]
    return D + D.T, M + M.T


def preconditions(S, D, M, snps, mism):
    """what the generator is for, asserted on the model alone (D, M: a full table as lists; snps, mism: its 30 % quantile values)"""
    forest = mst(D, M)
    cand = candidates(D, M)
    assert kruskal(S, sorted(cand, key=lambda e: (e[0], -e[1], -e[2]))) != forest                      # the tie rule decides
    for crit in ({"max_snps": snps}, {"max_mismatches": mism}, {"max_snps": snps, "max_mismatches": mism}):
        assert 2 <= S - len(mst(D, M, **crit)) < S, crit                                               # a forest of several trees
    first, _ = boruvka(S, [e for e in cand if e[1] < BAND])
    assert {(i, j) for _, i, j in first} - forest                                                      # a later band displaces a line of the first
    assert mst_streamed(D, M, S)[1] >= 3


@pytest.fixture(scope="module", params=SHAPES, ids=lambda p: f"S{p[0]}-k{p[1]}")
def case(request, E):
    S, k, L, seed = request.param
    names = [f"s{i}" for i in range(S)]
    arr = E.DictSet.build([E.record_stream(r) for r in samples(S, seed, L)], k, True).merge(names)
    ref = {}
    for mf in MIN_FREQS:
        for filt in (True, False):
            table, constant, rows = arr.distance_filtered(mf, filt)
            D, M = _matrices(table, S)
            P = len(table)
            sd, sm = np.sort(table["distance"]), np.sort(table["mismatch_prop"])
            ranks = (math.ceil(0.02 * P), math.ceil(0.3 * P))
            ref[(mf, filt)] = {"table": table.copy(), "constant": constant, "rows": rows, "D": D.tolist(), "M": M.tolist(),
                               "snps": [float(sd[r - 1]) for r in ranks], "mism": [float(sm[r - 1]) for r in ranks],
                               "above": (float(sd[-1]) + 1.0, 1.0), "forest": {}}
    return {"S": S, "k": k, "names": names, "arr": arr, "ref": ref}


def _model(r, **criteria):
    """the model's forest of a table under the criteria, computed once"""
    key = tuple(sorted(criteria.items()))
    if key not in r["forest"]:
        r["forest"][key] = sorted(mst(r["D"], r["M"], **criteria))
    return r["forest"][key]


def _check(case, mf, filt, band_rows=0, **criteria):
    """one call against the model; -> (pairs, info)"""
    S, r = case["S"], case["ref"][(mf, filt)]
    pairs, constant, rows, info = case["arr"].distance_mst(mf, filt, band_rows=band_rows, **criteria)
    assert (constant, rows) == (r["constant"], r["rows"])
    want = _model(r, **criteria)
    got = list(zip(pairs["i"].tolist(), pairs["j"].tolist()))
    assert got == want, (mf, filt, band_rows, criteria, len(got), len(want), sorted(set(got) ^ set(want))[:5])
    idx = [_pair_index(S, i, j) for i, j in want]
    assert pairs["d"].tobytes() == r["table"][idx].tobytes(), (mf, filt, band_rows, criteria)
    assert info["edges"] == len(want) and info["edges"] + info["components"] == S
    return pairs, info


def test_preconditions(case):
    """the inputs reach what the comparisons are meant to cover (asserted on the model side: the test fails if they do not)"""
    for (mf, filt), r in case["ref"].items():
        assert r["rows"] >= 1100
        preconditions(case["S"], r["D"], r["M"], r["snps"][1], r["mism"][1])
    assert case["ref"][(0.6, True)]["rows"] < case["ref"][(0.0, True)]["rows"]


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_forest_and_thresholds(case, filt):
    S = case["S"]
    for mf in MIN_FREQS:
        r = case["ref"][(mf, filt)]
        _, info = _check(case, mf, filt)
        assert info["candidates"] == S * (S - 1) // 2 and info["bands"] == 1 and info["rounds"] >= 2
        assert info["rounds"] == mst_streamed(r["D"], r["M"], S)[1]
        for v in [0.0] + r["snps"] + [r["above"][0]]:
            _check(case, mf, filt, max_snps=v)
        for v in [0.0] + r["mism"] + [r["above"][1]]:
            _check(case, mf, filt, max_mismatches=v)
        pairs, info = _check(case, mf, filt, max_snps=r["snps"][1], max_mismatches=r["mism"][1])
        assert info["candidates"] == len(candidates(r["D"], r["M"], max_snps=r["snps"][1], max_mismatches=r["mism"][1])) and 2 <= info["components"] < S
        _check(case, mf, filt, max_snps=r["snps"][0], max_mismatches=r["mism"][1], band_rows=BAND)


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_band_rows(case, filt):
    S, r = case["S"], case["ref"][(0.6, filt)]
    for band in (0, 64, 50, 1, S, 1000):
        for crit in ({}, {"max_snps": r["snps"][1]}, {"max_snps": r["snps"][1], "max_mismatches": r["mism"][1]}):
            _, info = _check(case, 0.6, filt, band_rows=band, **crit)
            if band:
                assert info["bands"] == math.ceil(S / band) and info["band_rows"] == min(band, S)
            else:
                assert info["bands"] == 1
            assert info["count_buffer_bytes"] == info["band_rows"] * S * 128 <= 1 << 30
            if band in (64, 50, S):
                assert info["rounds"] == mst_streamed(r["D"], r["M"], band, **crit)[1], (band, crit)


def test_repeatable_and_the_array_stays(case):
    arr, r = case["arr"], case["ref"][(0.6, False)]
    before = arr.export()
    for filt in (True, False):
        for crit in ({}, {"max_snps": r["snps"][1], "band_rows": BAND}):
            a = arr.distance_mst(0.6, filt, **crit)
            b = arr.distance_mst(0.6, filt, **crit)
            assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    assert all(np.array_equal(x, y) for x, y in zip(arr.export(), before))


def test_all_rows_through_the_twelve_class_sweep(case, monkeypatch):
    """SKX_KNOBS=stale_row_mask: every row goes through the 8-plane sweep -- same pairs"""
    r = case["ref"][(0.6, False)]
    crits = ({}, {"max_snps": r["snps"][1], "max_mismatches": r["mism"][1], "band_rows": BAND})
    want = [case["arr"].distance_mst(0.6, False, **c)[0].tobytes() for c in crits]
    set_knob(monkeypatch, "stale_row_mask", 1)
    assert [_check(case, 0.6, False, **c)[0].tobytes() for c in crits] == want


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_mst_tsv_of_a_file(case, filt, tmp_path):
    """skh_distance_mst_tsv: the header and the model's lines, in the table's order and text"""
    arr, S, names = case["arr"], case["S"], case["names"]
    path = str(tmp_path / "s.skf")
    arr.save(path)
    for mf in MIN_FREQS:
        r = case["ref"][(mf, filt)]
        for crit in ({}, {"max_snps": r["snps"][1]}, {"max_mismatches": r["mism"][0]}):
            t = r["table"]
            lines = [FMT % (names[i], names[j], t["distance"][n], t["mismatch_prop"][n], t["match_count"][n], t["mismatch_count"][n])
                     for i, j in _model(r, **crit) for n in [_pair_index(S, i, j)]]
            assert arr.ctx.distance_mst_tsv(path, mf, filt, **crit).decode() == "\n".join([HEADER] + lines) + "\n", (mf, crit)


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_prefiltered_array(E, case, filt):
    """skx_array_distance_mst_prefiltered (what skh_distance_mst_tsv calls after the one-pass filtered load): every row swept, the constant as
    given -- against the model on skx_array_distance's table of the same array and constant"""
    arr, S = case["arr"], case["S"]
    for constant in (0, 17):
        table = arr.distance(float(constant), filt)
        D, M = _matrices(table, S)
        sd, sm = np.sort(table["distance"]), np.sort(table["mismatch_prop"])
        snps, mism = float(sd[math.ceil(0.3 * len(sd)) - 1]), float(sm[math.ceil(0.3 * len(sm)) - 1])
        for crit in ({}, {"max_snps": snps}, {"max_mismatches": mism, "band_rows": BAND}, {"max_snps": snps, "max_mismatches": mism, "band_rows": 50}):
            want = sorted(mst(D.tolist(), M.tolist(), **{k: v for k, v in crit.items() if k != "band_rows"}))
            pairs, info = arr.distance_mst_prefiltered(constant, filt, **crit)
            assert 0 < len(want) < len(table) and list(zip(pairs["i"].tolist(), pairs["j"].tolist())) == want, (constant, crit)
            assert pairs["d"].tobytes() == table[[_pair_index(S, i, j) for i, j in want]].tobytes(), (constant, crit)
            assert info["bands"] == math.ceil(S / crit.get("band_rows", S)) and info["edges"] + info["components"] == S
    with pytest.raises(E.EngineError) as e:
        arr.distance_mst_prefiltered(-1, filt)
    assert e.value.code == E.EINVAL and "distance mst:" in str(e.value)


def test_refusals(E, case):
    nan = float("nan")
    for crit in ({"max_snps": nan}, {"max_mismatches": nan}, {"max_mismatches": 1.5}, {"band_rows": -1}):
        with pytest.raises(E.EngineError) as e:
            case["arr"].distance_mst(0.0, True, **crit)
        assert e.value.code == E.EINVAL and "distance mst:" in str(e.value), (crit, str(e.value))


def test_levels(E, case):
    """skh_mst_levels_csv is the model's text, and every level's partition is the single-linkage one of the banded clusters at that threshold"""
    arr, S, names = case["arr"], case["S"], case["names"]
    for (mf, filt) in ((0.0, True), (0.6, False)):
        r = case["ref"][(mf, filt)]
        pairs, _, _, _ = arr.distance_mst(mf, filt)
        top = math.ceil(r["above"][0])
        ladder = [top, r["snps"][1], 2.5, float(math.floor(r["snps"][0])), 0]
        ladder = [x for n, x in enumerate(ladder) if x not in ladder[:n]]
        columns, csv = levels(r["D"], r["M"], _model(r), ladder, names)
        assert E.mst_levels_csv(names, pairs, ladder) == csv
        assert len(set(columns[0])) == 1 and 2 <= len(set(columns[1])) < len(set(columns[-1])) <= S
        assert len(set(columns[-1])) < S or not filt                                           # (the copies of a founder are at 0 by default)
        for L, col in zip(ladder, columns):
            labels, _, _, _, _ = arr.distance_banded(mf, filt, labels=True, cluster_snps=L, cluster_mismatches=1.0)
            roots = sorted(set(labels.tolist()))
            assert col == [roots.index(x) + 1 for x in labels.tolist()], (mf, filt, L)
    # names that need quotes, and a forest of several trees
    odd = ['a,b', 'c"d', "e"]
    three = np.zeros(1, E.PAIR_DT)
    three["i"], three["j"], three["d"]["distance"] = 0, 2, 1.004
    assert E.mst_levels_csv(odd, three, [1, 0.5]) == 'id,snps_1,snps_0.5,address\n"a,b",1,1,1.1\n"c""d",2,2,2.2\ne,1,3,1.3\n'
    with pytest.raises(E.EngineError):
        bad = three.copy()
        bad["j"] = 3
        E.mst_levels_csv(odd, bad, [1])


def _samples_small(n, seed=7):
    rng = np.random.default_rng(seed)
    base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=300)
    recs = []
    for i in range(n):
        s = base.copy()
        for p in rng.integers(20, 280, size=int(rng.integers(0, 3))):                  # 0-2 mutations: many equal distances
            s[p] = b"ACGT"[(b"ACGT".index(int(s[p])) + 1 + int(rng.integers(0, 3))) % 4]
        recs.append(s.tobytes())
    return recs


def test_small_arrays(E):
    """one sample: no pair; two: the one line, or none below it; 65 samples in bands of 64: a second band of one row"""
    recs = _samples_small(65)
    one = E.DictSet.build([E.record_stream([recs[0]])], 9, True).merge(["only"])
    pairs, _, _, info = one.distance_mst(0.0, True)
    assert len(pairs) == 0 and (info["edges"], info["components"]) == (0, 1)
    far = bytearray(recs[0])
    far[100] = b"ACGT"[(b"ACGT".index(far[100]) + 1) % 4]
    two = E.DictSet.build([E.record_stream([recs[0]]), E.record_stream([bytes(far)])], 9, True).merge(["x", "y"])
    table, _, _ = two.distance_filtered(0.0, True)
    assert table["distance"][0] >= 1.0
    pairs, _, _, info = two.distance_mst(0.0, True)
    assert len(pairs) == 1 and (pairs["i"][0], pairs["j"][0]) == (0, 1) and pairs["d"].tobytes() == table.tobytes() and info["rounds"] == 1
    pairs, _, _, info = two.distance_mst(0.0, True, max_snps=float(table["distance"][0]) - 0.5)
    assert len(pairs) == 0 and (info["candidates"], info["components"], info["rounds"]) == (0, 2, 0)
    arr = E.DictSet.build([E.record_stream([x]) for x in recs], 9, True).merge([f"t{n}" for n in range(65)])
    table, _, _ = arr.distance_filtered(0.0, True)
    D, M = _matrices(table, 65)
    for crit in ({}, {"max_snps": 1.0}):
        pairs, _, _, info = arr.distance_mst(0.0, True, band_rows=64, **crit)
        want = sorted(mst(D.tolist(), M.tolist(), **crit))
        assert list(zip(pairs["i"].tolist(), pairs["j"].tolist())) == want and (info["bands"], info["band_rows"]) == (2, 64)
        assert pairs["d"].tobytes() == table[[_pair_index(65, i, j) for i, j in want]].tobytes()


def _mst_columns(S, i, j, d, keep):
    """mst_model.mst on the table's columns with numpy, for tables too long for the plain model: Kruskal over the kept lines in the stable order
    of (distance, place in the table) -> indices of the forest's lines, ascending"""
    idx = np.flatnonzero(keep)
    idx = idx[np.argsort(d[idx], kind="stable")]
    up = list(range(S))
    out = []
    for n, a, b in zip(idx.tolist(), i[idx].tolist(), j[idx].tolist()):
        while up[a] != a:
            up[a] = up[up[a]]
            a = up[a]
        while up[b] != b:
            up[b] = up[up[b]]
            b = up[b]
        if a != b:
            up[max(a, b)] = min(a, b)
            out.append(n)
            if len(out) == S - 1:
                break
    return np.sort(np.array(out, dtype=np.int64))


def test_the_engines_own_band_choice_with_two_bands(E):
    """band_rows = 0 where one band's counters would pass 1 GiB: S = 2 900 gives 2 880 first samples a band and a second band of 20; against the
    full table through the numpy form of the model, which is first held against the model itself on a small table full of ties"""
    rng = np.random.default_rng(3)
    S0 = 40
    i0, j0 = np.triu_indices(S0, 1)
    d0, m0 = rng.integers(0, 4, len(i0)).astype(float), rng.integers(0, 5, len(i0)) / 4
    D0, M0 = np.zeros((S0, S0)), np.zeros((S0, S0))
    D0[i0, j0], M0[i0, j0] = d0, m0
    for crit, keep in (({}, np.ones(len(d0), bool)), ({"max_snps": 1.0}, d0 <= 1.0), ({"max_snps": 0.0, "max_mismatches": 0.0}, (d0 <= 0.0) & (m0 <= 0.0))):
        k = _mst_columns(S0, i0, j0, d0, keep)
        assert set(zip(i0[k].tolist(), j0[k].tolist())) == mst((D0 + D0.T).tolist(), (M0 + M0.T).tolist(), **crit), crit
    S = 2900
    arr = E.DictSet.build([E.record_stream([x]) for x in _samples_small(S, seed=11)], 9, True).merge([f"t{n}" for n in range(S)])
    table, constant, rows = arr.distance_filtered(0.0, True)
    i, j = np.triu_indices(S, 1)
    d, m = table["distance"], table["mismatch_prop"]
    third = float(np.sort(m)[len(m) // 3])
    for crit, keep in (({}, np.ones(len(d), bool)), ({"max_snps": 1.0, "max_mismatches": third}, (d <= 1.0) & (m <= third))):
        pairs, c, n_rows, info = arr.distance_mst(0.0, True, **crit)
        assert (c, n_rows) == (constant, rows)
        assert (info["bands"], info["band_rows"]) == (2, 2880) and info["count_buffer_bytes"] == 2880 * S * 128 <= 1 << 30
        k = _mst_columns(S, i, j, d, keep)
        assert 0 < len(k) == info["edges"] == S - info["components"]
        assert np.array_equal(pairs["i"], i[k]) and np.array_equal(pairs["j"], j[k]) and pairs["d"].tobytes() == table[k].tobytes(), crit
    arr.free()
