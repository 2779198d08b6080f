"""skx_array_distance_select / skh_distance_select_tsv (`-m gpu`), through skx_engine.py, against the selection model (tests/select_model.py)
applied to the float64 values of the full table (Array.distance_filtered on the same array, whose printed form the existing tests pin to
the oracle).  The shapes sit on the pair sweep's tile edges (64-slot tiles of the 4-plane sweep, 32-slot tiles of the 8-plane one: S = 70
and 130) and the thresholds are values of the table itself, so equality with a pair's own value is exercised.  What is compared: the set of
(i, j), their ascending order, and every pair's skx_dist byte for byte against the table's entry."""
import math

import numpy as np
import pytest
from conftest import set_knob

import sites_model as SM
from select_model import select

pytestmark = pytest.mark.gpu

FMT = "%s\t%s\t%.2f\t%.5f\t%d\t%d"
HEADER = "Sample1\tSample2\tDistance\tMismatches (proportion)\tMatch count\tMismatch count"
MIN_FREQS = (0.0, 0.6)
KS = lambda S: (1, 4, 7, 64, S - 1, S + 5)
BAND = 64
PLANTED = (10, 30, 65, 66, 68)        # where the fourth clade sits after the shuffle (_samples)


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def _samples(S, seed):
    """one ancestor; clades of five consecutive samples: a founder (30 point mutations), members 0 and 1 equal to it (duplicates: distance 0,
    ties at every K), members 2-4 with 1-3 mutations of their own; every third sample truncated (missing rows, the tail below a min_freq
    of 0.6); each sample's second record a window of itself with a base changed every 90 (the ambiguous cells); then the order shuffled
    with a seeded permutation, so that the members of a clade sit in different bands of the pair matrix.
    Two additions make every table reach what test_preconditions asks for.  The second and third clade take the first clade's founder: their
    six founder copies are equally far from each other, a tie at the fourth and fifth place (a clade of five alone has its four members 30
    mutations closer than anyone else: no tie at K = 4).  And after the shuffle the fourth clade is moved to the places 10, 30, 65, 66 and 68:
    the sample at 66 has nearest below 64 (met in the first band's column launch), at 65 (the second band's) and at 68 (its own row)."""
    rng = np.random.default_rng(seed)
    L = 6000
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    anc = rng.choice(acgt, size=L)

    def mutate(s, n):
        for p in rng.integers(600, L, size=n):                     # (the first 600 bases stay: constant rows at any k)
            s[p] = b"ACGT"[(b"ACGT".index(int(s[p])) + 1 + int(rng.integers(0, 3))) % 4]

    out, founder = [], None
    for i in range(S):
        if i % 5 == 0:
            founder = anc.copy()
            mutate(founder, 30)
            if i == 0:
                first = founder
            elif i in (5, 10):
                founder = first.copy()
        s = founder.copy()
        if i % 5 >= 2:
            mutate(s, i % 5 - 1)
        if i % 3 == 0:
            s = s[: int(L * 0.7) - 7 * i]
        w0 = int(rng.integers(600, 3000))
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


@pytest.fixture(scope="module", params=[(70, 9), (130, 9), (70, 41)], ids=lambda p: f"S{p[0]}-k{p[1]}")
def case(request, E):
    S, k = request.param
    samples = _samples(S, 1000 * S + k)
    names = [f"s{i}" for i in range(S)]
    arr = E.DictSet.build([E.record_stream(r) for r in samples], k, True).merge(names)
    ref = {}
    for mf in MIN_FREQS:
        for filt in (True, False):
            table, constant, rows = arr.distance_filtered(mf, filt)
            D, M = _matrices(table, S)
            P = len(table)
            sd, sm = np.sort(table["distance"]), np.sort(table["mismatch_prop"])
            ranks = (math.ceil(0.02 * P), math.ceil(0.3 * P))
            ref[(mf, filt)] = {"table": table.copy(), "constant": constant, "rows": rows, "D": D.tolist(), "M": M.tolist(), "Dn": D,
                               "snps": [float(sd[r - 1]) for r in ranks], "mism": [float(sm[r - 1]) for r in ranks],
                               "above": (float(sd[-1]) + 1.0, 1.0)}
    return {"S": S, "k": k, "names": names, "arr": arr, "ref": ref}


def _check(case, mf, filt, band_rows=0, **criteria):
    """one call against the model; -> (pairs, info)"""
    S, r = case["S"], case["ref"][(mf, filt)]
    pairs, constant, rows, info = case["arr"].distance_select(mf, filt, band_rows=band_rows, **criteria)
    assert (constant, rows) == (r["constant"], r["rows"])
    want = sorted(select(r["D"], r["M"], **criteria))
    got = list(zip(pairs["i"].tolist(), pairs["j"].tolist()))
    assert got == want, (mf, filt, band_rows, criteria, len(got), len(want), sorted(set(got) ^ set(want))[:5])
    idx = [_pair_index(S, i, j) for i, j in want]
    assert pairs["d"].tobytes() == r["table"][idx].tobytes(), (mf, filt, band_rows, criteria)
    return pairs, info


def _nearest(D, s, K):
    order = sorted((D[s][t], t) for t in range(len(D)) if t != s)
    return order[:K], order


def test_preconditions(case):
    """the inputs reach what the comparisons are meant to cover (asserted on the model side: the test fails if they do not)"""
    S = case["S"]
    for (mf, filt), r in case["ref"].items():
        assert r["rows"] >= 1100
        P, D, M = S * (S - 1) // 2, r["D"], r["M"]
        for crit in [{"max_snps": v} for v in r["snps"]] + [{"max_mismatches": v} for v in r["mism"]]:
            assert 0 < len(select(D, M, **crit)) < P, (mf, filt, crit)
        ties = {K: sum(1 for s in range(S) if (lambda o: o[K - 1][0] == o[K][0])(_nearest(D, s, K)[1])) for K in (1, 4, 7)}
        spans = {K: 0 for K in (4, 7, 64)}                                            # a list filled from two bands, from its row and its column
        for K in spans:
            for s in range(S):
                near = [t for _, t in _nearest(D, s, K)[0]]
                spans[K] += len({min(s, t) // BAND for t in near}) >= 2 and min(near) < s < max(near)
        print(f"S={S} k={case['k']} min_freq={mf} filt_ambig={filt}: ties at the K-th place {ties}, lists over two bands {spans}")
        # a tie at the K-th place, where the index rule decides: at K = 4 and 7 in every table, at K = 1 in the default mode's
        assert ties[4] and ties[7] and (ties[1] or not filt), (mf, filt, ties)
        assert all(spans.values()), (mf, filt, spans)
    assert case["ref"][(0.6, True)]["rows"] < case["ref"][(0.0, True)]["rows"]


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_thresholds(case, filt):
    for mf in MIN_FREQS:
        r = case["ref"][(mf, filt)]
        snps = [0.0] + r["snps"] + [r["above"][0]]
        mism = [0.0] + r["mism"] + [r["above"][1]]
        for v in snps:
            _check(case, mf, filt, max_snps=v)
        for v in mism:
            _check(case, mf, filt, max_mismatches=v)
        pairs, info = _check(case, mf, filt, max_snps=r["snps"][1], max_mismatches=r["mism"][1])
        assert info["candidates"] == len(pairs)
        _check(case, mf, filt, max_snps=r["snps"][0], max_mismatches=r["mism"][1], band_rows=BAND)


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_closest(case, filt):
    S = case["S"]
    for mf in MIN_FREQS:
        r = case["ref"][(mf, filt)]
        for K in KS(S):
            pairs, info = _check(case, mf, filt, band_rows=BAND, closest=K)
            assert info["candidates"] == S * (S - 1) // 2 and info["bands"] == math.ceil(S / BAND)
            _check(case, mf, filt, band_rows=BAND, closest=K, max_snps=r["snps"][1])
            _check(case, mf, filt, band_rows=BAND, closest=K, max_mismatches=r["mism"][1])
        _check(case, mf, filt, closest=4, max_snps=0.0)
        _check(case, mf, filt, closest=7, max_snps=r["snps"][1], max_mismatches=r["mism"][1])


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_band_rows(case, filt):
    S, r = case["S"], case["ref"][(0.6, filt)]
    for band in (0, 64, 50, 1, S, 1000):
        for crit in ({"max_snps": r["snps"][1]}, {"closest": 7}, {"closest": 4, "max_mismatches": r["mism"][1]}):
            _, info = _check(case, 0.6, filt, band_rows=band, **crit)
            if band:
                assert info["bands"] == math.ceil(S / band) and info["band_rows"] == min(band, S)
            else:
                assert info["bands"] == 1
            assert info["count_buffer_bytes"] == info["band_rows"] * S * 128 <= 1 << 30


def test_repeatable_and_the_array_stays(case):
    arr, r = case["arr"], case["ref"][(0.6, False)]
    before = arr.export()
    for filt in (True, False):
        for crit in ({"max_snps": r["snps"][1]}, {"closest": 7, "band_rows": BAND}):
            a = arr.distance_select(0.6, filt, **crit)
            b = arr.distance_select(0.6, filt, **crit)
            assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    assert all(np.array_equal(x, y) for x, y in zip(arr.export(), before))


def test_all_rows_through_the_twelve_class_sweep(case, monkeypatch):
    """SKX_KNOBS=stale_row_mask: every row goes through the 8-plane sweep -- same pairs"""
    r = case["ref"][(0.6, False)]
    crits = ({"max_snps": r["snps"][1], "max_mismatches": r["mism"][1]}, {"closest": 7, "band_rows": BAND})
    want = [case["arr"].distance_select(0.6, False, **c)[0].tobytes() for c in crits]
    set_knob(monkeypatch, "stale_row_mask", 1)
    assert [_check(case, 0.6, False, **c)[0].tobytes() for c in crits] == want


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_select_tsv_of_a_file(case, filt, tmp_path):
    """skh_distance_select_tsv: the header and the model's lines, in the table's order and text"""
    arr, S, names = case["arr"], case["S"], case["names"]
    path = str(tmp_path / "s.skf")
    arr.save(path)
    for mf in MIN_FREQS:
        r = case["ref"][(mf, filt)]
        for crit in ({"max_snps": r["snps"][1]}, {"max_mismatches": r["mism"][0]}, {"closest": 4, "max_mismatches": r["mism"][1]}):
            t = r["table"]
            lines = [FMT % (names[i], names[j], t["distance"][n], t["mismatch_prop"][n], t["match_count"][n], t["mismatch_count"][n])
                     for i, j in sorted(select(r["D"], r["M"], **crit)) for n in [_pair_index(S, i, j)]]
            assert arr.ctx.distance_select_tsv(path, mf, filt, **crit).decode() == "\n".join([HEADER] + lines) + "\n", (mf, crit)


def test_texts_long_enough_for_a_second_formatting_thread(case, tmp_path):
    """the host's writers hand rows (the whole table: a second thread from 32 samples) or slices of 4 096 lines (the selected lines, the sites:
    a second thread from 8 192) to threads.  With every pair selected the S = 130 table has 8 385 lines, and its sites file is cut where it
    passes 8 192 records: the three texts are the model's, whichever thread wrote a line"""
    import ora
    arr, S, names, r = case["arr"], case["S"], case["names"], case["ref"][(0.0, True)]
    path = str(tmp_path / "s.skf")
    arr.save(path)
    t = r["table"]
    lines = [FMT % (names[i], names[j], t["distance"][n], t["mismatch_prop"][n], t["match_count"][n], t["mismatch_count"][n])
             for n, (i, j) in enumerate(SM.all_pairs(S))]
    whole = "\n".join([HEADER] + lines) + "\n"
    assert (len(lines) >= 8192) == (S == 130) and S >= 32
    assert arr.ctx.distance_skf_tsv(path, 0.0, True).decode() == whole
    assert arr.ctx.distance_select_tsv(path, 0.0, True, max_snps=r["above"][0]).decode() == whole
    # the sites of the nearest pairs, up to the distance at which the records (a line's Distance is its number of sites) pass 8 192
    d = np.sort(t["distance"])
    cut = float(d[min(int(np.searchsorted(np.cumsum(d), 8192)), len(d) - 1)])
    pairs = [p for n, p in enumerate(SM.all_pairs(S)) if t["distance"][n] <= cut]
    table = arr.ctx.distance_sites(path, str(tmp_path / "p"), 0.0, max_snps=cut).decode()
    assert table == "\n".join([HEADER] + [lines[_pair_index(S, i, j)] for i, j in pairs]) + "\n"
    oa = ora.Array.load(path)
    keys, var, counts = oa.export()
    assert oa.names == names
    recs = SM.sites(var, SM.sweep_flags(var, 0.0, counts), pairs)
    print(f"S={S} k={case['k']}: {len(lines)} lines; --max-snps {cut:g}: {len(pairs)} lines, {len(recs)} records")
    assert len(recs) >= 8192
    assert open(str(tmp_path / "p.sites.tsv")).read() == SM.sites_text(names, keys, case["k"], pairs, recs)


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_prefiltered_array(E, case, filt):
    """skx_array_distance_select_prefiltered (what skh_distance_select_tsv calls after the one-pass filtered load): every row swept, the constant
    as given -- against the model on skx_array_distance's table of the same array and constant"""
    arr, S = case["arr"], case["S"]
    for constant in (0, 17):
        table = arr.distance(float(constant), filt)
        D, M = _matrices(table, S)
        sd, sm = np.sort(table["distance"]), np.sort(table["mismatch_prop"])
        snps, mism = float(sd[math.ceil(0.3 * len(sd)) - 1]), float(sm[math.ceil(0.3 * len(sm)) - 1])
        for crit in ({"max_snps": snps}, {"max_mismatches": mism}, {"closest": 4, "band_rows": BAND}, {"closest": 7, "max_snps": snps, "max_mismatches": mism, "band_rows": 50}):
            model = {k: v for k, v in crit.items() if k != "band_rows"}
            want = sorted(select(D.tolist(), M.tolist(), **model))
            pairs, info = arr.distance_select_prefiltered(constant, filt, **crit)
            assert 0 < len(want) < len(table) and list(zip(pairs["i"].tolist(), pairs["j"].tolist())) == want, (constant, crit)
            assert pairs["d"].tobytes() == table[[_pair_index(S, i, j) for i, j in want]].tobytes(), (constant, crit)
            assert info["bands"] == math.ceil(S / crit.get("band_rows", S))
    with pytest.raises(E.EngineError) as e:
        arr.distance_select_prefiltered(-1, filt, max_snps=1.0)
    assert e.value.code == E.EINVAL and "distance select:" in str(e.value)


def test_refusals(E, case):
    arr, S = case["arr"], case["S"]
    nan = float("nan")
    bad = [{"max_snps": nan}, {"max_mismatches": nan}, {"max_mismatches": 1.5}, {"closest": -1}, {"max_snps": 1.0, "band_rows": -1}, {}]
    for crit in bad:
        with pytest.raises(E.EngineError) as e:
            arr.distance_select(0.0, True, **crit)
        assert e.value.code == E.EINVAL and "distance select:" in str(e.value), (crit, str(e.value))


def test_closest_range_and_small_arrays(E):
    """1 024 < K < S - 1 is refused, K >= S - 1 is no constraint; fewer than two samples give no pair"""
    rng = np.random.default_rng(7)
    base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=300)
    recs = []
    for i in range(1030):
        s = base.copy()
        s[20 + (i % 250)] = b"ACGT"[(b"ACGT".index(int(s[20 + (i % 250)])) + 1 + i // 250 % 3) % 4]
        recs.append(s.tobytes())
    arr = E.DictSet.build([E.record_stream([r]) for r in recs], 9, True).merge([f"t{i}" for i in range(1030)])
    with pytest.raises(E.EngineError) as e:
        arr.distance_select(0.0, True, closest=1025)
    assert e.value.code == E.EINVAL and "distance select:" in str(e.value)
    table, _, _ = arr.distance_filtered(0.0, True)
    pairs, _, _, info = arr.distance_select(0.0, True, closest=1029)
    assert len(pairs) == len(table) and pairs["d"].tobytes() == table.tobytes() and info["bands"] == 1
    D, M = _matrices(table, 1030)
    # the longest list the engine holds, nearly every pair a candidate: most of a list is one long tie that the index rule orders
    pairs, _, _, _ = arr.distance_select(0.0, True, closest=1024, max_snps=2.0)
    got = set(zip(pairs["i"].tolist(), pairs["j"].tolist()))
    cand = (D <= 2.0) & ~np.eye(1030, dtype=bool)
    near = np.argsort(np.where(cand, D * 4096 + np.arange(1030)[None, :], 1e12), axis=1, kind="stable")[:, :1024]
    want = {(min(s, int(t)), max(s, int(t))) for s in range(1030) for t in near[s] if cand[s][t]}
    assert got == want and 0 < len(got) < len(table)
    assert int(cand.sum(axis=1).max()) > 1024                                          # some list is full
    one = E.DictSet.build([E.record_stream([recs[0]])], 9, True).merge(["only"])
    pairs, _, _, _ = one.distance_select(0.0, True, max_snps=1.0)
    assert len(pairs) == 0


def _select_columns(i, j, d, m, max_snps=None, max_mismatches=None, closest=0):
    """select_model.select on the table's columns with numpy, for tables too long for the plain model -> mask of the pairs kept"""
    cand = np.ones(len(d), bool)
    if max_snps is not None:
        cand &= d <= max_snps
    if max_mismatches is not None:
        cand &= m <= max_mismatches
    if not closest:
        return cand
    idx = np.flatnonzero(cand)
    own, other = np.concatenate((i[idx], j[idx])), np.concatenate((j[idx], i[idx]))
    order = np.lexsort((other, np.concatenate((d[idx], d[idx])), own))                  # every sample's candidates by (distance, partner)
    owner = own[order]
    keep = np.zeros(len(d), bool)
    keep[np.concatenate((idx, idx))[order[np.arange(len(order)) - np.searchsorted(owner, owner, side="left") < closest]]] = True
    return keep


def test_the_engines_own_band_choice_with_two_bands(E):
    """band_rows = 0 where one band's counters would pass 1 GiB: S = 2 900 gives 2 880 first samples a band (the largest multiple of 64 within
    1 GiB) and a second band of 20; thresholds and --closest against the full table through the numpy form of the model, which is first
    held against the model itself on a small table full of ties"""
    rng = np.random.default_rng(3)
    S0 = 40
    i0, j0 = np.triu_indices(S0, 1)
    d0, m0 = rng.integers(0, 4, len(i0)).astype(float), rng.integers(0, 5, len(i0)) / 4
    D0, M0 = np.zeros((S0, S0)), np.zeros((S0, S0))
    D0[i0, j0], M0[i0, j0] = d0, m0
    for crit in ({"closest": 1}, {"closest": 4}, {"closest": 7, "max_snps": 2.0}, {"closest": 3, "max_mismatches": 0.5, "max_snps": 1.0}, {"max_mismatches": 0.5}):
        k = _select_columns(i0, j0, d0, m0, **crit)
        assert set(zip(i0[k].tolist(), j0[k].tolist())) == select((D0 + D0.T).tolist(), (M0 + M0.T).tolist(), **crit), crit
    S = 2900
    rng = np.random.default_rng(11)
    base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=300)
    recs = []
    for n in range(S):
        s = base.copy()
        for p in rng.integers(20, 280, size=int(rng.integers(0, 3))):                  # 0-2 mutations: many equal distances
            s[p] = b"ACGT"[(b"ACGT".index(int(s[p])) + 1 + int(rng.integers(0, 3))) % 4]
        recs.append(s.tobytes())
    arr = E.DictSet.build([E.record_stream([x]) for x in recs], 9, True).merge([f"t{n}" for n in range(S)])
    table, constant, rows = arr.distance_filtered(0.0, True)
    i, j = np.triu_indices(S, 1)
    d, m = table["distance"], table["mismatch_prop"]
    for crit in ({"max_snps": 1.0}, {"closest": 3}, {"closest": 5, "max_mismatches": float(np.sort(m)[len(m) // 3])}):
        pairs, c, n_rows, info = arr.distance_select(0.0, True, **crit)
        assert (c, n_rows) == (constant, rows)
        assert (info["bands"], info["band_rows"]) == (2, 2880) and info["count_buffer_bytes"] == 2880 * S * 128 <= 1 << 30
        k = np.flatnonzero(_select_columns(i, j, d, m, **crit))
        assert 0 < len(k) < len(table)
        assert np.array_equal(pairs["i"], i[k]) and np.array_equal(pairs["j"], j[k]) and pairs["d"].tobytes() == table[k].tobytes(), crit
    arr.free()
