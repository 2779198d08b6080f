"""skx_array_distance_banded / skh_distance_banded_files / `ska distance --no-table` (`-m gpu`), through skx_engine.py.  The clusters are held
against skh_distance_clusters applied to the full table (Array.distance_filtered on the same array) and against the model of
tests/banded_model.py on the table's float64 values; the joins against skx_dist_nj on the full table, byte for byte.  The shapes sit on the pair
sweep's tile edges (S = 70 and 130), the band of 64 first samples cuts both into several bands, and the thresholds are printed values of the
table itself and those values +- 0.005 (+- 0.000005 for the proportion), so the printed-value rule is exercised on its boundary."""
import math
import os
import subprocess

import numpy as np
import pytest
from conftest import set_knob

from banded_model import clusters, printed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
MIN_FREQS = (0.0, 0.6)
BAND = 64
# the planted chain, in the order of its links: each link (a, b) lies in the band of min(a, b), a different one for every link; its lowest
# sample is the last one reached
CHAIN = {70: (69, 65, 3), 130: (129, 128, 70, 5)}


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def _point(s, p, step=1):
    s[p] = b"ACGT"[(b"ACGT".index(int(s[p])) + step) % 4]


def _samples(S, seed):
    """one ancestor; clades of five consecutive samples: a founder (30 point mutations), members 0 and 1 equal to it (duplicates: distance 0),
    members 2-4 with 1-3 mutations of their own; every third sample truncated (missing rows, the tail below a min_freq of 0.6); each sample's
    second record a window of itself with a base changed every 90 (the ambiguous cells); then the order shuffled with a seeded permutation,
    so that the members of a clade sit in different bands of the pair matrix.  Last, the places of CHAIN[S] take a chain of their own clade:
    every member four mutations (120 bases apart) further from the founder than the one before it."""
    rng = np.random.default_rng(seed)
    L = 6000
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    anc = rng.choice(acgt, size=L)

    def mutate(s, n):
        for p in rng.integers(600, L, size=n):                     # (the first 600 bases stay: constant rows at any k)
            _point(s, p, 1 + int(rng.integers(0, 3)))

    def with_window(s):
        w0 = int(rng.integers(600, 3000))
        win = s[w0:w0 + 400].copy()
        for p in range(60, len(win), 90):
            _point(win, p, 1 + int(rng.integers(0, 3)))
        return [s.tobytes(), win.tobytes()]

    out, founder = [], None
    for i in range(S):
        if i % 5 == 0:
            founder = anc.copy()
            mutate(founder, 30)
        s = founder.copy()
        if i % 5 >= 2:
            mutate(s, i % 5 - 1)
        if i % 3 == 0:
            s = s[: int(L * 0.7) - 7 * i]
        out.append(with_window(s))
    order = [int(p) for p in np.random.default_rng(S).permutation(S)]
    out = [out[p] for p in order]
    link = anc.copy()
    mutate(link, 30)
    for n, place in enumerate(CHAIN[S]):
        for m in range(4 * n, 4 * n + 4):
            _point(link, 700 + 120 * m)
        out[place] = with_window(link.copy())
    return out


def _matrices(table, S):
    D, M = np.zeros((S, S)), np.zeros((S, S))
    iu = np.triu_indices(S, 1)                                      # row-major (i < j): the table's order
    D[iu], M[iu] = table["distance"], table["mismatch_prop"]
    return (D + D.T).tolist(), (M + M.T).tolist()


def _thresholds(table):
    """(cluster_snps values, cluster_mismatches values): 0, a value no pair exceeds, and printed values of the table with their neighbours"""
    P = len(table)
    sd, sm = np.sort(table["distance"]), np.sort(table["mismatch_prop"])
    snps, mism = [0.0, float(sd[-1]) + 1.0], [0.0, 1.0]
    for r in (math.ceil(0.004 * P), math.ceil(0.02 * P)):
        v = printed(float(sd[r - 1]), 2)
        snps += [v, v + 0.005, max(v - 0.005, 0.0)]
    v = printed(float(sm[math.ceil(0.3 * P) - 1]), 5)
    mism += [v, v + 0.000005, max(v - 0.000005, 0.0)]
    return snps, mism


@pytest.fixture(scope="module", params=[(70, 9), (130, 9), (70, 41)], ids=lambda p: f"S{p[0]}-k{p[1]}")
def case(request, E):
    S, k = request.param
    names = [f"s{i}" for i in range(S)]
    arr = E.DictSet.build([E.record_stream(r) for r in _samples(S, 1000 * S + k)], k, True).merge(names)
    ref = {}
    for mf in MIN_FREQS:
        for filt in (True, False):
            table, constant, rows = arr.distance_filtered(mf, filt)
            D, M = _matrices(table, S)
            snps, mism = _thresholds(table)
            ref[(mf, filt)] = {"table": table.copy(), "constant": constant, "rows": rows, "D": D, "M": M, "snps": snps, "mism": mism, "model": {}}
    return {"S": S, "k": k, "names": names, "arr": arr, "ref": ref}


def _model(r, cs, cm):
    if (cs, cm) not in r["model"]:
        r["model"][(cs, cm)] = clusters(r["D"], r["M"], cs, cm)
    return r["model"][(cs, cm)]


def _check_labels(E, case, mf, filt, cs, cm, band_rows=0):
    """one call against skh_distance_clusters on the full table and against the model; -> (labels, info)"""
    r, names = case["ref"][(mf, filt)], case["names"]
    labels, joins, constant, rows, info = case["arr"].distance_banded(mf, filt, cluster_snps=cs, cluster_mismatches=cm, band_rows=band_rows)
    assert joins is None and (constant, rows) == (r["constant"], r["rows"])
    want, edges, n_clusters = _model(r, cs, cm)
    assert labels.tolist() == want, (mf, filt, cs, cm, band_rows)
    assert E.clusters_csv(names, labels) == E.distance_clusters(names, r["table"], cs, cm)[0], (mf, filt, cs, cm, band_rows)
    assert (info["edges"], info["clusters"]) == (edges, n_clusters), (mf, filt, cs, cm, band_rows)
    return labels, info


def _chain_threshold(case):
    """the largest printed distance among the chain's links, in the default table"""
    D, chain = case["ref"][(0.0, True)]["D"], CHAIN[case["S"]]
    return max(printed(D[a][b], 2) for a, b in zip(chain, chain[1:]))


def test_preconditions(case):
    """the inputs reach what the comparisons are meant to cover (asserted on the model side: the test fails if they do not)"""
    S, chain = case["S"], CHAIN[case["S"]]
    for (mf, filt), r in case["ref"].items():
        assert r["rows"] >= 1100
        # at least two clusters of more than one sample at one of the thresholds tested (the duplicates are 0 apart only without ambiguous cells)
        multi = {cs: int((np.bincount(_model(r, cs, 1.0)[0], minlength=S) > 1).sum()) for cs in r["snps"]}
        print(f"S={S} k={case['k']} min_freq={mf} filt_ambig={filt}: clusters of more than one sample per cluster_snps {multi}")
        assert max(multi.values()) >= 2, (mf, filt, multi)
        counts = {_model(r, cs, 1.0)[2] for cs in r["snps"]} | {_model(r, r["snps"][1], cm)[2] for cm in r["mism"]}
        assert 1 in counts and len(counts) >= 4, (mf, filt, counts)                 # the thresholds bite differently, the largest joins all
        # thresholds that equal a printed value of the table, and such a pair changes sides half a hundredth below
        printed_d = {printed(v, 2) for v in r["table"]["distance"].tolist()}
        on = [cs for cs in r["snps"][2:] if cs in printed_d]
        assert on, (mf, filt)
        assert any(_model(r, cs, 1.0)[1] > _model(r, max(cs - 0.005, 0.0), 1.0)[1] for cs in on), (mf, filt)
        printed_m = {printed(v, 5) for v in r["table"]["mismatch_prop"].tolist()}
        assert r["mism"][2] in printed_m
    assert case["ref"][(0.6, True)]["rows"] < case["ref"][(0.0, True)]["rows"]
    # the chain: its links span bands, one band each; only consecutive members are within the threshold, nobody else is
    links = list(zip(chain, chain[1:]))
    assert len({min(a, b) // BAND for a, b in links}) == len(links) >= 2 and min(chain) == chain[-1]
    D, T = case["ref"][(0.0, True)]["D"], _chain_threshold(case)
    for x in chain:
        near = {y for y in range(S) if y != x and printed(D[x][y], 2) <= T}
        assert near == {c for c in chain if abs(chain.index(c) - chain.index(x)) == 1}, (x, near)


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_labels_at_the_tables_own_thresholds(E, case, filt):
    for mf in MIN_FREQS:
        r = case["ref"][(mf, filt)]
        for cs in r["snps"]:
            for band in (BAND, 0):
                _check_labels(E, case, mf, filt, cs, 1.0, band)
        for cm in r["mism"]:
            for band in (BAND, 0):
                _check_labels(E, case, mf, filt, r["snps"][1], cm, band)
        _check_labels(E, case, mf, filt, r["snps"][5], r["mism"][2], BAND)


def test_band_rows(E, case):
    S, r = case["S"], case["ref"][(0.6, False)]
    for band in (0, 64, 50, 1, S, 1000):
        _, info = _check_labels(E, case, 0.6, False, r["snps"][5], r["mism"][3], band)
        if band:
            assert info["bands"] == math.ceil(S / band) and info["band_rows"] == min(band, S)
        else:
            assert info["bands"] == 1
        assert info["count_buffer_bytes"] == info["band_rows"] * S * 128 <= 1 << 30


def test_the_plain_union_gives_the_same_labels(E, case, monkeypatch):
    """SKX_KNOBS=union_per_edge: one link per passing pair instead of one per distinct root of a wave's part of the row"""
    set_knob(monkeypatch, "union_per_edge", 1)
    r = case["ref"][(0.6, False)]
    for cs in r["snps"]:
        for band in (BAND, 0):
            _check_labels(E, case, 0.6, False, cs, r["mism"][3], band)
    chain, T = CHAIN[case["S"]], _chain_threshold(case)
    labels, _ = _check_labels(E, case, 0.0, True, T, 1.0, 1)
    assert [int(labels[c]) for c in chain] == [min(chain)] * len(chain)


def test_planted_chain_is_one_cluster_rooted_at_its_lowest_sample(E, case):
    chain, T = CHAIN[case["S"]], _chain_threshold(case)
    for band in (BAND, 1, 0):
        labels, _ = _check_labels(E, case, 0.0, True, T, 1.0, band)
        assert [int(labels[c]) for c in chain] == [min(chain)] * len(chain)
        assert int((labels == min(chain)).sum()) == len(chain)


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_tree(E, case, filt):
    arr, S, names = case["arr"], case["S"], case["names"]
    for mf in MIN_FREQS:
        r = case["ref"][(mf, filt)]
        want = arr.ctx.dist_nj(r["table"], S)
        text = E.nj_newick(names, want)
        for band in (BAND, 0, 50):
            labels, joins, constant, rows, info = arr.distance_banded(mf, filt, labels=False, tree=True, band_rows=band)
            assert labels is None and (constant, rows) == (r["constant"], r["rows"]) and info["edges"] == info["clusters"] == 0
            assert joins.tobytes() == want.tobytes(), (mf, filt, band)
            assert E.nj_newick(names, joins) == text


def test_both_outputs_in_one_call_equal_each_alone(E, case):
    arr = case["arr"]
    for mf, filt in ((0.0, True), (0.6, False)):
        r = case["ref"][(mf, filt)]
        cs, cm = r["snps"][5], r["mism"][2]
        for band in (BAND, 0):
            only_l = arr.distance_banded(mf, filt, cluster_snps=cs, cluster_mismatches=cm, band_rows=band)
            only_t = arr.distance_banded(mf, filt, labels=False, tree=True, band_rows=band)
            both = arr.distance_banded(mf, filt, labels=True, tree=True, cluster_snps=cs, cluster_mismatches=cm, band_rows=band)
            assert both[0].tobytes() == only_l[0].tobytes() and both[1].tobytes() == only_t[1].tobytes()
            assert both[2:] == only_l[2:]
            assert 1 < both[4]["clusters"] < case["S"]


@pytest.mark.parametrize("filt", [True, False], ids=["filter-ambiguous", "allow-ambiguous"])
def test_prefiltered_array(E, case, filt):
    """skx_array_distance_banded_prefiltered (what skh_distance_banded_files calls after the one-pass filtered load): every row swept, the
    constant as given -- against skh_distance_clusters and skx_dist_nj on skx_array_distance's table of the same array and constant"""
    arr, S, names = case["arr"], case["S"], case["names"]
    for constant in (0, 17):
        table = arr.distance(float(constant), filt)
        D, M = _matrices(table, S)
        snps, mism = _thresholds(table)
        want_joins = arr.ctx.dist_nj(table, S)
        for cs, cm, band in ((snps[5], 1.0, BAND), (snps[2], mism[2], 50), (snps[1], mism[4], 0)):
            labels, joins, info = arr.distance_banded_prefiltered(constant, filt, labels=True, tree=True, cluster_snps=cs, cluster_mismatches=cm, band_rows=band)
            want, edges, n_clusters = clusters(D, M, cs, cm)
            assert labels.tolist() == want and (info["edges"], info["clusters"]) == (edges, n_clusters), (constant, cs, cm)
            assert E.clusters_csv(names, labels) == E.distance_clusters(names, table, cs, cm)[0]
            assert joins.tobytes() == want_joins.tobytes()
            assert info["bands"] == math.ceil(S / (band or S))
    with pytest.raises(E.EngineError) as e:
        arr.distance_banded_prefiltered(-1, filt)
    assert e.value.code == E.EINVAL and "distance banded:" in str(e.value)


def test_refusals(E, case):
    arr = case["arr"]
    nan = float("nan")
    bad = [{"labels": False, "tree": False}, {"cluster_snps": nan}, {"cluster_mismatches": nan}, {"cluster_snps": -1.0}, {"cluster_mismatches": -0.1},
           {"band_rows": -1}, {"labels": False, "tree": True, "band_rows": -1}]
    for kw in bad:
        with pytest.raises(E.EngineError) as e:
            arr.distance_banded(0.0, True, **kw)
        assert e.value.code == E.EINVAL and str(e.value).split("] ", 1)[1].startswith("distance banded:"), (kw, str(e.value))
    # the thresholds are the clusters': a tree alone does not read them
    assert arr.distance_banded(0.0, True, labels=False, tree=True, cluster_snps=nan)[1] is not None


def test_repeatable_and_the_array_stays(case):
    arr, r = case["arr"], case["ref"][(0.6, False)]
    before = arr.export()
    a = arr.distance_banded(0.6, False, tree=True, cluster_snps=r["snps"][5], band_rows=BAND)
    b = arr.distance_banded(0.6, False, tree=True, cluster_snps=r["snps"][5], band_rows=BAND)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:]
    assert all(np.array_equal(x, y) for x, y in zip(arr.export(), before))


def test_fully_connected(E, monkeypatch):
    """all samples identical at S = 130: every pair is an edge, the union's worst case -- one cluster, S (S - 1) / 2 edges"""
    S = 130
    rng = np.random.default_rng(5)
    rec = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=1500).tobytes()
    arr = E.DictSet.build([E.record_stream([rec])] * S, 9, True).merge([f"t{i}" for i in range(S)])
    for plain in (0, 1):
        set_knob(monkeypatch, "union_per_edge", plain)
        for band in (BAND, 1, 0):
            labels, _, _, _, info = arr.distance_banded(0.0, True, cluster_snps=0.0, cluster_mismatches=0.0, band_rows=band)
            assert labels.tolist() == [0] * S and (info["edges"], info["clusters"]) == (S * (S - 1) // 2, 1)
    arr.free()


def test_one_and_two_samples(E):
    rng = np.random.default_rng(9)
    base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=400)
    other = base.copy()
    for p in (100, 200, 300):
        _point(other, p)
    one = E.DictSet.build([E.record_stream([base.tobytes()])], 9, True).merge(["only"])
    labels, joins, _, _, info = one.distance_banded(0.0, True)
    assert labels.tolist() == [0] and joins is None and (info["edges"], info["clusters"]) == (0, 1)
    with pytest.raises(E.EngineError) as e:
        one.distance_banded(0.0, True, labels=False, tree=True)
    assert e.value.code == E.EINVAL
    two = E.DictSet.build([E.record_stream([base.tobytes()]), E.record_stream([other.tobytes()])], 9, True).merge(["a", "b"])
    table, _, _ = two.distance_filtered(0.0, True)
    d = printed(float(table["distance"][0]), 2)
    assert d > 0
    for cs, want, edges in ((d, [0, 0], 1), (d - 0.005, [0, 1], 0)):
        labels, joins, _, _, info = two.distance_banded(0.0, True, tree=True, cluster_snps=cs)
        assert labels.tolist() == want and (info["edges"], info["clusters"]) == (edges, 2 - edges)
        assert joins.tobytes() == two.ctx.dist_nj(table, 2).tobytes()


@pytest.mark.parametrize("allow", [False, True], ids=["filter-ambiguous", "allow-ambiguous"])
def test_executable_writes_the_table_paths_files_and_nothing_else(case, tmp_path, allow):
    """`ska distance x.skf --no-table --tree t.nwk --clusters c --cluster-snps N`: the files of the same command without --no-table, no
    c.graph.dot, nothing on stdout"""
    r = case["ref"][(0.0, not allow)]
    src = str(tmp_path / "x.skf")
    case["arr"].save(src)
    args = ["distance", src, "--tree", "t.nwk", "--clusters", "c", "--cluster-snps", repr(r["snps"][5]), "--cluster-mismatches", repr(r["mism"][2])]
    args += ["--allow-ambiguous"] if allow else []
    out = {}
    for name, extra in (("table", []), ("banded", ["--no-table"])):
        wd = tmp_path / name
        wd.mkdir()
        p = subprocess.run([SKA, *args, *extra], cwd=str(wd), capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr[-1500:].decode(errors="replace")
        out[name] = (p.stdout, {f: (wd / f).read_bytes() for f in sorted(os.listdir(wd))})
    assert out["banded"][0] == b"" and out["table"][0].count(b"\n") == 1 + case["S"] * (case["S"] - 1) // 2
    assert sorted(out["table"][1]) == ["c.clusters.csv", "c.graph.dot", "t.nwk"] and sorted(out["banded"][1]) == ["c.clusters.csv", "t.nwk"]
    for f in ("c.clusters.csv", "t.nwk"):
        assert out["banded"][1][f] == out["table"][1][f], f
    assert 2 < len(set(ln.rsplit(b",", 1)[1] for ln in out["banded"][1]["c.clusters.csv"].splitlines()[1:])) < case["S"]
