"""The model of `ska distance --mst` (tests/mst_model.py) against independent restatements, on seeded integer tables whose distances lie in
0..3 so that most lines tie and the (Distance, i, j) rule decides.  No device."""
import numpy as np
import pytest

from mst_model import boruvka, candidates, components, kruskal, levels, mst, mst_streamed, mst_text
from select_model import select

SIZES = (2, 3, 17, 40)
CRITERIA = ({}, {"max_snps": 1.0}, {"max_mismatches": 0.5}, {"max_snps": 0.0, "max_mismatches": 0.0})


def _table(S, seed=0):
    rng = np.random.default_rng(100 * S + seed)
    D, M = np.zeros((S, S)), np.zeros((S, S))
    iu = np.triu_indices(S, 1)
    D[iu], M[iu] = rng.integers(0, 4, len(iu[0])), rng.integers(0, 5, len(iu[0])) / 4
    return (D + D.T).tolist(), (M + M.T).tolist()


def _prim(D, cand):
    """Prim from the lowest unreached sample of every component, the frontier ordered by (distance, lower index, higher index)"""
    S = len(D)
    adj = [[] for _ in range(S)]
    for i, j in cand:
        adj[i].append(j)
        adj[j].append(i)
    reached, kept = set(), set()
    for start in range(S):
        if start in reached:
            continue
        reached.add(start)
        while True:
            frontier = [(D[s][t], min(s, t), max(s, t)) for s in reached for t in adj[s] if t not in reached]
            if not frontier:
                break
            _, i, j = min(frontier)
            kept.add((i, j))
            reached.update((i, j))
    return kept


@pytest.mark.parametrize("S", SIZES)
def test_mst_is_prims_forest_and_the_streamed_form_agrees(S):
    D, M = _table(S)
    for crit in CRITERIA:
        cand = select(D, M, **crit)
        want = _prim(D, cand)
        assert mst(D, M, **crit) == want, crit
        assert len(want) == S - len(set(components(S, cand)))
        for band in (1, 3, 16, S):
            got, rounds = mst_streamed(D, M, band, **crit)
            assert got == want, (crit, band)
            assert (rounds >= 1) == bool(want)
    if S >= 17:
        assert 0 < len(mst(D, M, **CRITERIA[3])) < S - 1                                  # the thresholds leave a forest, not a tree


@pytest.mark.parametrize("S", (17, 40))
def test_the_tie_rule_decides(S):
    """the same Kruskal with the ties taken from the table's end gives another forest: equal distances alone do not fix the lines"""
    D, M = _table(S)
    for crit in CRITERIA[:2]:
        cand = candidates(D, M, **crit)
        reverse = kruskal(S, sorted(cand, key=lambda e: (e[0], -e[1], -e[2])))
        assert reverse != mst(D, M, **crit) and len(reverse) == len(mst(D, M, **crit))


def test_boruvka_rounds():
    """a path whose distances fall towards one end joins in one round; equal distances on a path pair up and halve the trees every round"""
    S = 8
    fall = [(float(S - i), i, i + 1) for i in range(S - 1)]
    assert boruvka(S, fall) == (set(fall), 1)
    flat = [(1.0, i, i + 1) for i in range(S - 1)]
    kept, rounds = boruvka(S, flat)
    assert kept == set(flat) and rounds == 1                                                # (every sample's smallest line is the one to its left)
    assert boruvka(S, []) == (set(), 0)


@pytest.mark.parametrize("filt_ambig", (True, False))
def test_the_printed_distance_is_strictly_increasing_in_the_key(filt_ambig):
    """key -> distance is the engine's key_distance: the key itself by default, key / 36 with --allow-ambiguous"""
    last = -1.0
    for key in range(100001):
        d = float(key) if filt_ambig else float(key) / 36.0
        printed = float("%.2f" % d)
        assert printed > last, key
        last = printed


@pytest.mark.parametrize("S", SIZES)
def test_levels_are_the_single_linkage_clusters_of_the_candidates(S):
    D, M = _table(S, seed=1)
    names = [f"s{i}" for i in range(S)]
    for crit in CRITERIA[:3]:
        edges = mst(D, M, **crit)
        ladder = [3, 2.5, 2, 1, 0]
        columns, csv = levels(D, M, edges, ladder, names)
        for L, col in zip(ladder, columns):
            label = components(S, [(i, j) for i, j in select(D, M, **crit) if float("%.2f" % D[i][j]) <= L])
            # the same partition, numbered 1, 2, ... by the lowest sample
            roots = sorted(set(label))
            assert col == [roots.index(r) + 1 for r in label], (crit, L)
            assert col[0] == 1 and all(c <= max(col[:n]) + 1 for n, c in enumerate(col) if n)
        assert csv.splitlines()[0] == "id,snps_3,snps_2.5,snps_2,snps_1,snps_0,address" and len(csv.splitlines()) == S + 1


def test_the_worked_example():
    names = ["a", "b", "c", "d,x", 'e"']
    lines = {(0, 1): 0, (0, 2): 3, (0, 3): 9, (0, 4): 100, (1, 2): 3, (1, 3): 9, (1, 4): 100, (2, 3): 7, (2, 4): 100, (3, 4): 50}
    D = [[0.0] * 5 for _ in range(5)]
    for (i, j), d in lines.items():
        D[i][j] = D[j][i] = float(d)
    M = [[0.0] * 5 for _ in range(5)]
    edges = mst(D, M)
    assert edges == {(0, 1), (0, 2), (2, 3), (3, 4)}                                       # (0, 2) before (1, 2): the line's place in the table
    assert mst(D, M, max_snps=8.0) == {(0, 1), (0, 2), (2, 3)}
    columns, csv = levels(D, M, edges, [50, 5.5, 0], names)
    assert columns == [[1, 1, 1, 1, 1], [1, 1, 1, 2, 3], [1, 1, 2, 3, 4]]
    assert csv == ('id,snps_50,snps_5.5,snps_0,address\n'
                   'a,1,1,1,1.1.1\n'
                   'b,1,1,1,1.1.1\n'
                   'c,1,1,2,1.1.2\n'
                   '"d,x",1,2,3,1.2.3\n'
                   '"e""",1,3,4,1.3.4\n')
    header = "Sample1\tSample2\tDistance\tMismatches (proportion)\tMatch count\tMismatch count\n"
    text = header + "".join(f"{names[i]}\t{names[j]}\t{d:.2f}\t0.00000\t10\t0\n" for (i, j), d in sorted(lines.items()))
    kept = mst_text(text).splitlines()
    assert kept[0] + "\n" == header and [ln.split("\t")[:2] for ln in kept[1:]] == [["a", "b"], ["a", "c"], ["c", "d,x"], ["d,x", 'e"']]
