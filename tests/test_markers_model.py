"""tests/markers_model.py (the model the GPU tests of `ska markers` compare against) held against a worked example written out by hand, a
second, set-based restatement in plain Python, and the oracle: its delete_samples (a group's private rows are the rows the delete drops) and
its weed (the model's FASTA, weeded in reverse, keeps exactly the marker rows).  CPU only."""
import functools

import numpy as np
import pytest

import markers_model as MM
import subset_model as M

PART = [[4, 5, 6, 7], [9, 11, 8, 10], [0, 3, 1, 2], [12]]                 # the large cases' partition
PART_TINY = [[0, 3], [1, 2, 4], [5]]
P_, A_ = MM.PRESENCE, MM.ALLELE


def _tuples(recs):
    return [(int(r["group"]), int(r["row"]), int(r["n_in"]), int(r["n_out"]), int(r["kind"]), int(r["bases_in"]), int(r["bases_out"])) for r in recs]


# ---- 1. a worked example: 6 samples; groups A = {0, 1}, B = {2, 3}, C = {4}; sample 5 is listed by no group ----
EXAMPLE = [
    "AA----",     # 0  only A has it                              presence of A
    "AACCCC",     # 1  A holds A, everybody else C                allele of A (B and C share C with the others)
    "AACCGG",     # 2  A: A / others C, G;  B: C / others A, G    allele of A and of B; C shares G with the unlisted sample
    "RRCCCC",     # 3  A holds R = {A, G}, the others C           allele of A with an ambiguous set
    "RRGGGG",     # 4  R stands for A and G: G is outside too     nobody's
    "AAAAAA",     # 5  the same set on both sides                 nobody's
    "--TT--",     # 6  only B                                     presence of B
    "----A-",     # 7  only C                                     presence of C
    "-----A",     # 8  only the unlisted sample                   nobody's: the unnamed segment is never reported
    "A-CCCC",     # 9  half of A                                  nobody's at P = 1; allele of A at P = 0.5
    "TT---T",     # 10 A and one other sample, same base          nobody's at Q = 0; presence of A at Q = 0.25 (t_out = floor(4 * 0.25) = 1)
]
EX_VAR = np.array([[ord(c) for c in row] for row in EXAMPLE], np.uint8)
EX_SEG = MM.partition(6, [[0, 1], [2, 3], [4]])
EX_WANT = [
    (0, 0, 2, 0, P_, 1, 0), (0, 1, 2, 4, A_, 1, 2), (0, 2, 2, 4, A_, 1, 2 | 8), (0, 3, 2, 4, A_, 1 | 8, 2),
    (1, 2, 2, 4, A_, 2, 1 | 8), (1, 6, 2, 0, P_, 4, 0),
    (2, 7, 1, 0, P_, 1, 0),
]


def test_worked_example():
    recs, counts = MM.markers(EX_VAR, EX_SEG, 3)
    assert _tuples(recs) == EX_WANT
    assert counts == [(1, 3), (1, 1), (1, 0)]
    assert list(EX_SEG) == [0, 0, 1, 1, 2, 3]
    assert MM.thresholds(2, 6, 1.0, 0.0) == (2, 0) and MM.thresholds(2, 6, 0.5, 0.25) == (1, 1) and MM.thresholds(1, 6, 0.0, 0.0) == (1, 0)
    # the two kinds one at a time: an allele marker stays "not a presence marker" whichever are asked for
    assert _tuples(MM.markers(EX_VAR, EX_SEG, 3, kinds=P_)[0]) == [t for t in EX_WANT if t[4] == P_]
    assert _tuples(MM.markers(EX_VAR, EX_SEG, 3, kinds=A_)[0]) == [t for t in EX_WANT if t[4] == A_]
    # a group that is not reported still counts as others
    recs, counts = MM.markers(EX_VAR, EX_SEG, 3, reported=[True, False, True])
    assert _tuples(recs) == [t for t in EX_WANT if t[0] != 1] and counts[1] == (0, 0)
    half = _tuples(MM.markers(EX_VAR, EX_SEG, 3, P=0.5)[0])
    assert (0, 9, 1, 4, A_, 1, 2) in half and set(EX_WANT) <= set(half)
    loose = _tuples(MM.markers(EX_VAR, EX_SEG, 3, Q=0.25)[0])
    assert (0, 10, 2, 1, P_, 4, 4) in loose
    assert (0, 1, 2, 4, A_, 1, 2) in loose                              # out = 4 > t_out = 1: still an allele marker


def test_worked_example_texts():
    nk = "k=5\nsamples=6\nsample_names=[\"a0\", \"a1\", \"b0\", \"b1\", \"c0\", \"x\"]\nsample_kmers=[]\n\n" + "".join(
        f"{'ACGT'[i % 4]}{'ACGT'[i // 4]}\tTT\t{','.join(row)}\n" for i, row in enumerate(EXAMPLE)) + "\n"
    groups = [("A", ["a0", "a1"]), ("B", ["b1", "b0"]), ("C", ["c0"])]
    t = MM.texts(nk, groups, fasta=True)
    assert t[".markers.summary.tsv"] == "Group\tSamples\tPresence\tAllele\nA\t2\t1\t3\nB\t2\t1\t1\nC\t1\t1\t0\n"
    assert t[".markers.tsv"] == ("Group\tUpper\tLower\tKind\tIn\tOut\tBases\tOther bases\n"
                                 "A\tAA\tTT\tpresence\t2/2\t0/4\tA\t-\nA\tCA\tTT\tallele\t2/2\t4/4\tA\tC\nA\tGA\tTT\tallele\t2/2\t4/4\tA\tS\n"
                                 "A\tTA\tTT\tallele\t2/2\t4/4\tR\tC\nB\tGA\tTT\tallele\t2/2\t4/4\tC\tR\nB\tGC\tTT\tpresence\t2/2\t0/4\tT\t-\n"
                                 "C\tTC\tTT\tpresence\t1/1\t0/5\tA\t-\n")
    assert t[".A.markers.fa"].split("\n")[6:8] == [">A_4 kind=allele in=2/2 out=4/4 bases=R", "TAATTN"]      # the first of A, C, G, T in the set
    assert t[".B.markers.fa"] == ">B_1 kind=allele in=2/2 out=4/4 bases=C\nGACTTN\n>B_2 kind=presence in=2/2 out=0/4 bases=T\nGCTTTN\n"
    small = MM.texts(nk, groups, min_group_size=2, fasta=True)
    assert small[".markers.summary.tsv"].endswith("C\t1\t-\t-\n") and ".C.markers.fa" not in small
    assert small[".markers.tsv"] == "".join(l + "\n" for l in t[".markers.tsv"].split("\n")[:-1] if not l.startswith("C\t"))


# ---- 2. a second restatement: Python sets, cell by cell ----
_SETS = {c: {b for b, bit in (("A", 1), ("C", 2), ("T", 4), ("G", 8)) if MM.IUPAC.index(c) & bit} for c in MM.IUPAC}


def _by_sets(var, seg, n_groups, reported, P, Q, kinds):
    import math
    U, S = var.shape
    out = []
    for g in range(n_groups):
        if not reported[g]:
            continue
        n = sum(1 for s in range(S) if seg[s] == g)
        t_in, t_out = max(1, math.ceil(n * P)), math.floor((S - n) * Q)
        for r in range(U):
            cells = [_SETS["-" if var[r, s] == 0 else chr(var[r, s])] for s in range(S)]
            mine = [c for s, c in enumerate(cells) if seg[s] == g]
            rest = [c for s, c in enumerate(cells) if seg[s] != g]
            n_in, n_out = sum(1 for c in mine if c), sum(1 for c in rest if c)
            b_in, b_out = set().union(*mine), set().union(*rest)
            if n_in < t_in:
                continue
            kind = P_ if n_out <= t_out else (A_ if not (b_in & b_out) else 0)
            if kind & kinds:
                out.append((g, r, n_in, n_out, kind, sum(MM.IUPAC.index(b) for b in b_in), sum(MM.IUPAC.index(b) for b in b_out)))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_against_the_set_restatement(seed):
    rng = np.random.default_rng(seed)
    S, U, G = int(rng.integers(1, 12)), 160, int(rng.integers(1, 5))
    letters = np.frombuffer((MM.IUPAC + "\0").encode(), np.uint8)
    seg = rng.integers(0, G + 1, size=S).astype(np.int32)
    # a letter per (row, segment), gaps, and some noise: markers of both kinds occur, and so do ambiguous sets and the 0 byte
    var = letters[rng.integers(0, 17, size=(U, G + 1))][:, seg]
    var[rng.random((U, S)) < 0.35] = ord("-")
    noise = rng.random((U, S)) < 0.1
    var[noise] = letters[rng.integers(0, 17, size=int(noise.sum()))]
    reported = [bool((seg == g).any()) and (g % 3 != 2) for g in range(G)]
    seen = set()
    for P, Q, kinds in ((1.0, 0.0, 3), (0.5, 0.1, 3), (0.0, 0.0, 3), (0.75, 0.3, 1), (0.6, 0.0, 2)):
        recs, counts = MM.markers(var, seg, G, reported, P, Q, kinds)
        want = _by_sets(var, seg, G, reported, P, Q, kinds)
        assert _tuples(recs) == want, (seed, P, Q, kinds)
        assert counts == [(sum(1 for t in want if t[0] == g and t[4] == P_), sum(1 for t in want if t[0] == g and t[4] == A_)) for g in range(G)]
        seen |= {t[4] for t in want}
    if S > 2 and any(reported):
        assert seen == {P_, A_}, seed


# ---- 3. - 5. the oracle, on the inputs of tests/subset_model.py ----
@functools.lru_cache(maxsize=None)
def _nk(case):
    return M._oracle_array(case).nk(full_info=True)


def _part(case):
    return PART_TINY if case == "tiny" else PART


@pytest.mark.parametrize("case,group,want", [("k31", (4, 5, 6, 7), 1171), ("k9", (4, 5, 6, 7), 228), ("k41", (4, 5, 6, 7), 1499), ("tiny", (5,), 12)])
def test_private_rows_are_what_the_oracles_delete_drops(case, group, want):
    """rows with in >= 1 and out == 0 (the presence markers at P = 0, Q = 0) = nrows(all) - nrows(after delete_samples(g))"""
    var = M.oracle_export(case)
    seg = MM.partition(var.shape[1], [list(group)])
    _, counts = MM.markers(var, seg, 1, P=0.0, Q=0.0, kinds=P_)
    a = M._oracle_array(case)
    before = a.nrows
    a.delete_samples([M.names_of(case)[i] for i in group])
    assert counts[0][0] == before - a.nrows == want


@pytest.mark.parametrize("case,g,want", [("k31", 0, 543), ("k9", 0, 164), ("k41", 0, 753), ("tiny", 2, 14)])
def test_the_oracles_weed_keeps_exactly_the_marker_rows(case, g, want, tmp_path):
    """weed(reverse=True, min_freq=0) with the model's FASTA of a group leaves exactly that group's marker rows"""
    names = M.names_of(case)
    groups = [(f"g{i}", [names[s] for s in idx]) for i, idx in enumerate(_part(case))]
    t = MM.texts(_nk(case), groups, fasta=True)
    fa = tmp_path / "g.fa"
    fa.write_text(t[f".g{g}.markers.fa"])
    assert t[f".g{g}.markers.fa"].count(">") == want
    _, upper, lower, var = MM.parse_nk(_nk(case))
    recs, _ = MM.markers(var, MM.partition(len(names), _part(case)), len(groups))
    rows = recs["row"][recs["group"] == g].astype(np.int64)
    assert len(rows) == want
    a = M._oracle_array(case)
    a.weed(str(fa), reverse=True, min_freq=0.0)
    assert a.nrows == want
    _, u2, l2, v2 = MM.parse_nk(a.nk(full_info=True))
    assert sorted(zip(u2, l2)) == sorted((upper[r], lower[r]) for r in rows)
    assert sorted(r.tobytes() for r in v2) == sorted(var[r].tobytes() for r in rows)


ANCHORS = {
    ("k31", 1.0, 0.0): [(531, 12), (569, 18), (613, 15), (685, 19)],
    ("k9", 1.0, 0.0): [(145, 19), (95, 7), (124, 14), (83, 11)],
    ("k31", 0.5, 0.1): [(841, 22), (839, 27), (878, 25), (685, 19)],
}


@pytest.mark.parametrize("case,P,Q", sorted(ANCHORS))
def test_anchors(case, P, Q):
    var = M.oracle_export(case)
    recs, counts = MM.markers(var, MM.partition(var.shape[1], PART), len(PART), P=P, Q=Q)
    assert counts == ANCHORS[(case, P, Q)]
    assert len(recs) == sum(p + a for p, a in counts)
    assert (np.diff(recs["group"].astype(np.int64) << 32 | recs["row"].astype(np.int64)) > 0).all()      # sorted by (group, row), each once
