"""The selection model (tests/select_model.py) on hand-made tables and on the golden tables' text: the union rule, the index tie at the K-th
place, K >= S - 1, fewer than K candidates, a threshold equal to a value.  No device."""
import os

from select_model import select, select_text, table_arrays

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "correct")


def _sym(S, pairs, fill=0.0):
    m = [[fill] * S for _ in range(S)]
    for (i, j), v in pairs.items():
        m[i][j] = m[j][i] = v
    return m


def _full(S):
    return {(i, j) for i in range(S) for j in range(i + 1, S)}


def test_union_rule_keeps_a_line_for_one_side_only():
    # 0 and 1 are each other's nearest; 2 is nearest to 0, but 0's nearest is 1: (0, 2) is kept because of 2 alone; 3 likewise through 2
    D = _sym(4, {(0, 1): 1, (0, 2): 2, (0, 3): 9, (1, 2): 3, (1, 3): 9, (2, 3): 4})
    M = _sym(4, {})
    assert select(D, M, closest=1) == {(0, 1), (0, 2), (2, 3)}
    # K = 2: 3's second place is a tie at 9 between 0 and 1, which the lower index takes
    assert select(D, M, closest=2) == {(0, 1), (0, 2), (1, 2), (2, 3), (0, 3)}


def test_index_tie_at_the_kth_place():
    # sample 0 is at distance 5 from 1, 2 and 3: K = 1 takes 1, K = 2 takes 1 and 2; the others see 0 first (distance 5 against 7)
    D = _sym(4, {(0, 1): 5, (0, 2): 5, (0, 3): 5, (1, 2): 7, (1, 3): 7, (2, 3): 7})
    M = _sym(4, {})
    assert select(D, M, closest=1) == {(0, 1), (0, 2), (0, 3)}
    D5 = _sym(5, {p: 5 for p in _full(5)})
    assert select(D5, _sym(5, {}), closest=1) == {(0, 1), (0, 2), (0, 3), (0, 4)}
    assert select(D5, _sym(5, {}), closest=2) == {(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4)}


def test_k_at_least_s_minus_one_is_no_constraint():
    D = _sym(5, {p: float(sum(p)) for p in _full(5)})
    M = _sym(5, {p: 0.1 * p[0] for p in _full(5)})
    for K in (4, 5, 100):
        assert select(D, M, closest=K) == _full(5)
        assert select(D, M, max_snps=4, closest=K) == select(D, M, max_snps=4)
    assert select(D, M, closest=3) != _full(5)


def test_fewer_than_k_candidates():
    # the threshold leaves sample 3 one candidate and sample 4 none
    D = _sym(5, {(0, 1): 1, (0, 2): 1, (1, 2): 1, (0, 3): 2, (1, 3): 8, (2, 3): 8, (0, 4): 9, (1, 4): 9, (2, 4): 9, (3, 4): 9})
    M = _sym(5, {})
    assert select(D, M, max_snps=2, closest=3) == {(0, 1), (0, 2), (1, 2), (0, 3)}
    assert select(D, M, max_snps=2, closest=1) == {(0, 1), (0, 2), (0, 3)}


def test_threshold_equal_to_a_value_keeps_it():
    D = _sym(4, {(0, 1): 1.5, (0, 2): 2.0, (0, 3): 2.5, (1, 2): 2.0, (1, 3): 3.0, (2, 3): 0.0})
    M = _sym(4, {(0, 1): 0.25, (0, 2): 0.5, (0, 3): 0.5, (1, 2): 0.75, (1, 3): 0.0, (2, 3): 1.0})
    assert select(D, M, max_snps=2.0) == {(0, 1), (0, 2), (1, 2), (2, 3)}
    assert select(D, M, max_snps=0.0) == {(2, 3)}
    assert select(D, M, max_mismatches=0.5) == {(0, 1), (0, 2), (0, 3), (1, 3)}
    assert select(D, M, max_mismatches=0.0) == {(1, 3)}
    assert select(D, M, max_snps=2.0, max_mismatches=0.5) == {(0, 1), (0, 2)}
    # thresholds before the ranking: 2's nearest overall is 3 (distance 0), which the mismatch threshold removes
    assert select(D, M, max_mismatches=0.5, closest=1) == {(0, 1), (0, 2), (0, 3)}


def _golden(name):
    return open(os.path.join(GOLD, name)).read()


def _named(text, kept):
    names = table_arrays(text)[0]
    return {(names[i], names[j]) for i, j in kept}


def test_golden_multidist_cases():
    text = _golden("multidist.stdout")
    names, D, M, _ = table_arrays(text)
    assert names == ["N_test_1", "N_test_2", "ambig_test_1", "ambig_test_2", "test_1", "test_2"]
    assert sum(1 for i in range(6) for j in range(i + 1, 6) if D[i][j] == 0.0 and M[i][j] == 1.0) == 8
    assert len(select(D, M, max_mismatches=0.6)) == 7
    assert len(select(D, M, max_mismatches=0.6, max_snps=1)) == 5
    assert _named(text, select(D, M, closest=1, max_mismatches=0.6)) == {
        ("N_test_1", "test_1"), ("N_test_1", "test_2"), ("N_test_2", "test_1"), ("ambig_test_1", "ambig_test_2")}
    assert len(select_text(text, max_mismatches=0.6).splitlines()) == 8 and select_text(text, closest=5) == text


def test_golden_minfreq_all_pairs_equal():
    text = _golden("multidist.minfreq.stdout")
    _, D, M, _ = table_arrays(text)
    assert len({D[i][j] for i in range(6) for j in range(6) if i != j}) == 1
    assert _named(text, select(D, M, closest=1)) == {("N_test_1", n) for n in ("N_test_2", "ambig_test_1", "ambig_test_2", "test_1", "test_2")}
