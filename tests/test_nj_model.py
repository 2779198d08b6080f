"""CPU checks of the yardstick of `ska distance --tree / --clusters` (tests/nj_model.py) and of the two host-only entry points it is
compared with (skh_nj_newick, skh_distance_clusters: no device is touched).  On additive matrices neighbour joining must return the
generating tree, and with integer branch lengths every value of the run is exact in float64, so the comparisons are `==`."""
import numpy as np
import pytest

import nj_model as M
import skx_engine as E


def _joins(rows):
    out = np.zeros(len(rows), M.NJ_DT)
    for i, r in enumerate(rows):
        out[i] = r
    return out


@pytest.mark.parametrize("S", [3, 4, 5, 8, 33, 64, 65, 200, 400])
def test_model_recovers_additive_trees_exactly(S):
    rng = np.random.default_rng(1000 + S)
    D, truth = M.random_additive(S, rng, 1, 20)
    got = M.splits(M.nj(D), S)
    assert got == truth
    if S <= 65:
        assert M.splits(M.nj(D, recompute=True), S) == truth


@pytest.mark.parametrize("S", [3, 4, 5, 8, 33, 64, 65, 200, 400])
def test_model_with_zero_length_branches(S):
    rng = np.random.default_rng(2000 + S)
    D, truth = M.random_additive(S, rng, 0, 3)
    got = M.splits(M.nj(D), S)
    for s, length in truth.items():
        if length > 0:
            assert got.get(s) == length, (sorted(s), length, got.get(s))
    for s, length in got.items():
        if not truth.get(s, 0.0) > 0:
            assert length == 0, (sorted(s), length)


def test_model_tie_rule_and_record_form():
    # all distances equal: every Q ties at every step, so the lowest (min id, max id) is what decides
    D = np.ones((5, 5)) - np.eye(5)
    j = M.nj(D)
    assert [(int(r["a"]), int(r["b"])) for r in j] == [(0, 1), (2, 3), (4, 5), (6, 7)]
    assert j[-1]["len_b"] == 0 and j[-1]["len_a"] == 0           # a star: every leaf 0.5 from the one centre
    assert j[0]["len_a"] == 0.5 and j[0]["len_b"] == 0.5
    two = M.nj(np.array([[0.0, 7.0], [7.0, 0.0]]))
    assert two.tolist() == [(0, 1, 7.0, 0.0)]
    # replay of the model's own joins: the chosen pair is a minimum and the lengths are the formula's
    rng = np.random.default_rng(5)
    A = rng.choice([0, 0, 0, 1, 1, 2, 3, 5, 8, 0.5, 12, 40], (32, 32))
    A = np.triu(A, 1) + np.triu(A, 1).T
    jj = M.nj(A)
    for (q, qmin, la, lb, n, dmax), rec in zip(M.replay(A, jj), jj):
        assert q == qmin and rec["len_a"] == la and rec["len_b"] == lb
    assert np.array_equal(jj, M.nj(A, recompute=True))


NAMES4 = ["s0", "s1", "s2", "s3"]
# ((s0:1,s1:2):3,(s2:4,s3:5)) unrooted: joins (0,1)->4, then (2,3) as the last-but-one ... written by hand
JOINS4 = [(0, 1, 1.0, 2.0), (2, 3, 4.0, 5.0), (4, 5, 3.0, 0.0)]


def _both(names, rows):
    j = _joins(rows)
    a, b = M.newick(names, j), E.nj_newick(names, j)
    assert a == b
    return a


def test_newick_midpoint_root_and_child_order():
    # furthest pair: s1 - s3 = 2 + 3 + 5 = 10, so the root is 5 from s1: 2 up s1's branch, then 3 along the inner branch = at node 5's end
    text = _both(NAMES4, JOINS4)
    assert text == "((s0:1.00000,s1:2.00000):3.00000,(s2:4.00000,s3:5.00000):0.00000);\n"
    # a root inside a leaf branch, and children ordered by their lowest leaf, not by the order of the joins
    text = _both(NAMES4, [(2, 3, 1.0, 1.0), (1, 4, 1.0, 1.0), (0, 5, 20.0, 0.0)])
    assert text == "(s0:11.00000,(s1:1.00000,(s2:1.00000,s3:1.00000):1.00000):9.00000);\n"
    assert _both(["a", "b"], [(0, 1, 3.0, 0.0)]) == "(a:1.50000,b:1.50000);\n"
    # ties in the furthest pair go to the lowest (id, id): all leaves 2 apart -> (0, 1), root in the middle of the path 0 - 4 - 1
    text = _both(["a", "b", "c"], [(0, 1, 1.0, 1.0), (2, 3, 1.0, 0.0)])
    assert text == "(a:1.00000,(b:1.00000,c:1.00000):0.00000);\n"


def test_newick_negative_lengths_move_to_the_sibling():
    # raw -0.5 / 2.5 keeps the 2.0 between the two joined nodes: 0 / 2.0
    text = _both(NAMES4, [(0, 1, -0.5, 2.5), (2, 3, 4.0, 5.0), (4, 5, 3.0, 0.0)])
    sp, _ = M.newick_splits(text, NAMES4)
    assert sp[frozenset([1])] == 2.0 and sp[frozenset([1, 2, 3])] == 0.0
    text = _both(NAMES4, [(0, 1, 2.5, -0.5), (2, 3, 4.0, 5.0), (4, 5, 3.0, 0.0)])
    sp, _ = M.newick_splits(text, NAMES4)
    assert sp[frozenset([1])] == 0.0 and sp[frozenset([1, 2, 3])] == 2.0


def test_newick_quoting_and_parser_round_trip():
    names = ["plain_1.fa", "has space", "it's", "a(b)", "semi;colon", "co,mma", "br[x]", "c:d"]
    rng = np.random.default_rng(3)
    D, truth = M.random_additive(len(names), rng, 1, 9)
    j = M.nj(D)
    text = _both(names, j)
    for q in ("'has space'", "'it''s'", "'a(b)'", "'semi;colon'", "'co,mma'", "'br[x]'", "'c:d'"):
        assert q in text
    assert "'plain_1.fa'" not in text and "plain_1.fa:" in text
    sp, (d0, d1) = M.newick_splits(text, names)
    assert sp == {s: float(v) for s, v in truth.items()}
    assert abs(d0 - d1) < 1e-4                      # midpoint: the deepest leaves on both sides are equally far (to the printed decimals)


@pytest.mark.parametrize("S", [5, 33, 200])
def test_newick_of_random_trees_matches_the_writer_under_test(S):
    rng = np.random.default_rng(4000 + S)
    D, truth = M.random_additive(S, rng, 0, 3)
    D += rng.choice([0.0, 0.5], D.shape)             # not additive any more: negative raw lengths appear
    D = np.triu(D, 1) + np.triu(D, 1).T
    names = [f"n{i}" for i in range(S)]
    j = M.nj(D)
    text = _both(names, j)
    sp, (d0, d1) = M.newick_splits(text, names)
    assert len(sp) == 2 * S - 3 and abs(d0 - d1) < 1e-4 * S


def _table(n, vals):
    d = np.zeros(n * (n - 1) // 2, E.DIST_DT)
    for i, (snps, mism) in enumerate(vals):
        d[i] = (snps, mism, 0, 0)
    return d


def test_clusters_numbering_rounding_and_files():
    names = ["a", "b", "c", "d", "e", "f"]
    big = (99.0, 0.9)
    # pairs row-major: ab ac ad ae af bc bd be bf cd ce cf de df ef
    vals = [big] * 15
    pair = {(i, j): k for k, (i, j) in enumerate((i, j) for i in range(6) for j in range(i + 1, 6))}
    vals[pair[(3, 4)]] = (1.0, 0.01)                 # d - e
    vals[pair[(4, 5)]] = (2.0, 0.050004)             # e - f: passes 0.05 only as printed (0.05000)
    vals[pair[(1, 2)]] = (2.004, 0.01)               # b - c: 2.00 as printed
    vals[pair[(0, 1)]] = (2.0, 0.049996)             # a - b: prints 0.05000 too, passes
    vals[pair[(0, 3)]] = (2.0, 0.050006)             # a - d: prints 0.05001, fails
    vals[pair[(2, 5)]] = (2.006, 0.01)               # c - f: prints 2.01, fails
    d = _table(6, vals)
    csv, dot = E.distance_clusters(names, d, 2.0, 0.05)
    assert csv == "id,Cluster__autocolour\na,1\nb,1\nc,1\nd,2\ne,2\nf,2\n"
    assert dot == ('strict graph {\n\t"a";\n\t"b";\n\t"c";\n\t"d";\n\t"e";\n\t"f";\n\t"a" -- "b";\n\t"b" -- "c";\n\t"d" -- "e";\n\t"e" -- "f";\n}\n')
    # the model on the text of the same table
    rows = [(i, j, float("%.2f" % d[k]["distance"]), float("%.5f" % d[k]["mismatch_prop"])) for (i, j), k in pair.items()]
    part, mcsv, mdot = M.clusters(names, rows, 2.0, 0.05)
    assert (mcsv, mdot) == (csv, dot) and part == [[0, 1, 2], [3, 4, 5]]
    # sizes decide the numbers, ties by the lowest sample: {c} {a} stay behind {d, e, f} and {b ...}
    vals2 = [big] * 15
    vals2[pair[(3, 4)]] = vals2[pair[(4, 5)]] = (0.0, 0.0)
    vals2[pair[(1, 2)]] = (0.0, 0.0)
    csv, _ = E.distance_clusters(names, _table(6, vals2), 10.0, 1.0 - 0.5)
    assert csv == "id,Cluster__autocolour\nd,1\ne,1\nf,1\nb,2\nc,2\na,3\n"
    # a value that passes its threshold as stored and fails it as printed: 0.049996 <= 0.049998 < 0.05000
    one = _table(2, [(1.0, 0.049996)])
    assert E.distance_clusters(["x", "y"], one, 10.0, 0.049998)[0] == "id,Cluster__autocolour\nx,1\ny,2\n"
    assert M.clusters(["x", "y"], [(0, 1, 1.0, float("%.5f" % 0.049996))], 10.0, 0.049998)[0] == [[0], [1]]
    assert E.distance_clusters(["x", "y"], one, 10.0, 0.05)[0] == "id,Cluster__autocolour\nx,1\ny,1\n"
    # everything / nothing
    assert E.distance_clusters(names, _table(6, vals), 1000.0, 1.0)[0].splitlines()[1:] == [f"{n},1" for n in names]
    assert E.distance_clusters(names, _table(6, vals), 0.0, 0.0)[0].splitlines()[1:] == [f"{n},{i + 1}" for i, n in enumerate(names)]


def test_clusters_quoting():
    names = ['x,y', 'q"r', "back\\slash"]
    csv, dot = E.distance_clusters(names, _table(3, [(0.0, 0.0), (50.0, 0.0), (50.0, 0.0)]), 10.0, 1.0)
    assert csv == 'id,Cluster__autocolour\n"x,y",1\n"q""r",1\nback\\slash,2\n'
    assert dot == 'strict graph {\n\t"x,y";\n\t"q\\"r";\n\t"back\\\\slash";\n\t"x,y" -- "q\\"r";\n}\n'
    _, mcsv, mdot = M.clusters(names, [(0, 1, 0.0, 0.0), (0, 2, 50.0, 0.0), (1, 2, 50.0, 0.0)], 10.0, 1.0)
    assert (mcsv, mdot) == (csv, dot)


def test_host_entry_points_refuse_bad_arguments():
    with pytest.raises(E.EngineError):
        E.nj_newick(["a", "b", "c"], _joins([(0, 1, 1.0, 1.0), (2, 9, 1.0, 0.0)]))      # a node that does not exist
