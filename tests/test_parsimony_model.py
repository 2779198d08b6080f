"""tests/parsimony_model.py held against what it restates (CPU): a brute-force minimum over every assignment, the identities of Fitch parsimony, a
worked example written out by hand in the model's docstring and two wrong variants of itself; and the host's tree functions
(skh_newick_joins, skh_parsimony_newick, skh_parsimony_branches) through ctypes against the model's reader and writers.  No device is touched."""
import numpy as np
import pytest

import parsimony_model as PM
import skx_engine as E

ALPHABET = np.frombuffer(b"ACGT" * 4 + b"----" + b"MRWSYKVHDBN", np.uint8)        # bases, gaps, every ambiguity code


def _random_var(rng, U, S):
    return ALPHABET[rng.integers(0, len(ALPHABET), size=(U, S))]


# ---- the model against the definition ----
def test_the_worked_example():
    keep = np.ones(5, bool)
    r = PM.fitch(PM.WORKED_VAR, keep, PM.WORKED_JOINS)
    assert r["score"].tolist() == [1, 2, 1, 1, 1]
    assert r["min_score"].tolist() == [1, 1, 1, 1, 0]
    assert [PM.IUPAC[b] for b in r["bases"]] == list("MMRRC")
    got = [(int(c["row"]), int(c["node"]), chr(c["from"]), chr(c["to"])) for c in r["changes"]]
    assert got == [(0, 5, "A", "C"), (1, 3, "A", "C"), (1, 1, "A", "C"), (2, 5, "A", "G"), (3, 5, "A", "G"), (4, 0, "C", "A")]
    assert r["branch_changes"].tolist() == [1, 1, 0, 1, 0, 3]
    assert r["sites"]["row"].tolist() == [1, 4] and r["sites"]["score"].tolist() == [2, 1]
    assert r["info"] == dict(rows_swept=5, rows_variable=5, rows_homoplasic=2, score=6, min_score=4)
    # rows that are not swept give nothing
    keep[[1, 2]] = False
    r = PM.fitch(PM.WORKED_VAR, keep, PM.WORKED_JOINS)
    assert r["score"].tolist() == [1, 0, 0, 1, 1] and r["branch_changes"].tolist() == [1, 0, 0, 0, 0, 2] and r["info"]["rows_swept"] == 3


def test_the_wrong_variants_differ_on_the_worked_example():
    keep = np.ones(5, bool)
    right = PM.fitch(PM.WORKED_VAR, keep, PM.WORKED_JOINS)["score"]
    fifth = PM.fitch(PM.WORKED_VAR, keep, PM.WORKED_JOINS, missing_as_state=True)["score"]
    blind = PM.fitch(PM.WORKED_VAR, keep, PM.WORKED_JOINS, ambiguous_as_missing=True)["score"]
    assert fifth.tolist() == [1, 2, 2, 1, 1] and (fifth != right).tolist() == [False, False, True, False, False]
    assert blind.tolist() == [1, 2, 1, 1, 0] and (blind != right).tolist() == [False, False, False, False, True]


@pytest.mark.parametrize("S", [2, 3, 4, 5])
def test_score_is_the_brute_force_minimum_and_the_sum_of_changes(S):
    rng = np.random.default_rng(S)
    for trial in range(12):
        joins = PM.random_tree(S, rng)
        var = _random_var(rng, 6, S)
        keep = np.ones(6, bool)
        r = PM.fitch(var, keep, joins)
        code = PM.CODE[var]
        for u in range(6):
            assert r["score"][u] == PM.brute_force_score([int(c) for c in code[u]], joins), (joins, var[u].tobytes())
        assert np.array_equal(np.bincount(r["changes"]["row"].astype(np.int64), minlength=6), r["score"])
        assert (r["score"] >= r["min_score"]).all()
        assert r["branch_changes"].sum() == r["score"].sum() == r["info"]["score"]
        # the two branches under the root never both change in the same row
        a, b = joins[-1]
        ra, rb = (set(r["changes"]["row"][r["changes"]["node"] == c].tolist()) for c in (a, b))
        assert not ra & rb


@pytest.mark.parametrize("S", [3, 4, 7, 12])
def test_score_does_not_depend_on_the_root(S):
    rng = np.random.default_rng(100 + S)
    joins = PM.random_tree(S, rng)
    var = _random_var(rng, 200, S)
    keep = np.ones(200, bool)
    want = PM.fitch(var, keep, joins)["score"]
    others = PM.rerooted(joins, S)
    assert len(others) == 2 * S - 3                                   # one rooting per edge of the unrooted tree
    for j in others:
        assert np.array_equal(PM.fitch(var, keep, j)["score"], want), j


def test_trees_of_the_three_shapes():
    for S in (2, 3, 4, 5, 64, 65):
        for joins in (PM.caterpillar(S), PM.balanced(S), PM.random_tree(S, np.random.default_rng(S))):
            PM.check_joins(joins, S)
    assert PM.caterpillar(4) == [(0, 1), (4, 2), (5, 3)] and PM.balanced(4) == [(0, 1), (2, 3), (4, 5)]


# ---- Newick: the model's reader and writer, and the host's ----
def _names(S, rng=None):
    names = [f"s{i:03d}" for i in range(S)]
    if rng is not None:                                              # names the writer has to quote
        for i, extra in zip(rng.permutation(S)[:6], ["it's", "a b", "x(1)", "c,d", "e:f", "[g];"]):
            names[i] += extra
    return names


def _text_of(names, joins, root_three=False, lengths=None, rng=None):
    """a Newick text of the joins with what a reader has to drop: branch lengths, inner labels, comments, white space"""
    tr = PM.Tree(joins, len(names), root_three)
    out, stack = [], [(tr.root, 0)]
    pad = (lambda: "") if rng is None else (lambda: ["", " ", "\n", "[c]", " [a(b,c);] "][rng.integers(0, 5)])
    while stack:
        v, i = stack.pop()
        kids = [] if v < tr.S else tr.kids(v)
        if i == len(kids):
            out.append(PM.newick_name(names[v]) if v < tr.S else ")" + ("" if rng is None or rng.random() < 0.5 else f"'in {v}'" if rng.random() < 0.5 else f"{v / 7:.3f}"))
            if v != tr.root and (rng is None or rng.random() < 0.8):
                out.append(pad() + ":" + pad() + ("1e-3" if lengths is None else str(lengths[v])))
            out.append(pad())
            continue
        out.append(("(" if i == 0 else ",") + pad())
        stack.append((v, i + 1))
        stack.append((kids[i], 0))
    return pad() + "".join(out) + ";" + pad()


def _both(text, names):
    """the model's reader and the host's give the same joins"""
    want, three = PM.newick_joins(text, names)
    got, got_three = E.newick_joins(text, names)
    assert [(int(a), int(b)) for a, b in zip(got["a"], got["b"])] == want and got_three == three
    return want, three


@pytest.mark.parametrize("S", [2, 3, 4, 9, 40])
def test_reader_and_writer_round_trip_on_random_trees(S):
    rng = np.random.default_rng(7 * S)
    for trial in range(6):
        names = _names(S, rng if S >= 9 else None)
        joins = PM.random_tree(S, rng)
        # a text lists a node's inner children before the node: renumber the joins in the order of their ')'
        joins, three = PM.newick_joins(_text_of(names, joins), names)
        text = _text_of(names, joins, rng=rng)
        got, three = _both(text, names)
        assert got == joins and not three
        changes = rng.integers(0, 1000, size=2 * S - 2)
        nwk = PM.parsimony_newick(names, joins, False, changes)
        assert E.parsimony_newick(names, joins, False, changes) == nwk
        assert E.parsimony_branches(names, joins, False, changes) == PM.branches_text(names, joins, False, changes)
        # what was written reads back as the same tree, and its lengths are the changes
        assert _both(nwk, names) == (joins, False)


def test_a_written_example():
    names = ["a", "b c", "d", "e"]
    joins, three = _both("((a:1,'b c':2)x:0.5,(d,e));", names)
    assert joins == [(0, 1), (2, 3), (4, 5)] and not three
    changes = [3, 0, 1, 2, 5, 7]
    assert E.parsimony_newick(names, joins, False, changes) == "((a:3,'b c':0)n1:5,(d:1,e:2)n2:7);\n"
    assert E.parsimony_branches(names, joins, False, changes) == (
        "Node\tParent\tLeaves\tLowest leaf\tChanges\na\tn1\t1\ta\t3\nb c\tn1\t1\tb c\t0\nd\tn2\t1\td\t1\ne\tn2\t1\te\t2\nn1\troot\t2\ta\t5\nn2\troot\t2\td\t7\n")
    assert PM.branches_text(names, joins, False, changes) == E.parsimony_branches(names, joins, False, changes)


def test_a_trifurcating_root_read_three_ways():
    """(a, b, c) at the root becomes R = (a, Y), Y = (b, c).  Whichever child comes first, every row keeps its score and the tree its length, and
    the rows that change above a and above Y are never the same, so the branch above a is changes(a) + changes(Y) exactly.  Where a row's changes
    lie is Fitch's choice among equally short reconstructions and may differ between the three readings: A, C, G on the three branches cost two
    changes, and the reading decides which two branches carry them."""
    rng = np.random.default_rng(3)
    names = _names(7)
    var = _random_var(rng, 400, 7)
    keep = np.ones(400, bool)
    sub = {"A": "(s000,s001)", "B": "((s002,s003),s004)", "C": "(s005,s006)"}
    scores, totals = [], []
    for order in ("ABC", "BCA", "CAB"):
        text = "(" + ",".join(sub[x] for x in order) + ");"
        joins, three = _both(text, names)
        assert three and joins[-1][1] == 2 * 7 - 3
        r = PM.fitch(var, keep, joins)
        tr = PM.Tree(joins, 7, True)
        ln = tr.lengths(r["branch_changes"])
        a, y = joins[-1]
        rows_a, rows_y = (set(r["changes"]["row"][r["changes"]["node"] == c].tolist()) for c in (a, y))
        assert not rows_a & rows_y and ln[a] == len(rows_a) + len(rows_y) == len(rows_a | rows_y) and len(rows_y) > 0
        assert len(ln) == 12 and ln[tr.hidden] == 0
        scores.append(r["score"])
        totals.append(sum(ln))
        nwk = PM.parsimony_newick(names, joins, True, r["branch_changes"])
        assert E.parsimony_newick(names, joins, True, r["branch_changes"]) == nwk and nwk.count("(") == 5 and nwk.count(":") == 11
        assert _both(nwk, names) == (joins, True)
        branches = PM.branches_text(names, joins, True, r["branch_changes"])
        assert E.parsimony_branches(names, joins, True, r["branch_changes"]) == branches
        assert branches.count("\n") == 12 and branches.count("\troot\t") == 3 and f"n{tr.hidden - 7 + 1}" not in branches
    assert np.array_equal(scores[0], scores[1]) and np.array_equal(scores[0], scores[2])
    assert totals[0] == totals[1] == totals[2] == int(scores[0].sum()) > 0
    # the three bases on the three branches: two changes in every reading, on two different pairs of branches
    tri = np.array([list(b"ACG")], np.uint8)
    got = []
    for text in ("(s000,s001,s002);", "(s001,s002,s000);", "(s002,s000,s001);"):
        joins, three = _both(text, _names(3))
        r = PM.fitch(tri, np.ones(1, bool), joins)
        got.append(PM.Tree(joins, 3, True).lengths(r["branch_changes"])[:3])
    assert got == [[1, 0, 1], [0, 1, 1], [0, 1, 1]]                   # (worked by hand: the root's state is A, the lowest bit, in all three)


def test_caterpillars_of_5000_leaves():
    S = 5000
    names = _names(S)
    for joins in (PM.caterpillar(S), [(1, 0)] + [(t + 1, S + t - 1) for t in range(1, S - 1)]):      # nested on the left, and on the right
        text = _text_of(names, joins)
        depth = np.cumsum([(c == "(") - (c == ")") for c in text])
        assert depth.max() == S - 1 and depth[-1] == 0
        got, three = _both(text, names)
        assert got == joins and not three
        changes = np.arange(2 * S - 2)
        assert E.parsimony_newick(names, joins, False, changes) == PM.parsimony_newick(names, joins, False, changes)
        assert E.parsimony_branches(names, joins, False, changes) == PM.branches_text(names, joins, False, changes)


REFUSALS = [
    ("((a,b,c),d);", "position 7: a node with 3 children (only the root may have three)"),
    ("(a,b,c,d);", "position 8: a node with 4 children (only the root may have three)"),
    ("((a),b,c,d);", "position 3: a node with one child"),
    ("((a,b),(c,x));", "position 10: leaf 'x' is not a sample of the array"),
    ("((a,b),(c,a));", "position 10: sample 'a' is named twice"),
    ("((a,b),c);", "sample 'd' is missing from the tree"),
    ("((a,b),(c,d)); x", "position 15: text after the tree"),
    ("((a,b),(c,d))(", "position 13: text after the tree"),
    ("((a,b),(c,d)", "position 12: the text ends inside the tree"),
    ("((a,b),(c,d))", "position 13: the text ends inside the tree"),
    ("((a,b),(c,d);", "position 12: the tree ends inside a node"),
    ("((a,b),(c,d)));", "position 13: text after the tree"),
    ("((a,b),(c,'d));", "position 10: a quoted label without its end"),
    ("((a,b),[(c,d));", "position 7: a comment without its end"),
    ("((a,b),(c,));", "position 10: a leaf without a name"),
    ("((a,b),(,c),d);", "position 8: a ',' without a node before it"),
    ("((a,b)(c,d));", "position 6: unexpected character '('"),
    ("((a b),(c,d));", "position 4: unexpected character 'b'"),
    ("();", "position 1: a leaf without a name"),
    (";", "position 0: a tree without a node"),
    ("", "position 0: the text ends inside the tree"),
    ("a;", "sample 'b' is missing from the tree"),
]


@pytest.mark.parametrize("text,why", REFUSALS)
def test_refusals(text, why):
    names = ["a", "b", "c", "d"]
    with pytest.raises(ValueError) as mi:
        PM.newick_joins(text, names)
    assert str(mi.value) == "newick: " + why
    with pytest.raises(E.EngineError) as ei:
        E.newick_joins(text, names)
    assert ei.value.code == E.EINVAL and str(ei.value) == f"[skx {E.EINVAL}] newick: {why}"


def test_every_truncation_of_a_text_is_refused_alike():
    names = ["a", "b c", "d", "e"]
    text = " ( (a:1 , 'b c'[x]:2e-1)'l''1':0.5,(d,e)[y]:3 ) ; "
    assert _both(text, names)[0] == [(0, 1), (2, 3), (4, 5)]
    for cut in range(len(text.rstrip()) - 1):
        with pytest.raises(ValueError) as mi:
            PM.newick_joins(text[:cut], names)
        with pytest.raises(E.EngineError) as ei:
            E.newick_joins(text[:cut], names)
        assert str(ei.value) == f"[skx {E.EINVAL}] {mi.value}", cut


def test_the_writers_refuse_a_table_that_is_not_a_tree():
    names = ["a", "b", "c"]
    for joins in ([(0, 1), (2, 4)], [(0, 1), (0, 3)], [(0, 0), (1, 2)]):
        with pytest.raises(E.EngineError) as ei:
            E.parsimony_newick(names, joins, False, [0, 0, 0, 0])
        assert ei.value.code == E.EINVAL and "skh_parsimony_newick:" in str(ei.value)
    with pytest.raises(E.EngineError):
        E.parsimony_branches(names, [(0, 1), (3, 2)], True, [0, 0, 0, 0])      # the root's second child is not node 2S-3


# ---- the texts of the record files ----
def test_record_texts():
    k = 7
    keys = np.zeros(5, E.KEY_DT)
    keys["lo"] = [0b000110_011011, 0b000000_000001, 0b111111_000000, 0b010101_101010, 0b000000_000000]
    r = PM.fitch(PM.WORKED_VAR, np.ones(5, bool), PM.WORKED_JOINS)
    assert PM.homoplasies_text(keys, k, r["sites"], r["min_score"]) == "Upper\tLower\tBases\tScore\tMinimum\nAAA\tAAA\tC\t1\t0\nAAA\tAAC\tM\t2\t1\n"
    assert PM.summary_text(r["info"]) == "Rows swept\t5\nRows variable\t5\nRows homoplasic\t2\nScore\t6\nMinimum score\t4\nConsistency index\t0.666667\n"
    assert PM.summary_text(dict(rows_swept=3, rows_variable=0, rows_homoplasic=0, score=0, min_score=0)).endswith("Consistency index\tNA\n")
    names = ["w", "x", "y", "z"]
    assert PM.changes_text(names, PM.WORKED_JOINS, False, keys, k, r["changes"]) == (
        "Branch\tUpper\tLower\tFrom\tTo\nw\tAAA\tAAA\tC\tA\nx\tAAA\tAAC\tA\tC\nz\tAAA\tAAC\tA\tC\nn2\tACT\tCTG\tA\tC\nn2\tCCC\tTTT\tA\tG\nn2\tGGG\tAAA\tA\tG\n")
