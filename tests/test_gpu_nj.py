"""Device neighbour joining (skx_dist_nj / skx_matrix_nj, csrc/skx_nj.hip) through skx_engine.py (`-m gpu`), against tests/nj_model.py and
against properties that do not depend on the model's rounding: on additive matrices the generating tree comes back; on tied and
non-additive data every chosen pair is a minimum of Q and every length is the formula's when the joins are replayed in numpy; where every
value of a run is exact in float64 the join list equals the model's, ids exactly, so the tie rule itself is tested.  All matrices are made
in numpy; the S = 1 000 case is the largest cost (a few seconds of numpy for nothing but the generating tree, the device run is short)."""
import os

import numpy as np
import pytest

import nj_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "input")
TOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    import skx_engine as E
    E.load_library()
    c = E.Context(0)
    yield c
    c.close()


def _sym(A):
    A = np.triu(np.asarray(A, np.float64), 1)
    return A + A.T


@pytest.mark.parametrize("S", [2, 3, 4, 5, 63, 64, 65, 129, 1000])
def test_additive_matrices_give_back_their_tree(ctx, S):
    rng = np.random.default_rng(100 + S)
    D, truth = M.random_additive(S, rng, 1, 20)
    joins = ctx.matrix_nj(D)
    assert len(joins) == S - 1
    got = M.splits(joins, S)
    assert set(got) == set(truth), (len(set(got) - set(truth)), len(set(truth) - set(got)))
    worst = max(abs(got[s] - truth[s]) for s in truth)
    print(f"S={S}: {len(truth)} splits, worst length error {worst:.3g}")
    assert worst <= TOL


@pytest.mark.parametrize("S", [8, 64, 200])
def test_additive_with_zero_length_branches(ctx, S):
    rng = np.random.default_rng(200 + S)
    D, truth = M.random_additive(S, rng, 0, 3)
    got = M.splits(ctx.matrix_nj(D), S)
    for s, length in truth.items():
        if length > 0:
            assert s in got and abs(got[s] - length) <= TOL, (sorted(s)[:8], length, got.get(s))
    for s, length in got.items():
        if not truth.get(s, 0.0) > 0:
            assert abs(length) <= TOL, (sorted(s)[:8], length)


def _check_replay(D, joins):
    S = D.shape[0]
    assert len(joins) == S - 1
    assert sorted(set(joins["a"]) | set(joins["b"])) == list(range(2 * S - 2)), "every node but the last is joined exactly once"
    worst_q = worst_l = 0.0
    for t, ((q, qmin, la, lb, n, dmax), rec) in enumerate(zip(M.replay(D, joins), joins)):
        tol = TOL * max(n - 2, 1) * max(dmax, 1e-300)
        worst_q, worst_l = max(worst_q, (q - qmin) / tol), max(worst_l, abs(rec["len_a"] - la) / tol, abs(rec["len_b"] - lb) / tol)
        assert q <= qmin + tol, (t, q, qmin, tol)
        assert abs(rec["len_a"] - la) <= tol and abs(rec["len_b"] - lb) <= tol, (t, rec, la, lb, tol)
    print(f"S={S}: worst Q excess {worst_q:.3g} tol, worst length error {worst_l:.3g} tol")


SMALL = [0, 0, 0, 1, 1, 2, 3, 5, 8, 0.5, 12, 40]


@pytest.mark.parametrize("S", [5, 64, 300])
def test_ties_and_non_additive_data_replay(ctx, S):
    rng = np.random.default_rng(300 + S)
    D = _sym(rng.choice(SMALL, (S, S)))
    _check_replay(D, ctx.matrix_nj(D))
    D = _sym(rng.integers(0, 4, (S, S)) * rng.integers(0, 2, (S, S)) + rng.choice([0.0, 0.5], (S, S)))       # mostly zeros and repeats
    _check_replay(D, ctx.matrix_nj(D))


def test_golden_table_replay(ctx):
    import skx_engine as E
    arr = E.Array.load(os.path.join(GOLD, "multidist.skf"), ctx=ctx)
    d, _, _ = arr.distance_filtered()
    S = arr.nsamples
    D = M.tri_to_matrix(d["distance"], S)
    joins = ctx.dist_nj(d, S)
    _check_replay(D, joins)
    arr.free()


@pytest.mark.parametrize("S", [5, 32, 64, 100])
def test_exact_matrices_equal_the_model_join_for_join(ctx, S):
    """entries from a few small integers and a half: every Q, row sum and updated distance of the run is exact in float64, so a tie is a
    tie on both sides and the ids must agree exactly"""
    rng = np.random.default_rng(400 + S)
    D = _sym(rng.choice(SMALL, (S, S)))
    got, want = ctx.matrix_nj(D), M.nj(D)
    assert np.array_equal(got["a"], want["a"]) and np.array_equal(got["b"], want["b"]), np.flatnonzero((got["a"] != want["a"]) | (got["b"] != want["b"]))[:5]
    assert np.abs(got["len_a"] - want["len_a"]).max() <= TOL and np.abs(got["len_b"] - want["len_b"]).max() <= TOL


def test_table_and_matrix_entries_agree_and_runs_repeat(ctx):
    import skx_engine as E
    rng = np.random.default_rng(7)
    S = 97
    D = _sym(rng.choice(SMALL, (S, S)) + rng.random((S, S)))
    d = np.zeros(S * (S - 1) // 2, E.DIST_DT)
    d["distance"] = D[np.triu_indices(S, 1)]
    d["mismatch_prop"] = 0.5
    a, b, c = ctx.dist_nj(d, S), ctx.matrix_nj(D), ctx.matrix_nj(D)
    assert a.tobytes() == b.tobytes() == c.tobytes()
    _check_replay(D, a)


def test_refusals(ctx):
    import skx_engine as E
    D = _sym(np.arange(16.0).reshape(4, 4))
    bad = D.copy(); bad[1, 2] += 1
    with pytest.raises(E.EngineError, match="not symmetric"):
        ctx.matrix_nj(bad)
    bad = D.copy(); bad[2, 2] = 1
    with pytest.raises(E.EngineError, match="diagonal"):
        ctx.matrix_nj(bad)
    with pytest.raises(E.EngineError, match="at least 2"):
        ctx.matrix_nj(np.zeros((1, 1)))
    with pytest.raises(E.EngineError, match="at least 2"):
        ctx.dist_nj(np.zeros(0, E.DIST_DT), 1)
    assert len(ctx.matrix_nj(D)) == 3                    # and the context still works
