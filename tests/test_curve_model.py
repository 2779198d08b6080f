"""tests/curve_model.py (the model `ska curve` is held to on the GPU) against what it must equal: tests/subset_model.py -- the restatement of the
oracle's delete_samples + filter the engine's subsets are held to -- for every prefix, the oracle chain itself for a few, a hand-worked example,
a cell-by-cell restatement, and written-out orders of the seeded generator.  Two wrong variants of the model (floor for ceil in the threshold,
ambiguous cells counted as bases) must fail these checks.  The host-only halves of the C++ side (skh_curve_orders, skh_curve_tsv) are held to
the model here too: they need no device.  CPU only."""
import math

import numpy as np
import pytest

import curve_model as CM
import subset_model as M

Opts = M.Opts
FREQS = (0.0, 0.5, 0.6, 0.9, 1.0)


def _against_subset_model(case, order, ts, f, **wrong):
    """the four counts of the prefixes ts of one order against subset_model.model -> how many (t, count) were compared"""
    var = M.oracle_export(case)
    got = CM.curve(var, [order], f, **wrong)[0]
    for t in ts:
        prefix = [int(s) for s in order[:t]]
        _, plain = M.model(var, prefix, Opts((f, False, 0, False, True)))
        _, sites = M.model(var, prefix, Opts((f, False, 3, False, True)))
        want = (plain["rows_present"], plain["kept"], sites["kept"])
        assert (int(got[t - 1, 0]), int(got[t - 1, 1]), int(got[t - 1, 3])) == want, (case, list(order), t, f)
    return len(ts)


def test_tiny_every_prefix_of_several_orders():
    S = M.CASES["tiny"]["S"]
    orders = [list(range(S)), list(range(S))[::-1]] + CM.orders(3, S, 4).tolist()
    for f in FREQS:
        for o in orders:
            _against_subset_model("tiny", o, range(1, S + 1), f)
    var = M.oracle_export("tiny")
    assert CM.curve(var, orders, 0.9)[:, :, 2].max() > 0 and CM.curve(var, orders, 0.9)[:, :, 3].max() > 0       # the case has variant sites to count


def test_k31_a_sample_of_orders_and_prefixes():
    S = M.CASES["k31"]["S"]
    rng = np.random.default_rng(31)
    for o in CM.orders(11, S, 3).tolist():
        for f in (0.6, 0.9):
            _against_subset_model("k31", o, sorted({1, S} | {int(t) for t in rng.integers(2, S, size=3)}), f)


def test_variant_is_the_no_min_freq_alignment():
    """variant = core_variant at min_freq 0 (thr = 1: every present row is core), which subset_model pins too"""
    var = M.oracle_export("tiny")
    S = var.shape[1]
    o = CM.orders(5, S, 1)[0].tolist()
    got = CM.curve(var, [o], 0.0)[0]
    assert np.array_equal(got[:, 2], got[:, 3]) and np.array_equal(got[:, 0], got[:, 1])
    assert np.array_equal(got[:, 2], CM.curve(var, [o], 0.9)[0][:, 2])                  # variant and pan do not depend on min_freq
    for t in range(1, S + 1):
        assert int(got[t - 1, 2]) == M.model(var, o[:t], Opts((0.0, False, 3, False, True)))[1]["kept"]


@pytest.mark.parametrize("case,prefix,f", [("tiny", (4, 1, 2), 0.6), ("tiny", (0, 1, 2, 3, 4, 5), 0.9), ("k9", (7, 3, 11, 0, 5), 0.9)])
def test_oracle_chain_for_a_few_prefixes(case, prefix, f):
    var = M.oracle_export(case)
    S = var.shape[1]
    order = list(prefix) + [s for s in range(S) if s not in prefix]
    got = CM.curve(var, [order], f)[0][len(prefix) - 1]
    group = tuple(sorted(prefix))
    cols, nrows, removed = M.oracle_chain(case, group, Opts((f, False, 0, False, True)))
    assert (int(got[0]), int(got[1])) == (nrows, len(cols))
    cols, _, _ = M.oracle_chain(case, group, Opts((f, False, 3, False, True)))
    assert int(got[3]) == len(cols)


# ---- a hand-worked example: 6 rows x 4 samples ----
HAND = np.array([list(r.encode()) for r in (
    "AAAA",      # constant and everywhere
    "NR-Y",      # only ambiguous cells: present, never variant
    "AAAC",      # the second base arrives with the last sample
    "-AC-",      # variant from the third sample on; at f = 0.9 never core (n = 0, 1, 2, 2 against 1, 2, 3, 4)
    "A--A",      # at f = 0.5 core, not core, core again (n = 1, 1, 1, 2 against 1, 1, 2, 2)
    "----",      # no cell present
)], np.uint8)
#                                 pan            core           variant        core_variant
HAND_WANT = {
    ((0, 1, 2, 3), 0.5): ([4, 5, 5, 5], [4, 5, 4, 5], [0, 0, 1, 2], [0, 0, 1, 2]),
    ((0, 1, 2, 3), 0.9): ([4, 5, 5, 5], [4, 3, 2, 2], [0, 0, 1, 2], [0, 0, 0, 1]),
    ((3, 2, 1, 0), 0.5): ([4, 5, 5, 5], [4, 5, 4, 5], [0, 1, 2, 2], [0, 1, 2, 2]),
}


def _hand(**wrong):
    for (order, f), want in HAND_WANT.items():
        got = CM.curve(HAND, [order], f, **wrong)[0]
        assert got.T.tolist() == [list(w) for w in want], (order, f)


def test_hand_worked_example():
    _hand()
    core = HAND_WANT[((0, 1, 2, 3), 0.5)][1]
    assert core[1] > core[2] < core[3]                                  # core goes down and up again
    for (order, f) in HAND_WANT:
        assert CM.curve(HAND, [order], f)[0].tolist() == CM.curve_slow(HAND, list(order), f)
    assert CM.thresholds(4, 0.9).tolist() == [1, 2, 3, 4] and CM.thresholds(4, 0.5).tolist() == [1, 1, 2, 2] and CM.thresholds(3, 0.0).tolist() == [1, 1, 1]


def test_cell_by_cell_restatement_on_random_matrices():
    rng = np.random.default_rng(8)
    letters = np.frombuffer(b"-ACGTMRWSYKVHDBN\0", np.uint8)
    for U, S in ((40, 7), (9, 1), (25, 12)):
        var = letters[rng.integers(0, len(letters), size=(U, S))]
        var[rng.random((U, S)) < 0.4] = ord("-")
        for o in CM.orders(U, S, 2).tolist():
            for f in (0.0, 1e-9, 0.5, 0.9, 1.0):
                assert CM.curve(var, [o], f)[0].tolist() == CM.curve_slow(var, o, f), (U, S, f)


@pytest.mark.parametrize("wrong", [dict(rounding=math.floor), dict(ambiguous_are_bases=True)])
def test_wrong_variants_are_caught(wrong):
    with pytest.raises(AssertionError):
        _hand(**wrong)
    S = M.CASES["tiny"]["S"]
    with pytest.raises(AssertionError):
        for o in ([list(range(S))] + CM.orders(3, S, 4).tolist()):
            _against_subset_model("tiny", o, range(1, S + 1), 0.9, **wrong)
    with pytest.raises(AssertionError):
        _against_subset_model("k31", CM.orders(11, 13, 1)[0].tolist(), range(1, 14), 0.9, **wrong)


# ---- the seeded orders ----
def test_generator_stream_and_first_orders():
    g = CM.SplitMix64(1234567)                                          # the published test vector of splitmix64
    assert [g.next() for _ in range(3)] == [6457827717110365317, 3203168211198807973, 9817491932198370423]
    assert CM.SplitMix64(0).next() == 0xE220A8397B1DCDAF
    # by hand from that vector: i = 2 takes j = 6457827717110365317 mod 3 = 0 (its digits sum to 81), i = 1 takes j = ...973 mod 2 = 1
    assert CM.orders(1234567, 3, 1).tolist() == [[2, 1, 0]]
    assert CM.orders(1, 13, 2).tolist() == [[1, 9, 4, 2, 12, 8, 11, 10, 3, 5, 0, 7, 6], [4, 2, 3, 5, 7, 8, 6, 1, 0, 9, 12, 10, 11]]
    assert CM.orders(7, 6, 3).tolist() == [[1, 5, 0, 2, 4, 3], [0, 1, 4, 2, 5, 3], [3, 0, 4, 2, 5, 1]]
    assert np.array_equal(CM.orders(1, 13, 5)[:2], CM.orders(1, 13, 2))                # one stream: order 0 first, later orders do not move it


def test_every_order_is_a_permutation():
    for seed, S, P in ((1, 1, 3), (2, 2, 50), (3, 13, 20), (2**64 - 1, 257, 4)):
        o = CM.orders(seed, S, P)
        assert o.shape == (P, S) and (np.sort(o, axis=1) == np.arange(S)).all()
    assert len({tuple(r) for r in CM.orders(2, 2, 50).tolist()}) == 2
    assert len({tuple(r) for r in CM.orders(3, 13, 20).tolist()}) == 20


def test_rejection_has_no_modulo_bias():
    """below(n) throws away the draws at or above the largest multiple of n: with n = 2^63 + 1 that is nearly every second draw"""
    n = (1 << 63) + 1
    g, h = CM.SplitMix64(9), CM.SplitMix64(9)
    for _ in range(50):
        x = h.next()
        while x >= n:
            x = h.next()
        assert g.below(n) == x


def test_host_generator_equals_the_model():
    import skx_engine as E
    for seed, S, P in ((1, 13, 2), (7, 6, 3), (2**64 - 1, 100, 5), (0, 1, 3), (5, 2, 40), (1234567, 3, 1)):
        assert np.array_equal(E.curve_orders(seed, S, P), CM.orders(seed, S, P)), (seed, S, P)


# ---- the texts ----
def test_mean_rounds_half_up_at_x0005():
    assert CM.mean_text(1, 2000) == "0.001"             # 0.0005 -> 0.001
    assert CM.mean_text(3, 2000) == "0.002"             # 0.0015 -> 0.002
    assert CM.mean_text(20001, 2000) == "10.001"        # 10.0005
    assert CM.mean_text(1, 2001) == "0.000"             # just below 0.0005
    assert CM.mean_text(7, 3) == "2.333" and CM.mean_text(8, 3) == "2.667" and CM.mean_text(5, 1) == "5.000"
    assert CM.mean_text(3 * (2**63), 3) == f"{2**63}.000"             # integers throughout: no double could hold this


def test_texts_by_hand_and_host_writer():
    counts = CM.curve(HAND, [(0, 1, 2, 3), (3, 2, 1, 0)], 0.5)
    head = "t\t" + "\t".join(f"{c}_{w}" for c in ("pan", "core", "variant", "core_variant") for w in ("min", "median", "max", "mean"))
    want = head + "\n" + "".join(l + "\n" for l in (
        "1\t4\t4\t4\t4.000\t4\t4\t4\t4.000\t0\t0\t0\t0.000\t0\t0\t0\t0.000",
        "2\t5\t5\t5\t5.000\t5\t5\t5\t5.000\t0\t0\t1\t0.500\t0\t0\t1\t0.500",
        "3\t5\t5\t5\t5.000\t4\t4\t4\t4.000\t1\t1\t2\t1.500\t1\t1\t2\t1.500",
        "4\t5\t5\t5\t5.000\t5\t5\t5\t5.000\t2\t2\t2\t2.000\t2\t2\t2\t2.000"))
    assert CM.summary_text(counts) == want
    names = ["a", "b", "c", "d"]
    perm = CM.permutations_text(counts, [(0, 1, 2, 3), (3, 2, 1, 0)], names)
    assert perm.splitlines()[0] == "permutation\tt\tsample\tpan\tcore\tvariant\tcore_variant\tnew"
    assert perm.splitlines()[1:3] == ["0\t1\ta\t4\t4\t0\t0\t4", "0\t2\tb\t5\t5\t0\t0\t1"]
    assert perm.splitlines()[5] == "1\t1\td\t4\t4\t0\t0\t4" and perm.count("\n") == 9
    t = CM.texts(HAND, names, min_freq=0.5, order_names=["d", "c", "b", "a"])
    assert t[".curve.permutations.tsv"].splitlines()[1:] == [l.replace("1\t", "0\t", 1) for l in perm.splitlines()[5:]]
    assert sorted(CM.texts(HAND, names, permutations=3)) == [".curve.tsv"]
    import skx_engine as E
    assert E.curve_tsv(counts) == want
    rng = np.random.default_rng(0)
    for P in (1, 2, 7, 2000):
        c = rng.integers(0, 3, size=(P, 3, 4)).astype(np.uint64)
        c[0, 0, 0] = 1 if P == 2000 else c[0, 0, 0]
        assert E.curve_tsv(c) == CM.summary_text(c), P
