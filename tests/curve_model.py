"""Model of skx_array_curve / skh_curve (`ska curve`): how a collection behaves as samples are added one by one.  numpy only.

Definition (restated in include/skx.h).  The array holds S samples and U rows in its current order.  code(cell) is the 4-bit IUPAC set of
skx_array_group_markers (A 1, C 2, T 4, G 8; '-' and the 0 byte are 0); a cell is unambiguous when popcount(code) == 1.  An order is a
permutation o[0..S) of the sample indices.  For t = 1..S the prefix is o[0..t).  For each row, n = cells of the prefix with code != 0 and
B = OR of the codes of its unambiguous cells.  The threshold is computed in doubles exactly so: thr(t) = max(1, (uint64)ceil(t * min_freq)).
Four counts over the rows per (order, t):

    pan           n >= 1                              the rows `ska delete` of everybody outside the prefix leaves
    core          n >= thr(t)                         `--min-freq f --filter no-filter` on the prefix
    variant       popcount(B) >= 2
    core_variant  n >= thr(t) and popcount(B) >= 2    the columns of `ska align --min-freq f --filter no-ambig-or-const --no-gap-only-sites`

core is not monotone in t when f < 1: it is counted at every step.  tests/test_curve_model.py holds this against tests/subset_model.py (the
oracle's delete_samples + filter) and a hand-worked example.

Seeded orders come from one stream (restated in host/ska_curve.cpp, skh_curve_orders).  The generator is splitmix64 with its state starting at
the seed: next() adds 0x9E3779B97F4A7C15 to the state, takes z = state, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) *
0x94D049BB133111EB and returns z ^ z >> 31, all modulo 2^64.  Order 0 is drawn first.  Each order starts as 0..S-1 and is shuffled by
Fisher-Yates from i = S-1 down to 1: j is drawn from [0, i] by rejection -- x = next() until x < 2^64 - (2^64 mod (i + 1)), j = x mod (i + 1),
so there is no modulo bias -- and o[i], o[j] change places.

Texts.  <PREFIX>.curve.tsv: the header line, then one line per t with t and, for each of the four counts, the minimum, the lower median (place
(P - 1) // 2 of the sorted values), the maximum and the mean over the P orders; the mean has three decimals and is rounded half up by integer
arithmetic, (sum * 1000 + P // 2) // P.  <PREFIX>.curve.permutations.tsv: permutation (from 0), t, the sample added at t, the four counts and
new = pan(t) - pan(t - 1), pan(0) = 0."""
import math

import numpy as np

from subset_model import CODE

COUNTS = ("pan", "core", "variant", "core_variant")
_POP4 = np.array([bin(x).count("1") for x in range(16)], np.uint8)
MASK64 = (1 << 64) - 1


def thresholds(S, min_freq, rounding=math.ceil):
    """thr(1..S)"""
    return np.array([max(1, int(rounding(t * float(min_freq)))) for t in range(1, S + 1)], np.int64)


def curve(var, orders, min_freq, rounding=math.ceil, ambiguous_are_bases=False):
    """var: [U, S] bytes; orders: [P, S] (or [S]) -> uint64 [P, S, 4].  The two keyword arguments make the wrong variants the tests must
    catch: math.floor for the threshold, and ambiguous cells counted into B."""
    var = np.asarray(var, np.uint8)
    U, S = var.shape
    orders = np.asarray(orders, np.int64).reshape(-1, S)
    code = CODE[var]
    assert not (code == 255).any(), "a byte outside the alphabet"
    thr = thresholds(S, min_freq, rounding)
    bases = code if ambiguous_are_bases else np.where(_POP4[code] == 1, code, np.uint8(0))
    out = np.zeros((len(orders), S, 4), np.uint64)
    for p, o in enumerate(orders):
        assert sorted(o.tolist()) == list(range(S)), "not a permutation"
        n = np.cumsum(code[:, o] != 0, axis=1, dtype=np.int64)                         # [U, S]: column t - 1 = the prefix of t samples
        B = np.bitwise_or.accumulate(bases[:, o], axis=1) if U else np.zeros((0, S), np.uint8)
        variant = _POP4[B] >= 2
        core = n >= thr[None, :]
        out[p, :, 0] = (n >= 1).sum(axis=0)
        out[p, :, 1] = core.sum(axis=0)
        out[p, :, 2] = variant.sum(axis=0)
        out[p, :, 3] = (core & variant).sum(axis=0)
    return out


def curve_slow(var, order, min_freq):
    """the definition cell by cell, for one order -> [S][4] as lists (the second restatement small inputs are held against)"""
    S = len(order)
    rows = []
    for t in range(1, S + 1):
        thr = max(1, int(math.ceil(t * float(min_freq))))
        c = [0, 0, 0, 0]
        for row in np.asarray(var, np.uint8):
            codes = [int(CODE[row[s]]) for s in order[:t]]
            n = sum(1 for x in codes if x != 0)
            B = 0
            for x in codes:
                if x in (1, 2, 4, 8):
                    B |= x
            v = bin(B).count("1") >= 2
            c[0] += n >= 1
            c[1] += n >= thr
            c[2] += v
            c[3] += n >= thr and v
        rows.append(c)
    return rows


class SplitMix64:
    def __init__(self, seed):
        self.state = int(seed) & MASK64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & MASK64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        return z ^ (z >> 31)

    def below(self, n):
        """from [0, n) by rejection"""
        limit = (1 << 64) - ((1 << 64) % n)
        while True:
            x = self.next()
            if x < limit:
                return x % n


def orders(seed, S, P):
    """-> int32 [P, S]: the P seeded orders of S samples"""
    g = SplitMix64(seed)
    out = np.zeros((P, S), np.int32)
    for p in range(P):
        o = list(range(S))
        for i in range(S - 1, 0, -1):
            j = g.below(i + 1)
            o[i], o[j] = o[j], o[i]
        out[p] = o
    return out


def mean_text(total, P):
    """the mean of P values summing to total: three decimals, rounded half up, integers only"""
    q = (int(total) * 1000 + P // 2) // P
    return f"{q // 1000}.{q % 1000:03d}"


def summary_text(counts):
    """<PREFIX>.curve.tsv from counts [P, S, 4]"""
    counts = np.asarray(counts, np.uint64)
    P, S, _ = counts.shape
    lines = ["t\t" + "\t".join(f"{c}_{w}" for c in COUNTS for w in ("min", "median", "max", "mean"))]
    for t in range(S):
        f = [str(t + 1)]
        for c in range(4):
            v = sorted(int(x) for x in counts[:, t, c])
            f += [str(v[0]), str(v[(P - 1) // 2]), str(v[-1]), mean_text(sum(v), P)]
        lines.append("\t".join(f))
    return "\n".join(lines) + "\n"


def permutations_text(counts, orders_, names):
    """<PREFIX>.curve.permutations.tsv"""
    counts = np.asarray(counts, np.uint64)
    lines = ["permutation\tt\tsample\tpan\tcore\tvariant\tcore_variant\tnew"]
    for p in range(counts.shape[0]):
        before = 0
        for t in range(counts.shape[1]):
            c = [int(x) for x in counts[p, t]]
            lines.append("\t".join([str(p), str(t + 1), names[int(orders_[p][t])]] + [str(x) for x in c] + [str(c[0] - before)]))
            before = c[0]
    return "\n".join(lines) + "\n"


def texts(var, names, min_freq=0.9, permutations=20, seed=1, order_names=None, all_permutations=False):
    """-> {file suffix: text} as `ska curve` writes them; order_names: the lines of --order-file"""
    S = len(names)
    if order_names is not None:
        assert sorted(order_names) == sorted(names)
        o = np.array([[names.index(n) for n in order_names]], np.int32)
    else:
        o = orders(seed, S, permutations)
    counts = curve(var, o, min_freq)
    out = {".curve.tsv": summary_text(counts)}
    if all_permutations or order_names is not None:
        out[".curve.permutations.tsv"] = permutations_text(counts, o, names)
    return out
