"""The definition of `ska distance --mst` in plain Python, over the full table: what the device forest (skx_array_distance_mst) is compared
against.  D and M are S x S arrays of the table's `distance` and `mismatch_prop` values (only the entries i != j are read; the table is
symmetric).  Nothing here is shared with the engine; the candidates are select_model.select's without `closest`.

The order.  The table's lines are ordered by (Distance, i, j), i < j the sample indices in the array's order: the distance, then the line's
place in the table.  The order is strict, so the minimum spanning forest of the candidate graph is unique, and every correct algorithm
(Kruskal here, Prim in the tests, Boruvka band by band in the engine) gives the same set of lines.
The engine orders by (key, i, j), key the exact integer numerator of the distance (over 1 by default, over 36 with --allow-ambiguous).  The
float64 distance is strictly increasing in key, and so is its "%.2f" print: two keys differ by at least 1/36 > 0.01 in distance.  So the
float64 table, the printed table and the integers all order the lines alike and give the same forest (tests/test_mst_model.py checks the
print for the keys 0 .. 10^5 in both modes)."""
from select_model import select, table_arrays


def candidates(D, M, max_snps=None, max_mismatches=None):
    """-> the candidate lines as (distance, i, j), in the order of the definition"""
    return sorted((D[i][j], i, j) for i, j in select(D, M, max_snps=max_snps, max_mismatches=max_mismatches))


def kruskal(S, ordered):
    """the lines of `ordered` (any (d, i, j) list, taken in the order given) that join two trees -> the set of (i, j)"""
    up = list(range(S))

    def find(x):
        while up[x] != x:
            up[x] = up[up[x]]
            x = up[x]
        return x

    kept = set()
    for _, i, j in ordered:
        a, b = find(i), find(j)
        if a != b:
            up[max(a, b)] = min(a, b)
            kept.add((i, j))
    return kept


def mst(D, M, max_snps=None, max_mismatches=None):
    """-> the set of (i, j), i < j, of the lines of the minimum spanning forest of the candidate graph under the order (Distance, i, j)"""
    return kruskal(len(D), candidates(D, M, max_snps, max_mismatches))


def mst_text(text, **criteria):
    """the table's header and the forest's lines, in the table's order"""
    _, D, M, by_pair = table_arrays(text)
    kept = mst(D, M, **criteria)
    return "".join([text.splitlines(keepends=True)[0]] + [by_pair[p] + "\n" for p in sorted(kept)])


def components(S, pairs):
    """-> label[s] = the lowest sample of s's connected component under the lines `pairs`"""
    up = list(range(S))

    def find(x):
        while up[x] != x:
            x = up[x]
        return x

    for i, j in pairs:
        a, b = find(i), find(j)
        if a != b:
            up[max(a, b)] = min(a, b)
    return [find(s) for s in range(S)]


def levels(D, M, edges, levels, names):
    """-> (columns, csv).  columns[n][s] = the cluster of sample s at levels[n]: the connected components of the forest's lines whose Distance
    as printed ("%.2f", read back as a number: the rule of the engine's --clusters) is <= the level, numbered 1, 2, ... in ascending order
    of their lowest sample.  csv: "id,snps_<L>,...,address", every L printed "%g", one line per sample in the array's order, the name in
    double quotes (inner quotes doubled) when it holds a comma, a quote or a line break, `address` the level columns joined by '.'"""
    S = len(D)
    columns = []
    for L in levels:
        label = components(S, [(i, j) for i, j in edges if float("%.2f" % D[i][j]) <= L])
        number = {root: n + 1 for n, root in enumerate(sorted(set(label)))}
        columns.append([number[r] for r in label])

    def quoted(s):
        return '"' + s.replace('"', '""') + '"' if any(c in s for c in ',"\n\r') else s

    csv = ",".join(["id"] + ["snps_%g" % L for L in levels] + ["address"]) + "\n"
    for s in range(S):
        col = [str(c[s]) for c in columns]
        csv += ",".join([quoted(names[s])] + col + [".".join(col)]) + "\n"
    return columns, csv


def boruvka(S, edges):
    """minimum spanning forest of `edges` ((d, i, j), any order) under the order (d, i, j), by rounds: every component takes its smallest
    outgoing edge, all chosen edges are joined -> (the set of (d, i, j) kept, the number of rounds that chose an edge)"""
    comp = list(range(S))
    kept, rounds = set(), 0
    while True:
        best = {}
        for e in edges:
            a, b = comp[e[1]], comp[e[2]]
            if a == b:
                continue
            for c in (a, b):
                if c not in best or e < best[c]:
                    best[c] = e
        if not best:
            return kept, rounds
        rounds += 1
        kept |= set(best.values())
        comp = components(S, [(i, j) for _, i, j in kept])


def mst_streamed(D, M, band_rows, max_snps=None, max_mismatches=None):
    """The form the engine uses: F = {}; for each band of first samples [lo, hi): F = MSF(F + the candidates with lo <= i < hi), each MSF by
    Boruvka rounds.  By the cycle property (the largest line of a cycle is in no minimum spanning forest, so a line dropped once stays
    dropped) it equals mst for every band size.  -> (the set of (i, j), the largest number of rounds a band took)"""
    S = len(D)
    cand = candidates(D, M, max_snps, max_mismatches)
    F, most = set(), 0
    for lo in range(0, S, band_rows):
        F, rounds = boruvka(S, sorted(F) + [e for e in cand if lo <= e[1] < lo + band_rows])
        most = max(most, rounds)
    return {(i, j) for _, i, j in F}, most
