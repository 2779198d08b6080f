"""The definition of `ska distance --max-snps / --max-mismatches / --closest` in plain Python, over the full table: what the device selection
(skx_array_distance_select) is compared against.  D and M are S x S arrays of the table's `distance` and `mismatch_prop` values (only the
entries i != j are read; the table is symmetric).  Nothing here is shared with the engine."""


def select(D, M, max_snps=None, max_mismatches=None, closest=0):
    """-> the set of (i, j), i < j, of the lines kept.
    A pair is a candidate when it passes every threshold given (distance <= max_snps, mismatch_prop <= max_mismatches).  With closest = K,
    every sample s orders its candidate partners t by (distance(s, t), t); its nearest are the first min(K, how many); a line is kept when
    either of its samples has the other among its nearest."""
    S = len(D)

    def candidate(i, j):
        return (max_snps is None or D[i][j] <= max_snps) and (max_mismatches is None or M[i][j] <= max_mismatches)

    cand = {(i, j) for i in range(S) for j in range(i + 1, S) if candidate(i, j)}
    if not closest:
        return cand
    kept = set()
    for s in range(S):
        partners = sorted((D[s][t], t) for t in range(S) if t != s and (min(s, t), max(s, t)) in cand)
        for _, t in partners[:closest]:
            kept.add((min(s, t), max(s, t)))
    return kept


def table_arrays(text):
    """the text of a `ska distance` table -> (names in the array's order, D, M, {(i, j): line}) with the values as the table prints them"""
    lines = text.splitlines()[1:]
    names = []
    for ln in lines:
        for n in ln.split("\t")[:2]:
            if n not in names:
                names.append(n)
    S = len(names)
    D = [[0.0] * S for _ in range(S)]
    M = [[0.0] * S for _ in range(S)]
    by_pair = {}
    for ln in lines:
        f = ln.split("\t")
        i, j = names.index(f[0]), names.index(f[1])
        assert i < j
        D[i][j] = D[j][i] = float(f[2])
        M[i][j] = M[j][i] = float(f[3])
        by_pair[(i, j)] = ln
    assert len(by_pair) == S * (S - 1) // 2
    return names, D, M, by_pair


def select_text(text, **criteria):
    """the table's header and the lines the criteria keep, in the table's order"""
    _, D, M, by_pair = table_arrays(text)
    kept = select(D, M, **criteria)
    return "".join([text.splitlines(keepends=True)[0]] + [by_pair[p] + "\n" for p in sorted(kept)])
