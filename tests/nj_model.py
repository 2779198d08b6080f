"""The yardstick of `ska distance --tree / --clusters`: neighbour joining as include/skx.h defines it, restated in numpy float64, the
Newick writer of include/skx_host.h and a parser for it, the clusters of a distance table by union-find, and the helpers the tests share
(random additive matrices with their generating splits, `splits`, the step-by-step replay of a join list).  No engine code is used here."""
import re

import numpy as np

NJ_DT = np.dtype([("a", "<u4"), ("b", "<u4"), ("len_a", "<f8"), ("len_b", "<f8")])


# ------------------------------------------------------------------------------------------------ neighbour joining
def nj(matrix, recompute=False):
    """Canonical NJ (Saitou-Nei, Studier-Keppler Q) on a symmetric matrix with a zero diagonal -> S - 1 records (NJ_DT).
    Leaves are nodes 0..S-1, join t makes node S + t; ties in Q go to the lowest (min id, max id).  Row sums are kept incrementally
    (recompute=True: summed afresh at every step, the definition taken literally)."""
    D = np.array(matrix, np.float64)
    S = D.shape[0]
    assert D.shape == (S, S) and S >= 2
    out = np.zeros(S - 1, NJ_DT)
    ids = np.arange(S, dtype=np.int64)
    r = D.sum(axis=1)
    n = S
    for t in range(S - 2):
        Dn = D[:n, :n]
        if recompute:
            r[:n] = Dn.sum(axis=1)
        Q = (n - 2) * Dn - (r[:n, None] + r[None, :n])
        Q[np.arange(n), np.arange(n)] = np.inf
        cand = np.argwhere(Q == Q.min())
        lo_id = np.minimum(ids[cand[:, 0]], ids[cand[:, 1]])
        hi_id = np.maximum(ids[cand[:, 0]], ids[cand[:, 1]])
        pick = np.lexsort((hi_id, lo_id))[0]
        x, y = (int(v) for v in cand[pick])
        sa, sb = (x, y) if ids[x] < ids[y] else (y, x)
        dab = D[sa, sb]
        len_a = dab / 2.0 + (r[sa] - r[sb]) / (2.0 * (n - 2))
        out[t] = (ids[sa], ids[sb], len_a, dab - len_a)
        u = ((D[sa, :n] + D[sb, :n]) - dab) / 2.0
        rn = ((r[:n] - D[sa, :n]) - D[sb, :n]) + u
        ru = ((r[sa] + r[sb]) - n * dab) / 2.0
        lo, hi = min(x, y), max(x, y)
        u[lo] = 0.0
        D[lo, :n] = u
        D[:n, lo] = u
        r[:n] = rn
        r[lo] = ru
        ids[lo] = S + t
        L = n - 1
        if hi != L:                                     # the last live slot takes the retired one
            row = D[L, :n].copy()
            D[hi, :n] = row
            D[:n, hi] = row
            D[hi, hi] = 0.0
            r[hi] = r[L]
            ids[hi] = ids[L]
        n -= 1
    sa, sb = (0, 1) if ids[0] < ids[1] else (1, 0)
    out[S - 2] = (ids[sa], ids[sb], D[0, 1], 0.0)
    return out


def replay(matrix, joins):
    """Walk a join list over the matrix in float64 (row sums summed afresh at every step) -> per step (q of the chosen pair, min q,
    len_a and len_b by the formula, n, max |D|): what a test needs to judge joins that may differ from the model's by rounding."""
    D = np.array(matrix, np.float64)
    S = D.shape[0]
    slot = {i: i for i in range(S)}                      # node id -> row
    big = np.zeros((2 * S - 1, 2 * S - 1))
    big[:S, :S] = D
    active = list(range(S))
    steps = []
    for t in range(S - 2):
        a, b = int(joins[t]["a"]), int(joins[t]["b"])
        assert a < b and a in slot and b in slot, (t, a, b)
        n = len(active)
        idx = np.array(active)
        Dn = big[np.ix_(idx, idx)]
        r = Dn.sum(axis=1)
        Q = (n - 2) * Dn - (r[:, None] + r[None, :])
        Q[np.arange(n), np.arange(n)] = np.inf
        ia, ib = active.index(a), active.index(b)
        dab = Dn[ia, ib]
        la = dab / 2.0 + (r[ia] - r[ib]) / (2.0 * (n - 2))
        steps.append((Q[ia, ib], Q.min(), la, dab - la, n, np.abs(Dn).max()))
        u = S + t
        big[u, idx] = (Dn[ia] + Dn[ib] - dab) / 2.0
        big[idx, u] = big[u, idx]
        active = [v for v in active if v not in (a, b)] + [u]
        slot.pop(a), slot.pop(b)
        slot[u] = u
    a, b = int(joins[S - 2]["a"]), int(joins[S - 2]["b"])
    assert sorted(active) == [a, b] and a < b
    steps.append((0.0, 0.0, big[a, b], 0.0, 2, abs(big[a, b])))
    return steps


def splits(joins, n):
    """Every branch of the tree of a join list as {leaf set not containing leaf 0 (frozenset): raw length}; the last record is one branch."""
    below = {i: frozenset([i]) for i in range(n)}
    everyone = frozenset(range(n))
    out = {}

    def put(s, length):
        s = everyone - s if 0 in s else s
        assert s not in out, "a split twice"
        out[s] = length
    for t in range(n - 1):
        a, b = int(joins[t]["a"]), int(joins[t]["b"])
        if t < n - 2:
            put(below[a], float(joins[t]["len_a"]))
            put(below[b], float(joins[t]["len_b"]))
        else:
            put(below[a], float(joins[t]["len_a"]) + float(joins[t]["len_b"]))
        below[n + t] = below[a] | below[b]
    return out


def random_additive(S, rng, lo, hi):
    """The path-length matrix of a random binary tree over S leaves with integer branch lengths in lo..hi, and that tree's branches in the
    form of `splits` (a zero-length branch is listed with length 0)."""
    D = np.zeros((S, S))
    clusters = [(np.array([i]), np.zeros(1)) for i in range(S)]          # (leaves, their depth below the cluster's top)
    everyone = frozenset(range(S))
    truth = {}

    def put(leaves, length):
        s = frozenset(int(v) for v in leaves)
        s = everyone - s if 0 in s else s
        truth[s] = truth.get(s, 0.0) + float(length)
    while len(clusters) > 1:
        i, j = sorted(rng.choice(len(clusters), 2, replace=False))
        (l1, d1), (l2, d2) = clusters[i], clusters[j]
        last = len(clusters) == 2
        b1 = int(rng.integers(lo, hi + 1))
        b2 = 0 if last else int(rng.integers(lo, hi + 1))                # the last join is one branch of the unrooted tree
        D[np.ix_(l1, l2)] = d1[:, None] + (b1 + b2) + d2[None, :]
        D[np.ix_(l2, l1)] = D[np.ix_(l1, l2)].T
        if last:
            put(l1, b1)
        else:
            put(l1, b1)
            put(l2, b2)
        clusters[i] = (np.concatenate([l1, l2]), np.concatenate([d1 + b1, d2 + b2]))
        del clusters[j]
    return D, truth


def tri_to_matrix(tri, n):
    """upper triangle, pairs (i < j) row-major -> the full symmetric matrix"""
    D = np.zeros((n, n))
    iu = np.triu_indices(n, 1)
    D[iu] = tri
    return D + D.T


# ------------------------------------------------------------------------------------------------ Newick
def _quote(name):
    if re.search(r"[()\[\]':;,\s]", name):
        return "'" + name.replace("'", "''") + "'"
    return name


def newick(names, joins):
    """skh_nj_newick restated: negative lengths to 0 with the difference moved to the sibling, midpoint root between the two leaves
    furthest apart (ties: lowest (id, id); distances accumulated outwards from the lower leaf; the root sits on the first edge of the path
    that reaches half the distance), children by lowest leaf id, lengths %.5f."""
    n = len(names)
    N = 2 * n - 2
    adj = [[] for _ in range(N + 1)]

    def link(x, y, length):
        adj[x].append([y, length])
        adj[y].append([x, length])
    for t in range(n - 1):
        a, b, la, lb = int(joins[t]["a"]), int(joins[t]["b"]), float(joins[t]["len_a"]), float(joins[t]["len_b"])
        if la < 0:
            lb += la
            la = 0.0
        if lb < 0:
            la += lb
            lb = 0.0
        la = max(la, 0.0)
        if t < n - 2:
            link(n + t, a, la)
            link(n + t, b, lb)
        else:
            link(a, b, la + lb)

    def sweep(x):
        dist, par = {x: 0.0}, {x: x}
        stack = [x]
        while stack:
            v = stack.pop()
            for to, length in adj[v]:
                if to != par[v]:
                    par[to] = v
                    dist[to] = dist[v] + length
                    stack.append(to)
        return dist, par
    best, bx, by = -1.0, 0, 1
    for x in range(n - 1):
        dist, _ = sweep(x)
        for y in range(x + 1, n):
            if dist[y] > best:
                best, bx, by = dist[y], x, y
    dist, par = sweep(bx)
    path = [by]
    while path[-1] != bx:
        path.append(par[path[-1]])
    path.reverse()
    half = dist[by] / 2
    for i in range(len(path) - 1):
        p, q = path[i], path[i + 1]
        if dist[q] >= half or i + 2 == len(path):
            lp, lq = max(half - dist[p], 0.0), max(dist[q] - half, 0.0)
            break
    root = N
    for e in adj[p]:
        if e[0] == q:
            e[0], e[1] = root, lp
            break
    for e in adj[q]:
        if e[0] == p:
            e[0], e[1] = root, lq
            break
    adj[root] = [[p, lp], [q, lq]]
    order, parent, blen = [root], {root: root}, {}
    for v in order:
        for to, length in adj[v]:
            if to != parent[v]:
                parent[to], blen[to] = v, length
                order.append(to)
    low = {v: (v if v < n else 1 << 60) for v in order}
    kids = {v: [] for v in order}
    for v in reversed(order[1:]):
        low[parent[v]] = min(low[parent[v]], low[v])
    for v in order[1:]:
        kids[parent[v]].append(v)
    text = {}
    for v in reversed(order):
        if kids[v]:
            body = "(" + ",".join(text.pop(c) for c in sorted(kids[v], key=low.get)) + ")"
        else:
            body = _quote(names[v])
        text[v] = body if v == root else f"{body}:{blen[v]:.5f}"
    return text[root] + ";\n"


def parse_newick(text):
    """One line of Newick -> nested (name | None, length | None, [children]); quoted names unquoted."""
    assert text.endswith(";\n") and text.count("\n") == 1, "one line, ';' and a newline at the end"
    s, pos = text[:-2], 0

    def node():
        nonlocal pos
        kids, name = [], None
        if s[pos] == "(":
            pos += 1
            kids.append(node())
            while s[pos] == ",":
                pos += 1
                kids.append(node())
            assert s[pos] == ")"
            pos += 1
        elif s[pos] == "'":
            pos += 1
            name = ""
            while True:
                if s[pos] == "'" and s[pos + 1: pos + 2] == "'":
                    name += "'"
                    pos += 2
                elif s[pos] == "'":
                    pos += 1
                    break
                else:
                    name += s[pos]
                    pos += 1
        else:
            m = re.compile(r"[^()\[\]':;,\s]+").match(s, pos)
            assert m, (pos, s[pos: pos + 20])
            name, pos = m.group(0), m.end()
        length = None
        if pos < len(s) and s[pos] == ":":
            m = re.compile(r"-?\d+\.\d{5}(?![\d.])").match(s, pos + 1)
            assert m, ("a length with five decimals", s[pos: pos + 20])
            length, pos = float(m.group(0)), m.end()
        return (name, length, kids)
    tree = node()
    assert pos == len(s), s[pos:]
    return tree


def newick_splits(text, names):
    """-> ({leaf set without leaf 0 (of indices into names): length}, (deepest leaf below the root's first child, below its second)).  The two
    branches at a two-child root are one branch of the unrooted tree: their lengths are added."""
    index = {nm: i for i, nm in enumerate(names)}
    assert len(index) == len(names)
    tree = parse_newick(text)
    everyone = frozenset(range(len(names)))
    out, seen = {}, []

    def walk(nd, top):
        name, length, kids = nd
        if not kids:
            seen.append(index[name])
            leaves, depth = frozenset([index[name]]), 0.0
        else:
            assert name is None
            parts = [walk(k, False) for k in kids]
            leaves, depth = frozenset().union(*[p[0] for p in parts]), max(p[1] for p in parts)
            assert [min(p[0]) for p in parts] == sorted(min(p[0]) for p in parts), "children by lowest leaf"
        if not top:
            assert length is not None and length >= 0
            s = everyone - leaves if 0 in leaves else leaves
            out[s] = out.get(s, 0.0) + length
            depth += length
        return leaves, depth
    name, length, kids = tree
    assert length is None and len(kids) == 2, "a root with two children and no length"
    parts = [walk(k, False) for k in kids]
    assert sorted(seen) == list(range(len(names))), "every sample once"
    return out, (parts[0][1], parts[1][1])


# ------------------------------------------------------------------------------------------------ clusters
def parse_tsv(text):
    """the table `ska distance` prints -> (names in first-appearance order, [(i, j, snps, mismatches)] in table order)"""
    lines = text.splitlines()
    assert lines[0] == "Sample1\tSample2\tDistance\tMismatches (proportion)\tMatch count\tMismatch count"
    names, rows = [], []
    for ln in lines[1:]:
        f = ln.split("\t")
        for nm in f[:2]:
            if nm not in names:
                names.append(nm)
        rows.append((names.index(f[0]), names.index(f[1]), float(f[2]), float(f[3])))
    return names, rows


def clusters(names, rows, max_snps, max_mismatches):
    """Union-find over the printed values -> (partition as a sorted list of sorted index lists, clusters.csv text, graph.dot text)."""
    up = list(range(len(names)))

    def find(x):
        while up[x] != x:
            x = up[x]
        return x

    def dq(s):
        return '"' + s.replace("\\", "\\\\").replace('"', '\\"') + '"'
    dot = "strict graph {\n" + "".join(f"\t{dq(nm)};\n" for nm in names)
    for i, j, snps, mism in rows:
        if snps <= max_snps and mism <= max_mismatches:
            dot += f"\t{dq(names[i])} -- {dq(names[j])};\n"
            a, b = find(i), find(j)
            if a != b:
                up[max(a, b)] = min(a, b)
    dot += "}\n"
    groups = {}
    for i in range(len(names)):
        groups.setdefault(find(i), []).append(i)
    ordered = sorted(groups.values(), key=lambda g: (-len(g), g[0]))
    csv = "id,Cluster__autocolour\n"
    for k, g in enumerate(ordered):
        for i in g:
            nm = names[i]
            if re.search(r'[,"\n\r]', nm):
                nm = '"' + nm.replace('"', '""') + '"'
            csv += f"{nm},{k + 1}\n"
    return sorted(ordered), csv, dot
