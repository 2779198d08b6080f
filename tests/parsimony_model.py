"""Model of Fitch parsimony of every swept row on a rooted binary tree, with numpy over rows and a Python loop over joins -- what a device pass
over the matrix would have to give; a Newick reader and writer, the model of skh_newick_joins / skh_parsimony_newick / skh_parsimony_branches
(include/skx_host.h); and the text of the five files a `ska parsimony` command would write.  numpy only.

Definition.
The array holds S samples and U rows in its current order.  code(cell) is the 4-bit set used by skx_array_group_markers (A 1, C 2, T 4, G 8; '-'
and the 0 byte are 0).  A row is swept when distance_filter_flags keeps it for min_freq: the rows skx_array_pair_sites takes
(sites_model.sweep_flags).
The tree is rooted and binary.  Nodes 0 .. S-1 are the samples in array order; join t (0 <= t < S-1) makes node S+t from children (a, b), both
< S+t; every node below the root 2S-2 is a child exactly once.  This is the node numbering of skx_nj_join.
Per swept row:
  Leaf set.   set[s] = code ? code : 15.  A missing cell allows everything.  An ambiguous cell allows its bases.
  Up-pass, joins ascending.   I = set[a] & set[b];  set[S+t] = I ? I : set[a] | set[b];  score += (I == 0).
  Down-pass, joins descending, child a before b.   state[root] = lowest set bit of set[root];
      state[c] = (state[p] & set[c]) ? state[p] : lowest set bit of set[c].
      A change on the branch above c is state[c] != state[p], recorded as (row, c, from, to) with the bases as ASCII.
  Bases.   bases is the OR of the row's unambiguous codes;  min_score = max(popcount(bases) - 1, 0);  excess = score - min_score, which is
      always >= 0.  A row with excess > 0 is homoplasic.
Derived totals: branch_changes[c] = the changes above c summed over swept rows, for c < 2S-2; info = rows swept, rows with score > 0,
homoplasic rows, the sum of score, the sum of min_score.

A worked example, by hand.  Four samples, the tree ((s0,s1),(s2,s3)): joins (0, 1) -> node 4, (2, 3) -> node 5, (4, 5) -> node 6 = root.

    row 0   A  A  C  C     sets 1 1 2 2.  Node 4 = {A}, node 5 = {C}, root: empty meet, {A, C}, score 1.  Down: root A (lowest bit), node 4 A,
                           node 5 C: one change, above node 5, A -> C.  bases {A, C}: minimum 1, excess 0.
    row 1   A  C  A  C     node 4 = {A, C} (score 1), node 5 = {A, C} (score 2), root = {A, C}.  Down, joins descending: root A; node 4 A, node 5 A;
                           s2 A, s3 C (change above 3, A -> C); s0 A, s1 C (change above 1, A -> C).  Score 2, minimum 1: homoplasic.
    row 2   A  -  -  G     sets 1 15 15 8.  Node 4 = {A}, node 5 = {G}, root {A, G}, score 1.  Down: root A, node 5 G (change above 5, A -> G).
                           Taking '-' as a fifth state would score 2 (missing_as_state).
    row 3   R  A  G  G     sets 9 1 8 8.  Node 4 = {A} (R allows A), node 5 = {G}, root {A, G}, score 1, one change above 5.  bases {A, G}: minimum
                           1.  Taking R as missing gives the same score here; row 4 tells the two apart.
    row 4   R  C  C  C     sets 9 2 2 2.  Node 4: empty meet, {A, C, G}, score 1; node 5 = {C}; root = {C}.  Down: root C, node 4 C, s0: C is not in
                           {A, G}, so A (lowest bit): change above 0, C -> A.  Score 1, bases {C}: minimum 0: homoplasic.  Taking R as missing
                           would score 0 (ambiguous_as_missing).
"""
import numpy as np

from subset_model import CODE

INFO_FIELDS = ("rows_swept", "rows_variable", "rows_homoplasic", "score", "min_score")
SITE_DT = np.dtype([("row", "<u8"), ("score", "<u4"), ("bases", "u1"), ("reserved", "u1", (3,))])                      # skx_parsimony_site
CHANGE_DT = np.dtype([("row", "<u8"), ("node", "<u4"), ("from", "u1"), ("to", "u1"), ("reserved", "u1", (2,))])         # skx_parsimony_change
JOIN_DT = np.dtype([("a", "<u4"), ("b", "<u4")])                                                                         # skx_tree_join
IUPAC = "-ACMTWYHGRSVKDBN"
_POP = np.array([bin(x).count("1") for x in range(16)], np.int64)
_ONE = np.isin(np.arange(16), (1, 2, 4, 8))
_LETTER = np.zeros(16, np.uint8)
for _c, _l in ((1, "A"), (2, "C"), (4, "T"), (8, "G")):
    _LETTER[_c] = ord(_l)

WORKED_VAR = np.array([list(b"AACC"), list(b"ACAC"), list(b"A--G"), list(b"RAGG"), list(b"RCCC")], np.uint8)
WORKED_JOINS = [(0, 1), (2, 3), (4, 5)]


def _lowbit(x):
    return x & (~x + 1)


def check_joins(joins, S):
    joins = [(int(a), int(b)) for a, b in joins]
    assert len(joins) == S - 1 and S >= 2
    seen = set()
    for t, (a, b) in enumerate(joins):
        for c in (a, b):
            assert 0 <= c < S + t and c not in seen, (t, c)
            seen.add(c)
    return joins


def fitch(var, keep, joins, missing_as_state=False, ambiguous_as_missing=False):
    """var: [U, S] bytes; keep[U]: the swept rows; joins: S-1 pairs -> dict with score[U], min_score[U], bases[U] (0 on rows not swept),
    branch_changes[2S-2], info, sites (SITE_DT), changes (CHANGE_DT, row ascending then the walk).  The two flags are the wrong variants the
    model's test holds up against this one: a missing cell as a fifth state, an ambiguous leaf as a missing one."""
    var = np.asarray(var, np.uint8)
    U, S = var.shape
    joins = check_joins(joins, S)
    keep = np.asarray(keep, bool)
    code = CODE[var].astype(np.int64)
    assert not (code == 255).any(), "a byte outside the alphabet"
    leaf = code.copy()
    if ambiguous_as_missing:
        leaf[~_ONE[code]] = 0
    leaf = np.where(leaf == 0, 16 if missing_as_state else 15, leaf)
    sets = np.zeros((2 * S - 1, U), np.int64)
    sets[:S] = leaf.T
    score = np.zeros(U, np.int64)
    for t, (a, b) in enumerate(joins):
        meet = sets[a] & sets[b]
        sets[S + t] = np.where(meet != 0, meet, sets[a] | sets[b])
        score += meet == 0
    state = np.zeros((2 * S - 1, U), np.int64)
    state[2 * S - 2] = _lowbit(sets[2 * S - 2])
    steps = []                                                       # (rows, node, from, to) in the order of the walk
    branch = np.zeros(2 * S - 2, np.int64)
    for t in range(S - 2, -1, -1):
        p = S + t
        for c in joins[t]:
            state[c] = np.where((state[p] & sets[c]) != 0, state[p], _lowbit(sets[c]))
            rows = np.flatnonzero(keep & (state[c] != state[p]))
            branch[c] = len(rows)
            steps.append((rows, c, state[p][rows], state[c][rows]))
    one = np.where(_ONE[code], code, 0)
    bases = np.bitwise_or.reduce(one, axis=1) if S else np.zeros(U, np.int64)
    min_score = np.maximum(_POP[bases] - 1, 0)
    score, min_score, bases = score * keep, min_score * keep, bases * keep
    n = sum(len(s[0]) for s in steps)
    ch = np.zeros(n, CHANGE_DT)
    order = np.zeros(n, np.int64)
    at = 0
    for i, (rows, c, f, to) in enumerate(steps):
        e = at + len(rows)
        ch["row"][at:e], ch["node"][at:e], order[at:e] = rows, c, i
        if not missing_as_state:
            ch["from"][at:e], ch["to"][at:e] = _LETTER[f], _LETTER[to]
        at = e
    ch = ch[np.lexsort((order, ch["row"]))]
    homo = np.flatnonzero(keep & (score > min_score))
    sites = np.zeros(len(homo), SITE_DT)
    sites["row"], sites["score"], sites["bases"] = homo, score[homo], bases[homo]
    info = dict(rows_swept=int(keep.sum()), rows_variable=int((keep & (score > 0)).sum()), rows_homoplasic=len(homo), score=int(score.sum()),
                min_score=int(min_score.sum()))
    return dict(score=score, min_score=min_score, bases=bases, branch_changes=branch, info=info, sites=sites, changes=ch)


def brute_force_score(codes, joins):
    """the fewest changes over every assignment of one base to every node, for one row (codes[S], 0 = missing): S <= 5"""
    import itertools
    S = len(codes)
    joins = check_joins(joins, S)
    leaves = [[b for b in (1, 2, 4, 8) if (c or 15) & b] for c in codes]
    best = None
    for lv in itertools.product(*leaves):
        for inner in itertools.product((1, 2, 4, 8), repeat=S - 1):
            st = list(lv) + list(inner)
            n = sum((st[a] != st[S + t]) + (st[b] != st[S + t]) for t, (a, b) in enumerate(joins))
            best = n if best is None else min(best, n)
    return best


# ---- trees ----
def caterpillar(S):
    """((((0,1),2),3),...): depth S-1"""
    return [(0, 1)] + [(S + t - 1, t + 1) for t in range(1, S - 1)]


def balanced(S):
    level, joins = list(range(S)), []
    while len(level) > 1:
        nxt = []
        for i in range(0, len(level) - 1, 2):
            joins.append((level[i], level[i + 1]))
            nxt.append(S + len(joins) - 1)
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return joins


def random_tree(S, rng):
    """two of the nodes left, drawn evenly, until one is left"""
    live, joins = list(range(S)), []
    while len(live) > 1:
        i = int(rng.integers(len(live)))
        a, live[i] = live[i], live[-1]
        live.pop()
        j = int(rng.integers(len(live)))
        b, live[j] = live[j], S + len(joins)
        joins.append((a, b))
    return joins


def rerooted(joins, S):
    """the same unrooted tree rooted on every one of its edges -> a list of join tables"""
    joins = check_joins(joins, S)
    root = 2 * S - 2
    adj = {v: [] for v in range(root)}
    for t, (a, b) in enumerate(joins):
        p = S + t
        if p == root:
            adj[a].append(b), adj[b].append(a)                       # the root's two branches are one edge
        else:
            adj[p] += [a, b]
            adj[a].append(p), adj[b].append(p)
    out = []
    for x, y in sorted({(min(u, v), max(u, v)) for u in adj for v in adj[u]}):
        new, ident = [], {}

        def build(v, parent):
            stack, post = [(v, parent)], []
            while stack:
                n, p = stack.pop()
                post.append((n, p))
                stack += [(k, n) for k in adj[n] if k != p]
            for n, p in reversed(post):
                kids = [ident[(k, n)] for k in adj[n] if k != p]
                if not kids:
                    ident[(n, p)] = n
                else:
                    new.append(tuple(kids))
                    ident[(n, p)] = S + len(new) - 1
            return ident[(v, parent)]
        l, r = build(x, y), build(y, x)
        new.append((l, r))
        out.append(check_joins(new, S))
    return out


# ---- Newick ----
_SPECIAL = "()[]':;, \t\n\r\v\f"


def newick_name(name):
    if not any(c in _SPECIAL for c in name):
        return name
    return "'" + name.replace("'", "''") + "'"


def newick_joins(text, names):
    """Newick text -> (joins, root_three).  Inner nodes are numbered as they close, so join t is the t-th ')' of the text; a root with three
    children (a, b, c) becomes R = (a, Y), Y = (b, c) and root_three is True.  Quoted labels with '' inside, [comments], branch lengths and inner
    labels (read and dropped), white space.  ValueError("newick: ...") for what skh_newick_joins refuses."""
    S = len(names)
    index = {}
    for i, n in enumerate(names):
        index.setdefault(n, i)
    seen, joins, stack = set(), [], []
    pos, n = 0, len(text)
    root, root_three, after = None, False, False                    # after: a node has just closed, so ',' ')' or ';' comes next

    def bad(msg, at=None):
        return ValueError(f"newick: position {pos if at is None else at}: {msg}")

    def skip():
        nonlocal pos
        while pos < n:
            if text[pos] in " \t\n\r\v\f":
                pos += 1
            elif text[pos] == "[":
                e = text.find("]", pos)
                if e < 0:
                    raise bad("a comment without its end")
                pos = e + 1
            else:
                break

    def label():
        nonlocal pos
        skip()
        if pos < n and text[pos] == "'":
            at, out = pos, []
            pos += 1
            while True:
                if pos >= n:
                    raise bad("a quoted label without its end", at)
                if text[pos] == "'":
                    if pos + 1 < n and text[pos + 1] == "'":
                        out.append("'")
                        pos += 2
                        continue
                    pos += 1
                    return "".join(out), True
                out.append(text[pos])
                pos += 1
        s = pos
        while pos < n and text[pos] not in _SPECIAL:
            pos += 1
        return text[s:pos], False

    def length():
        nonlocal pos
        skip()
        if pos < n and text[pos] == ":":
            pos += 1
            skip()
            while pos < n and text[pos] not in _SPECIAL:
                pos += 1

    def closed(node):
        nonlocal root
        nonlocal after
        length()
        after = True
        if stack:
            stack[-1].append(node)
        else:
            root = node

    while True:
        skip()
        if pos >= n:
            raise bad("the text ends inside the tree")
        ch = text[pos]
        if root is not None:
            if ch != ";":
                raise bad("text after the tree")
            pos += 1
            skip()
            if pos < n:
                raise bad("text after the tree")
            break
        if after and ch not in ",);":
            raise bad(f"unexpected character '{ch}'")
        if ch == "(":
            stack.append([])
            pos += 1
        elif ch == ",":
            if not after:
                raise bad("a ',' without a node before it")
            after = False
            pos += 1
            skip()
            if pos < n and text[pos] in ",)":
                raise bad("a leaf without a name")
        elif ch == ")":
            at = pos
            if not stack:
                raise bad("a ')' without its '('")
            kids = stack.pop()
            pos += 1
            if len(kids) == 1:
                raise bad("a node with one child", at)
            if len(kids) == 0:
                raise bad("a leaf without a name", at)
            if len(kids) == 3 and not stack:
                joins.append((kids[1], kids[2]))
                joins.append((kids[0], S + len(joins) - 1))
                root_three = True
            elif len(kids) != 2:
                raise bad(f"a node with {len(kids)} children (only the root may have three)", at)
            else:
                joins.append((kids[0], kids[1]))
            label()
            closed(S + len(joins) - 1)
        elif ch == ";":
            raise bad("the tree ends inside a node" if stack else "a tree without a node")
        else:
            at = pos
            name, quoted = label()
            if not name and not quoted:
                raise bad(f"unexpected character '{ch}'", at)
            if name not in index:
                raise bad(f"leaf '{name}' is not a sample of the array", at)
            if index[name] in seen:
                raise bad(f"sample '{name}' is named twice", at)
            seen.add(index[name])
            closed(index[name])
    for i, nm in enumerate(names):
        if i not in seen:
            raise ValueError(f"newick: sample '{nm}' is missing from the tree")
    if len(joins) != S - 1:
        raise ValueError("newick: the tree does not join all samples")
    return joins, root_three


class Tree:
    """what the writers need of a join table: parents, the hidden node Y of a trifurcating root, leaves below, lowest leaf"""

    def __init__(self, joins, S, root_three=False):
        self.S, self.joins, self.root = S, check_joins(joins, S), 2 * S - 2
        self.hidden = 2 * S - 3 if root_three else None
        assert not root_three or (S >= 3 and self.joins[-1][1] == self.hidden)
        self.parent = [self.root] * (2 * S - 1)
        self.leaves, self.low = [1] * S + [0] * (S - 1), list(range(S)) + [0] * (S - 1)
        for t, (a, b) in enumerate(self.joins):
            self.parent[a] = self.parent[b] = S + t
            self.leaves[S + t], self.low[S + t] = self.leaves[a] + self.leaves[b], min(self.low[a], self.low[b])

    def kids(self, v):
        """the children as the text has them"""
        a, b = self.joins[v - self.S]
        return [a, *self.joins[b - self.S]] if v == self.root and self.hidden is not None else [a, b]

    def shown(self):
        return [c for c in range(self.root) if c != self.hidden]

    def shown_parent(self, c):
        p = self.parent[c]
        return self.root if p == self.hidden else p

    def owner(self, c):
        """the branch a change above c is reported on: the hidden node's go to the root's first child"""
        return self.joins[-1][0] if c == self.hidden else c

    def label(self, names, c):
        return names[c] if c < self.S else "root" if c == self.root else f"n{c - self.S + 1}"

    def lengths(self, branch_changes):
        out = [0] * self.root
        for c in range(self.root):
            out[self.owner(c)] += int(branch_changes[c])
        return out


def parsimony_newick(names, joins, root_three, branch_changes):
    """PREFIX.parsimony.nwk: the input topology, child order and root, integer branch lengths, inner nodes n1... in the order their ')' come"""
    tr = Tree(joins, len(names), root_three)
    ln = tr.lengths(branch_changes)
    out, stack = [], [(tr.root, 0)]
    while stack:
        v, i = stack.pop()
        kids = [] if v < tr.S else tr.kids(v)
        if i == len(kids):
            out.append(newick_name(names[v]) if v < tr.S else ")" + ("" if v == tr.root else tr.label(names, v)))
            if v != tr.root:
                out.append(f":{ln[v]}")
            continue
        out.append("(" if i == 0 else ",")
        stack.append((v, i + 1))
        stack.append((kids[i], 0))
    return "".join(out) + ";\n"


def branches_text(names, joins, root_three, branch_changes):
    tr = Tree(joins, len(names), root_three)
    ln = tr.lengths(branch_changes)
    out = ["Node\tParent\tLeaves\tLowest leaf\tChanges\n"]
    for c in tr.shown():
        out.append(f"{tr.label(names, c)}\t{tr.label(names, tr.shown_parent(c))}\t{tr.leaves[c]}\t{names[tr.low[c]]}\t{ln[c]}\n")
    return "".join(out)


def _arms(key, k):
    half = (k - 1) // 2
    w = (int(key["hi"]) << 64) | int(key["lo"])
    lo = "".join("ACTG"[(w >> (2 * (half - 1 - b))) & 3] for b in range(half))
    w >>= 2 * half
    return "".join("ACTG"[(w >> (2 * (half - 1 - b))) & 3] for b in range(half)), lo


def _key_order(keys, rows):
    return sorted(range(len(rows)), key=lambda i: (int(keys[int(rows[i])]["hi"]), int(keys[int(rows[i])]["lo"])))


def homoplasies_text(keys, k, sites, min_score):
    """keys[r] = the split k-mer of row r; lines in ascending split k-mer"""
    out = ["Upper\tLower\tBases\tScore\tMinimum\n"]
    for i in _key_order(keys, sites["row"]):
        s = sites[i]
        up, lo = _arms(keys[int(s["row"])], k)
        out.append(f"{up}\t{lo}\t{IUPAC[int(s['bases'])]}\t{int(s['score'])}\t{int(min_score[int(s['row'])])}\n")
    return "".join(out)


def summary_text(info):
    ci = "NA" if info["score"] == 0 else f"{info['min_score'] / info['score']:.6f}"
    return (f"Rows swept\t{info['rows_swept']}\nRows variable\t{info['rows_variable']}\nRows homoplasic\t{info['rows_homoplasic']}\n"
            f"Score\t{info['score']}\nMinimum score\t{info['min_score']}\nConsistency index\t{ci}\n")


def changes_text(names, joins, root_three, keys, k, changes):
    """grouped by branch in node order (the hidden node's under the root's first child), ascending split k-mer within a branch"""
    tr = Tree(joins, len(names), root_three)
    out = ["Branch\tUpper\tLower\tFrom\tTo\n"]
    owner = np.array([tr.owner(int(c)) for c in changes["node"]], np.int64)
    for c in tr.shown():
        sel = np.flatnonzero(owner == c)
        for i in _key_order(keys, changes["row"][sel]):
            r = changes[sel[i]]
            up, lo = _arms(keys[int(r["row"])], k)
            out.append(f"{tr.label(names, c)}\t{up}\t{lo}\t{chr(r['from'])}\t{chr(r['to'])}\n")
    return "".join(out)
