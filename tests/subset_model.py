"""Model of skx_array_subset_filtered (`ska align --groups / --samples`): MergeSkaArray::delete_samples of everybody outside a group
(merge_ska_array.rs:231-271 with update_counts(false), :139-163) followed by generic_modes::apply_filters (generic_modes.rs:112-131) =
MergeSkaArray::filter (:289-402), restated per row on an exported [U, S] matrix -- plus the inputs, groups and option grid the tests of the
feature share, and the oracle chain (ora.Array.delete_samples + apply_filters + fasta) they are held against.  numpy only."""
import functools
import itertools

import numpy as np

FILTER_NAMES = ("no-filter", "no-const", "no-ambig", "no-ambig-or-const")
# ASCII middle base -> IUPAC set code (bit i = 2-bit base code i: A 1, C 2, T 4, G 8); 0 for '-' (and the 0 byte an export may hold for it)
_CODES = {"-": 0, "A": 1, "C": 2, "M": 3, "T": 4, "W": 5, "Y": 6, "H": 7, "G": 8, "R": 9, "S": 10, "V": 11, "K": 12, "D": 13, "B": 14, "N": 15}
CODE = np.full(256, 255, np.uint8)
CODE[0] = 0
for _b, _c in _CODES.items():
    CODE[ord(_b)] = _c
_ACGT = (1 << 1) | (1 << 2) | (1 << 4) | (1 << 8)
_POP16 = np.array([bin(x).count("1") for x in range(1 << 16)], np.uint8)
# is_ambiguous (bit_encoding.rs:58-61): what --ambig-mask turns into 'N'
MASKED = np.arange(256, dtype=np.uint8)
for _b in range(256):
    if chr(_b) not in "ACGTU-":
        MASKED[_b] = ord("N")


class Opts(tuple):
    """(min_freq, filter_ambig_as_missing, filter_type, mask_ambig, ignore_const_gaps)"""
    min_freq = property(lambda s: s[0])
    filter_ambig_as_missing = property(lambda s: s[1])
    filter_type = property(lambda s: s[2])
    mask_ambig = property(lambda s: s[3])
    ignore_const_gaps = property(lambda s: s[4])

    def ident(self):
        return f"mf{self[0]}-{FILTER_NAMES[self[2]]}" + ("-ambigmissing" if self[1] else "") + ("-mask" if self[3] else "") + ("-nogaponly" if self[4] else "")


ALL_OPTS = [Opts(o) for o in itertools.product((0.0, 0.6, 1.0), (False, True), (0, 1, 2, 3), (False, True), (False, True))]


def option_grid(n=12, seed=20261018):
    """n of the 96 combinations, drawn with a fixed seed; redrawn (next seed) until every filter type, both values of each flag and each
    min_freq are among them.  min_freq = 0 with no-const and nothing else is always the first: the tests' non-vacuity reference."""
    base = Opts((0.0, False, 1, False, False))
    while True:
        rng = np.random.default_rng(seed)
        pick = [base] + [ALL_OPTS[i] for i in rng.permutation(len(ALL_OPTS))[: n - 1] if ALL_OPTS[i] != base]
        if all(len({o[f] for o in pick}) == w for f, w in ((0, 3), (1, 2), (2, 4), (3, 2), (4, 2))):
            return pick
        seed += 1


GRID = option_grid()


def verdicts(var, group, opts):
    """var: [U, S] bytes; group: sample indices in any order.  -> per-row classes and the kept columns.
    class: 0 absent, 1 silent, 2 removed by frequency, 3 removed by type, 4 kept"""
    cols = sorted(int(g) for g in group)
    n = len(cols)
    sub = np.ascontiguousarray(np.asarray(var, np.uint8)[:, cols])
    code = CODE[sub]
    assert not (code == 255).any(), "a byte outside the alphabet"
    present = (code != 0).sum(axis=1)
    unambig = np.isin(code, (1, 2, 4, 8)).sum(axis=1)
    m = np.bitwise_or.reduce(np.where(code != 0, np.uint32(1) << code.astype(np.uint32), np.uint32(0)), axis=1).astype(np.uint32) if n else np.zeros(len(sub), np.uint32)
    threshold = int(np.ceil(n * opts.min_freq))
    count = unambig if opts.filter_ambig_as_missing else present
    has_gap = present < n
    gap = (has_gap & (not opts.ignore_const_gaps)).astype(np.int64)
    ft = opts.filter_type
    if ft == 0:
        type_ok = np.ones(len(sub), bool)
    elif ft == 1:
        type_ok = (_POP16[m] + gap) > 1
    elif ft == 2:
        type_ok = (m & ~np.uint32(_ACGT)) == 0
    else:
        type_ok = (_POP16[m & _ACGT] + gap) > 1
    cls = np.full(len(sub), 4, np.int8)
    cls[~type_ok] = 3
    cls[count < threshold] = 2
    if opts.filter_ambig_as_missing:
        cls[count == 0] = 1
    cls[present == 0] = 0
    kept = sub[cls == 4]
    kept = np.where(kept == 0, np.uint8(ord("-")), kept)
    if opts.mask_ambig:
        kept = MASKED[kept]
    return cls, kept


def model(var, group, opts):
    """-> (sorted kept columns as bytes of the group's samples in ascending index, counts)"""
    cls, kept = verdicts(var, group, opts)
    counts = {"absent": int((cls == 0).sum()), "silent": int((cls == 1).sum()), "removed_freq": int((cls == 2).sum()), "removed_type": int((cls == 3).sum()),
              "kept": int((cls == 4).sum())}
    counts["removed"] = counts["removed_freq"] + counts["removed_type"]
    counts["rows_present"] = len(cls) - counts["absent"]
    return sorted(r.tobytes() for r in kept), counts


def fasta_columns(aln):
    """the columns of a FASTA alignment (one line per sequence) as a sorted list of bytes"""
    seqs = aln.split(b"\n")[1::2]
    if not seqs or not seqs[0]:
        return []
    mat = np.frombuffer(b"".join(seqs), np.uint8).reshape(len(seqs), len(seqs[0]))
    return sorted(c.tobytes() for c in np.ascontiguousarray(mat.T))


def expected_fasta(names, var, group, opts):
    """the alignment in the given row order: what the engine writes when `var` is its own export (the kept rows stay in the array's order)"""
    cls, kept = verdicts(var, group, opts)
    cols = sorted(int(g) for g in group)
    return b"".join(b">" + names[c].encode() + b"\n" + np.ascontiguousarray(kept[:, j]).tobytes() + b"\n" for j, c in enumerate(cols))


# ---- inputs: the smallest shapes at which the kernels can go wrong (more than two 4 096-column compaction blocks, no multiple of 16) ----
def _point(s, p, step=1):
    s[p] = b"ACGT"[(b"ACGT".index(int(s[p])) + step) % 4]


def samples(S, L, k):
    """one random ancestor (seed 1000 S + k); clades of four consecutive samples, each with a founder 25 point mutations (beyond the first
    L/10 bases) from the ancestor; member i carries 2 (i mod 4) further mutations; every third sample is truncated to 0.7 L - 7 i bases; each
    sample's second record is a 400-base window of its clade's founder from L/5 + 50 (i div 4) on with a base changed every 90 -- the
    ambiguous cells, shared by the whole clade.  -> per sample the list of its records (bytes)"""
    rng = np.random.default_rng(1000 * S + k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    anc = rng.choice(acgt, size=L)

    def mutate(s, n):
        for p in rng.integers(L // 10, L, size=n):
            _point(s, p, 1 + int(rng.integers(0, 3)))

    out, founder = [], None
    for i in range(S):
        if i % 4 == 0:
            founder = anc.copy()
            mutate(founder, 25)
        s = founder.copy()
        mutate(s, 2 * (i % 4))
        if i % 3 == 0:
            s = s[: int(0.7 * L) - 7 * i]
        w0 = L // 5 + 50 * (i // 4)
        win = founder[w0:w0 + 400].copy()
        for p in range(60, len(win), 90):
            _point(win, p)
        out.append([s.tobytes()] + ([win.tobytes()] if len(win) else []))
    return out


LARGE = {"S": 13, "L": 9000, "groups": [[4, 5, 6, 7], [9, 11], [0, 3], [12, 1, 8, 2, 10], [6], list(range(1, 13)), list(range(13))]}
TINY = {"S": 6, "L": 60, "groups": [[0, 3], [1, 2, 4], [5]]}
CASES = {"k31": dict(LARGE, k=31), "k9": dict(LARGE, k=9), "k41": dict(LARGE, k=41), "tiny": dict(TINY, k=9)}
LARGE_CASES = ("k31", "k9", "k41")


def names_of(case):
    return [f"s{i:02d}" for i in range(CASES[case]["S"])]


@functools.lru_cache(maxsize=None)
def records(case):
    c = CASES[case]
    return samples(c["S"], c["L"], c["k"])


def _oracle_array(case):
    import ora
    k = CASES[case]["k"]
    dicts = []
    for recs in records(case):
        d = ora.Dict.new(k, True)
        for r in recs:
            d.add_record(r)
        dicts.append(d)
    return ora.Array.from_dicts(dicts, names_of(case))


@functools.lru_cache(maxsize=None)
def oracle_export(case):
    """the oracle's [U, S] matrix of the case (rows in its own order)"""
    return _oracle_array(case).export()[1]


@functools.lru_cache(maxsize=None)
def oracle_chain(case, group, opts):
    """a fresh ora.Array.from_dicts, delete_samples(everybody else), apply_filters, fasta -> (sorted columns, nrows after the delete, removed).
    The group of all samples has nobody to delete (the delete refuses to remove nothing): the filter alone."""
    a = _oracle_array(case)
    names = names_of(case)
    others = [nm for i, nm in enumerate(names) if i not in group]
    if others:
        a.delete_samples(others)
    nrows = a.nrows
    removed = a.apply_filters(opts.min_freq, opts.filter_ambig_as_missing, opts.filter_type, opts.mask_ambig, opts.ignore_const_gaps)
    aln = a.fasta()
    assert [l[1:].decode() for l in aln.split(b"\n")[0::2] if l] == [names[i] for i in sorted(group)]
    return fasta_columns(aln), nrows, removed
