"""Model of skx_array_group_markers / skh_markers (`ska markers`): which split k-mers, and which middle-base alleles, tell one group of samples
from everybody else -- restated per group, straight from a [U, S] matrix, with none of the kernel's tricks; and the three texts the command
writes, built from the lines of `ska nk --full-info`.  numpy only.

Definition (include/skx.h in the same words).
Inputs.  The array holds S samples and U rows.  Cells are bytes; code(cell) is the 4-bit IUPAC set (A 1, C 2, T 4, G 8; '-' and the 0 byte are 0).
A partition assigns every sample to exactly one segment: segments 0..G-1 are the groups of the file, in the order their labels first appear;
samples the file does not list form one further, unnamed segment, which is never reported -- its samples still count as "others".
Per-row quantities for a reported group g (n = its size): in = cells of g with code != 0; out = cells of all other samples with code != 0;
bases_in / bases_out = OR of the codes on each side.
Thresholds, computed in doubles exactly like this: t_in = max(1, (uint64)ceil(n * P)), t_out = (uint64)floor((S - n) * Q).
Kinds.  presence marker of g: in >= t_in and out <= t_out.  allele marker of g: in >= t_in, not a presence marker, and
bases_in & bases_out == 0.  An ambiguous cell stands for all its bases, which is conservative.  A row can be a marker of several groups; it is
a marker of one group at most once."""
import math

import numpy as np

from subset_model import CODE

PRESENCE, ALLELE = 1, 2
KIND_NAMES = {PRESENCE: "presence", ALLELE: "allele"}
IUPAC = "-ACMTWYHGRSVKDBN"                      # the letter of a 4-bit set
# the layout of skx_marker (skx_engine.MARKER_DT)
REC_DT = np.dtype([("row", "<u8"), ("group", "<u4"), ("n_in", "<u4"), ("n_out", "<u4"), ("kind", "u1"), ("bases_in", "u1"), ("bases_out", "u1"),
                   ("reserved", "u1")])


def thresholds(n, S, P, Q):
    return max(1, int(math.ceil(n * P))), int(math.floor((S - n) * Q))


def _or(codes):
    return np.bitwise_or.reduce(codes, axis=1) if codes.shape[1] else np.zeros(len(codes), np.uint8)


def markers(var, segment_of, n_groups, reported=None, P=1.0, Q=0.0, kinds=PRESENCE | ALLELE):
    """var: [U, S] bytes; segment_of[s] in 0..n_groups (n_groups: unlisted); reported[g]: default every group
    -> (records as REC_DT sorted by (group, row), [(presence, allele)] per group)"""
    var = np.asarray(var, np.uint8)
    seg = np.asarray(segment_of)
    U, S = var.shape
    assert len(seg) == S and ((seg >= 0) & (seg <= n_groups)).all()
    code = CODE[var]
    assert not (code == 255).any(), "a byte outside the alphabet"
    recs, counts = [], []
    for g in range(n_groups):
        if reported is not None and not reported[g]:
            counts.append((0, 0))
            continue
        mine = seg == g
        n = int(mine.sum())
        assert n > 0, "a reported group with no samples"
        inside, outside = code[:, mine], code[:, ~mine]
        n_in, n_out = (inside != 0).sum(axis=1), (outside != 0).sum(axis=1)
        b_in, b_out = _or(inside), _or(outside)
        t_in, t_out = thresholds(n, S, P, Q)
        presence = (n_in >= t_in) & (n_out <= t_out)
        allele = (n_in >= t_in) & ~presence & ((b_in & b_out) == 0)
        kind = np.where(presence & bool(kinds & PRESENCE), PRESENCE, np.where(allele & bool(kinds & ALLELE), ALLELE, 0))
        rows = np.flatnonzero(kind)
        r = np.zeros(len(rows), REC_DT)
        r["row"], r["group"], r["n_in"], r["n_out"], r["kind"], r["bases_in"], r["bases_out"] = rows, g, n_in[rows], n_out[rows], kind[rows], b_in[rows], b_out[rows]
        recs.append(r)
        counts.append((int((kind == PRESENCE).sum()), int((kind == ALLELE).sum())))
    return (np.concatenate(recs) if recs else np.zeros(0, REC_DT)), counts


def partition(S, groups):
    """groups: lists of sample indices -> segment_of (unlisted samples: len(groups))"""
    seg = np.full(S, len(groups), np.int32)
    for g, idx in enumerate(groups):
        assert (seg[idx] == len(groups)).all(), "a sample in two groups"
        seg[idx] = g
    return seg


# ---- the texts of `ska markers`, from the lines `ska nk --full-info` prints for the same file ----
def parse_nk(text):
    """`ska nk --full-info` -> (sample names, [upper], [lower], [U, S] matrix) in the order it prints the rows"""
    if isinstance(text, bytes):
        text = text.decode()
    head, _, body = text.partition("\n\n")
    names = None
    for line in head.split("\n"):
        if line.startswith("sample_names=["):
            names = [x[1:-1] for x in line[len("sample_names=["):-1].split(", ")]
    upper, lower, rows = [], [], []
    for line in body.split("\n"):
        if not line:
            continue
        u, l, cells = line.split("\t")
        upper.append(u)
        lower.append(l)
        rows.append([ord(c) for c in cells.split(",")])
    var = np.array(rows, np.uint8).reshape(len(rows), len(names))
    return names, upper, lower, var


def match_names(names, groups):
    """groups: [(label, [sample names])] in file order -> (segment_of, sizes); first match wins, as `ska delete` finds its samples"""
    seg = np.full(len(names), len(groups), np.int32)
    for g, (_, wanted) in enumerate(groups):
        for w in wanted:
            hit = [s for s, nm in enumerate(names) if nm == w and seg[s] == len(groups)]
            assert hit, f"Could not find sample(s): {w}"
            seg[hit[0]] = g
    return seg, [int((seg == g).sum()) for g in range(len(groups))]


def texts(nk_text, groups, P=1.0, Q=0.0, min_group_size=1, kinds=PRESENCE | ALLELE, fasta=False):
    """-> {file suffix: text}: ".markers.tsv", ".markers.summary.tsv" and with fasta ".<label>.markers.fa" of every reported group with a marker"""
    names, upper, lower, var = parse_nk(nk_text)
    S = len(names)
    seg, sizes = match_names(names, groups)
    reported = [n >= min_group_size for n in sizes]
    recs, counts = markers(var, seg, len(groups), reported, P, Q, kinds)
    out = {}
    tsv = "Group\tUpper\tLower\tKind\tIn\tOut\tBases\tOther bases\n"
    summary = "Group\tSamples\tPresence\tAllele\n"
    for g, (label, _) in enumerate(groups):
        if not reported[g]:
            summary += f"{label}\t{sizes[g]}\t-\t-\n"
            continue
        summary += f"{label}\t{sizes[g]}\t{counts[g][0]}\t{counts[g][1]}\n"
        fa = ""
        for i, r in enumerate(recs[recs["group"] == g], 1):           # (ascending row = the order nk prints)
            row, n = int(r["row"]), sizes[g]
            kind, bases = KIND_NAMES[int(r["kind"])], IUPAC[r["bases_in"]]
            tsv += f"{label}\t{upper[row]}\t{lower[row]}\t{kind}\t{r['n_in']}/{n}\t{r['n_out']}/{S - n}\t{bases}\t{IUPAC[r['bases_out']]}\n"
            middle = next(b for b, bit in (("A", 1), ("C", 2), ("G", 8), ("T", 4)) if r["bases_in"] & bit)
            fa += f">{label}_{i} kind={kind} in={r['n_in']}/{n} out={r['n_out']}/{S - n} bases={bases}\n{upper[row]}{middle}{lower[row]}N\n"
        if fasta and fa:
            out[f".{label}.markers.fa"] = fa
    out[".markers.tsv"] = tsv
    out[".markers.summary.tsv"] = summary
    return out
