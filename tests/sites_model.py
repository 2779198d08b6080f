"""Model of skx_array_pair_sites / skh_distance_sites (`ska distance --sites`): which rows make up the Distance of a pair, and which base each of
the two samples carries there -- restated per pair, straight from a [U, S] matrix, with none of the kernel's tricks; and the text of
PREFIX.sites.tsv.  numpy only.

Definition (include/skx.h in the same words).
The array holds S samples and U rows, in its current order.  Cells are bytes; code(cell) is the 4-bit IUPAC set (A 1, C 2, T 4, G 8; '-' and the
0 byte are 0); a cell is unambiguous when popcount(code) == 1.  A row is swept when it passes the two filters of generic_modes::distance for
min_freq: the threshold ceil(S * min_freq) on the row's count of present cells when min_freq * S >= 1, then NoConst (the row's cells, a gap
counting as one more value, are not all the same).

    sites(i, j) = { r swept : M[i][r] and M[j][r] unambiguous and M[i][r] != M[j][r] },  r ascending        (i < j)
"""
import math

import numpy as np

from subset_model import CODE

HEADER = "Sample1\tSample2\tUpper\tLower\tBase1\tBase2\n"
# the layout of skx_pair_site (skx_engine.PAIR_SITE_DT)
REC_DT = np.dtype([("row", "<u8"), ("pair", "<u4"), ("base_i", "u1"), ("base_j", "u1"), ("reserved", "u1", (2,))])
_ONE = np.isin(np.arange(16), (1, 2, 4, 8))


def threshold(S, min_freq):
    """generic_modes.rs:149-159: no frequency filter below one sample"""
    return int(math.ceil(S * min_freq)) if min_freq * S >= 1 else 0


def sweep_flags(var, min_freq, counts=None, use_threshold=True):
    """var: [U, S] bytes -> keep[U]: the rows the distance sweep takes.  counts: the rows' variant_count where the array carries its own (a loaded
    file's); otherwise the cells present.  use_threshold=False is the wrong variant the model's test holds up against this one."""
    var = np.asarray(var, np.uint8)
    U, S = var.shape
    code = CODE[var]
    assert not (code == 255).any(), "a byte outside the alphabet"
    present = (code != 0).sum(axis=1)
    count = present if counts is None else np.asarray(counts).astype(np.int64)
    keep = np.ones(U, bool)
    if use_threshold:
        keep &= count >= threshold(S, min_freq)
    # NoConst with gaps counting (merge_ska_array.rs:289-402): more than one distinct value among the row's cells
    distinct = np.array([len(set(row.tolist()) - {0}) for row in code], np.int64) if U else np.zeros(0, np.int64)
    keep &= (distinct + (present < S)) > 1
    return keep


def no_const_flags(var):
    """the NoConst stage alone"""
    return sweep_flags(var, 0.0, use_threshold=False)


def sites(var, keep, pairs, count_ambiguous=False):
    """var: [U, S] bytes; keep[U]; pairs: (i, j) with i < j, in any order, repeats allowed -> records as REC_DT sorted by (pair, row).
    count_ambiguous=True is the wrong variant the model's test holds up against this one: any two different present cells."""
    var = np.asarray(var, np.uint8)
    keep = np.asarray(keep, bool)
    code = CODE[var]
    out = []
    for p, (i, j) in enumerate(pairs):
        assert 0 <= i < j < var.shape[1]
        a, b = code[:, i], code[:, j]
        ok = ((a != 0) & (b != 0)) if count_ambiguous else (_ONE[a] & _ONE[b])
        rows = np.flatnonzero(keep & ok & (a != b))
        r = np.zeros(len(rows), REC_DT)
        r["row"], r["pair"], r["base_i"], r["base_j"] = rows, p, var[rows, i], var[rows, j]
        out.append(r)
    return np.concatenate(out) if out else np.zeros(0, REC_DT)


def counts_of(recs, n_pairs):
    return np.bincount(recs["pair"].astype(np.int64), minlength=n_pairs)[:n_pairs] if n_pairs else np.zeros(0, np.int64)


def all_pairs(S):
    return [(i, j) for i in range(S) for j in range(i + 1, S)]


def arms(key, k):
    """(upper, lower) of a split k-mer as `ska nk --full-info` spells them: two bits a base, A C T G = 0 1 2 3, the lower arm in the low bits"""
    half = (k - 1) // 2
    w = (int(key["hi"]) << 64) | int(key["lo"])
    lo = "".join("ACTG"[(w >> (2 * (half - 1 - b))) & 3] for b in range(half))
    w >>= 2 * half
    up = "".join("ACTG"[(w >> (2 * (half - 1 - b))) & 3] for b in range(half))
    return up, lo


def sites_text(names, keys, k, pairs, recs):
    """the text of PREFIX.sites.tsv: keys[r] = the split k-mer of row r (KEY_DT), pairs in the order of the table's lines"""
    out = [HEADER]
    for r in recs:
        i, j = pairs[int(r["pair"])]
        up, lo = arms(keys[int(r["row"])], k)
        out.append(f"{names[i]}\t{names[j]}\t{up}\t{lo}\t{chr(r['base_i'])}\t{chr(r['base_j'])}\n")
    return "".join(out)
