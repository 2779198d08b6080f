"""Model of skx_array_screen / skh_screen (`ska screen`): which samples carry which records of a sequence panel, and how well they match.  numpy
only, on an exported array (keys, variants [U, S]).

Definition (restated in include/skx.h).  A panel is a FASTA file of R records.  A record's windows are exactly those `ska map` gives a chromosome
(map_model.chrom_windows): runs of ACGT in either case, N splitting runs, and the end-of-record quirk (a run that starts less than k + 1 letters
before the end of its record gives none); each window has the position of its middle base, its canonical split k-mer and its is_rc.  Every window
counts on its own: a split k-mer that occurs twice counts twice, within a record or across records.  A window hits when its split k-mer is a row of
the array.  For a hit window and sample s the cell is the array's byte for (row, s), passed through RC_IUPAC when is_rc, as `ska map` gathers its
cells (map_model.MapModel.cells); the 0 byte an export may hold for '-' is '-'.  Per (record r, sample s), over r's hit windows:

    found   the cells that are not '-'
    match   the cells equal to the record's own middle base, upper-cased
    ambig   the cells that are present and none of A, C, G, T
    snp     found - match - ambig                                  (derived, not stored)

Per record: length = its bytes of sequence, windows = its windows, rows_hit = its hit windows.  A pair (r, s) passes when windows > 0 and
found >= max(1, ceil(C * windows)) and match >= ceil(I * found), the products in doubles; C is --min-cover (default 0.9), I --min-identity
(default 0).

Texts.  <PREFIX>.screen.tsv: the header, then one line per passing (record, sample) in panel order and then array order: record, length, windows,
sample, found, match, ambig, snp, cover = found / windows and identity = match / found, each the double quotient as %.4f.
<PREFIX>.screen.summary.tsv: one line per record, those without windows included: record, length, windows, rows_hit, samples_passing.
<PREFIX>.screen.matrix.tsv (--matrix): a header line "record" and the sample names, then per record its id and 1 where the pair passes, 0 where not.

`mutant=` switches on one deliberate mistake (MUTANTS); tests/test_screen_model.py shows by running them that each is caught."""
import math

import numpy as np

import map_model as MM

MUTANTS = (
    "no_rc_iupac",        # the cells of windows on the other strand are not passed through RC_IUPAC
    "gap_cells_found",    # '-' cells count as found
    "distinct_kmers",     # a split k-mer that occurs again, in the same record or a later one, is not counted again
    "floor_threshold",    # the two thresholds are rounded down
)

GAP = ord("-")
RECORD_DT = np.dtype([("length", "<u8"), ("windows", "<u8"), ("rows_hit", "<u8")])
_RC = MM._rc_table(None)
_ACGT = np.zeros(256, bool)
for _c in b"ACGT":
    _ACGT[_c] = True


def record_windows(panel, k, rc, mutant=None):
    """per record of panel [(id, bytes)]: its windows [(pos of the middle base, split k-mer, is_rc)]"""
    out, seen = [], set()
    for _, seq in panel:
        ws = MM.chrom_windows(bytes(seq), k, rc)
        if mutant == "distinct_kmers":
            ws = [w for w in ws if not (w[1] in seen or seen.add(w[1]))]
        out.append(ws)
    return out


def screen(keys, var, k, rc, panel, mutant=None):
    """-> (records as RECORD_DT [R], counts uint32 [R, S, 3] = found, match, ambig)"""
    assert mutant is None or mutant in MUTANTS, mutant
    var = np.asarray(var, np.uint8)
    S = var.shape[1]
    row_of = {key: r for r, key in enumerate(MM.key_ints(keys))}
    R = len(panel)
    records = np.zeros(R, RECORD_DT)
    counts = np.zeros((R, S, 3), np.uint32)
    rec, rows, want, strand = [], [], [], []
    for r, ((_, seq), ws) in enumerate(zip(panel, record_windows(panel, k, rc, mutant))):
        hit = 0
        for pos, split, is_rc in ws:
            row = row_of.get(split)
            if row is None:
                continue
            hit += 1
            rec.append(r), rows.append(row), want.append(bytes(seq)[pos] & 0xDF), strand.append(is_rc)
        records[r] = (len(seq), len(ws), hit)
    if not rows:
        return records, counts
    cells = var[np.array(rows, np.int64)]                                   # [hit windows][S]
    cells = np.where(cells == 0, np.uint8(GAP), cells)
    if mutant != "no_rc_iupac":
        cells = np.where(np.array(strand, bool)[:, None], _RC[cells], cells)
    present = cells != GAP
    rec = np.array(rec, np.int64)
    found = np.ones_like(present) if mutant == "gap_cells_found" else present
    np.add.at(counts[:, :, 0], rec, found.astype(np.uint32))
    np.add.at(counts[:, :, 1], rec, (cells == np.array(want, np.uint8)[:, None]).astype(np.uint32))
    np.add.at(counts[:, :, 2], rec, (present & ~_ACGT[cells]).astype(np.uint32))
    return records, counts


def screen_slow(keys, var, k, rc, panel):
    """the definition cell by cell in plain loops -> (records as lists, counts[r][s] = [found, match, ambig])"""
    rc_of = {"A": "T", "B": "V", "C": "G", "D": "H", "G": "C", "H": "D", "K": "M", "M": "K", "N": "N", "R": "Y", "S": "S", "T": "A", "V": "B", "W": "W", "Y": "R"}
    key_list = MM.key_ints(keys)
    S = len(var[0]) if len(var) else 0
    records, counts = [], []
    for _, seq in panel:
        ws = MM.chrom_windows(bytes(seq), k, rc)
        hits = 0
        per = [[0, 0, 0] for _ in range(S)]
        for pos, split, is_rc in ws:
            if split not in key_list:
                continue
            hits += 1
            row = key_list.index(split)
            base = chr(bytes(seq)[pos]).upper()
            for s in range(S):
                b = int(var[row][s])
                cell = "-" if b == 0 else chr(b)
                if is_rc:
                    cell = rc_of.get(cell.upper(), "-")
                if cell != "-":
                    per[s][0] += 1
                    if cell not in "ACGT":
                        per[s][2] += 1
                if cell == base:
                    per[s][1] += 1
        records.append([len(seq), len(ws), hits])
        counts.append(per)
    return records, counts


def passes(records, counts, min_cover=0.9, min_identity=0.0, mutant=None):
    """-> bool [R, S]"""
    rounding = math.floor if mutant == "floor_threshold" else math.ceil
    R, S = counts.shape[:2]
    out = np.zeros((R, S), bool)
    for r in range(R):
        w = int(records["windows"][r])
        if w == 0:
            continue
        need = max(1, int(rounding(float(min_cover) * float(w))))
        for s in range(S):
            f, m = int(counts[r, s, 0]), int(counts[r, s, 1])
            out[r, s] = f >= need and m >= int(rounding(float(min_identity) * float(f)))
    return out


def pairs_text(ids, records, counts, names, ok):
    lines = ["record\tlength\twindows\tsample\tfound\tmatch\tambig\tsnp\tcover\tidentity"]
    for r, s in np.argwhere(ok):
        f, m, a = (int(x) for x in counts[r, s])
        w = int(records["windows"][r])
        lines.append("\t".join([ids[r], str(int(records["length"][r])), str(w), names[s], str(f), str(m), str(a), str(f - m - a),
                                "%.4f" % (f / w), "%.4f" % (m / f)]))
    return "\n".join(lines) + "\n"


def summary_text(ids, records, ok):
    lines = ["record\tlength\twindows\trows_hit\tsamples_passing"]
    for r, i in enumerate(ids):
        lines.append("\t".join([i] + [str(int(records[f][r])) for f in ("length", "windows", "rows_hit")] + [str(int(ok[r].sum()))]))
    return "\n".join(lines) + "\n"


def matrix_text(ids, names, ok):
    lines = ["\t".join(["record"] + list(names))]
    for r, i in enumerate(ids):
        lines.append("\t".join([i] + ["1" if x else "0" for x in ok[r]]))
    return "\n".join(lines) + "\n"


def texts(keys, var, names, k, rc, panel, min_cover=0.9, min_identity=0.0, matrix=False, mutant=None):
    """-> {file suffix: text} as `ska screen` writes them; panel: [(id, bytes)] with the id cut at its first white space"""
    ids = [i for i, _ in panel]
    records, counts = screen(keys, var, k, rc, panel, mutant)
    ok = passes(records, counts, min_cover, min_identity, mutant)
    out = {".screen.tsv": pairs_text(ids, records, counts, list(names), ok), ".screen.summary.tsv": summary_text(ids, records, ok)}
    if matrix:
        out[".screen.matrix.tsv"] = matrix_text(ids, list(names), ok)
    return out
