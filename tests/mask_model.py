"""Model of skx_array_mask_regions / skh_mask (`ska mask`): regions of a reference taken out of an array, per sample or for every sample.
numpy only, built on map_model and density_model, on an exported array (keys, variants [U, S], counts [U]).

Definition (restated in include/skx.h).
Sites.  Reference, windows and sites are `ska density`'s (density_model.sites): `ska map`'s windows; a window is a site when its split k-mer
    is a row and occurs exactly once among the reference's windows.  Repeated windows are never sites, so a row is the row of at most one site.
    The split k-mer is the canonical one (with rc, the smaller of the window's and its reverse complement's): that is how the row is found.
    is_rc plays no other part: a cell is only ever made missing.
Intervals.  (sample or ALL, chromosome index, start, end), 0-based and inclusive, in positions of a window's middle base.  Per (sample,
    chromosome), and per chromosome for ALL, intervals that overlap or touch (start <= the other's end + 1) are merged first: the result does
    not depend on how the caller cut them.
Step 1.  Every row whose site lies in an ALL interval is removed (rows_all_samples).
Step 2.  For each remaining row whose site lies in an interval of sample s (sites_in_regions[s] counts it, present or not): if the cell
    (row, s) is present -- neither '-' nor the 0 byte -- it becomes '-', the row's count drops by one (never below 0) and cells_masked[s]
    counts it.
Step 3.  A row that lost a cell in step 2 and has no present cell left is removed (rows_emptied): delete_samples' update_counts(false) rule,
    applied to the rows the call touched.  Keys, variants and counts are compacted in the array's row order.  A row that is no site, or whose
    site lies in no interval, keeps every cell and its count -- also one that held no present cell before.
Whole call.  sites, rows_in, rows_all_samples, rows_emptied, rows_out, n_intervals_merged.  Everything is an integer.

Files.  A regions file is `ska density`'s OUT.density.regions.tsv or any tab-separated file of that shape: the first line that is neither blank
nor a comment is the header and is skipped; then sample, chromosome, start, end (1-based, inclusive), further columns ignored.  A BED file has
chromosome, start (0-based), end (exclusive), no header; its intervals are ALL intervals.  Both take CRLF, blank lines and lines that start
with '#'; both refuse, naming the line number from 1: a line with too few fields, an unknown sample or chromosome, a start or an end that is
no number, start < 1 (BED: nothing, a start is unsigned), end < start (BED: end <= start), an end past its chromosome.
PREFIX.mask.summary.tsv: header "sample\tintervals\tinterval_bases\tsites_in_regions\tcells_masked", a line per sample (intervals and their bases after
merging), then the lines "all_samples_intervals", "all_samples_bases", "sites", "rows_in", "rows_all_samples", "rows_emptied", "rows_out", each
with its value behind a tab.

`mutant=` switches on one deliberate mistake (MUTANTS); tests/test_mask_model.py shows by running them that each is caught."""
import numpy as np

import density_model as DM
import map_model as MM

MUTANTS = (
    "bed_end_inclusive",     # a BED line's exclusive end is read as inclusive
    "repeats_masked",        # windows whose split k-mer occurs again in the reference are sites too
    "empty_rows_kept",       # step 3 is left out
    "counts_not_lowered",    # a masked cell leaves the row's count as it was
    "double_decrement",      # intervals are not merged: a cell two of them cover lowers the count twice
    "row_of_forward_strand", # the row is looked up by the window's own split k-mer, not the canonical one
)

ALL = 0xFFFFFFFF
GAP = ord("-")
SAMPLE_DT = np.dtype([("sites_in_regions", "<u8"), ("cells_masked", "<u8")])
INFO_DT = np.dtype([(f, "<u8") for f in ("sites", "rows_in", "rows_all_samples", "rows_emptied", "rows_out", "n_intervals_merged")])
INTERVAL_DT = np.dtype([(f, "<u4") for f in ("sample", "chrom", "start", "end")])


def merge_intervals(intervals):
    """[(sample | ALL, chrom, start, end)] -> the merged ones, ascending by (sample, chrom, start); ALL is the highest sample"""
    out = []
    for s, c, a, b in sorted((int(s), int(c), int(a), int(b)) for s, c, a, b in intervals):
        assert a <= b
        if out and out[-1][0] == s and out[-1][1] == c and a <= out[-1][3] + 1:
            out[-1][3] = max(out[-1][3], b)
        else:
            out.append([s, c, a, b])
    return [tuple(x) for x in out]


def _sites(keys, k, rc, ref, mutant):
    """[(chrom, pos, row)] of the sites"""
    if mutant == "row_of_forward_strand":
        row_of = {key: r for r, key in enumerate(MM.key_ints(keys))}
        fwd = [MM.chrom_windows(bytes(s), k, False) for _, s in ref]
        can = [MM.chrom_windows(bytes(s), k, rc) for _, s in ref]
        count = {}
        for ws in can:
            for _, split, _ in ws:
                count[split] = count.get(split, 0) + 1
        return [(c, f[0], row_of[f[1]]) for c in range(len(ref)) for f, w in zip(fwd[c], can[c]) if count[w[1]] == 1 and f[1] in row_of]
    return [(c, pos, row) for c, pos, row, _, _ in DM.sites(keys, k, rc, ref, "repeats_kept" if mutant == "repeats_masked" else None)[2]]


def mask(keys, var, counts, k, rc, ref, intervals, mutant=None):
    """-> dict: keys, var, counts (the masked array), samples (SAMPLE_DT [S]), info (INFO_DT record), kept (bool [U])"""
    assert mutant is None or mutant in MUTANTS, mutant
    var = np.array(var, np.uint8, copy=True)
    counts = np.array(counts, np.int64, copy=True)
    U, S = var.shape
    lens = [len(s) for _, s in ref]
    for s, c, a, b in intervals:
        assert (s == ALL or 0 <= s < S) and 0 <= c < len(ref) and 0 <= a <= b < lens[c], (s, c, a, b)
    merged = merge_intervals(intervals)
    work = sorted((int(s), int(c), int(a), int(b)) for s, c, a, b in intervals) if mutant == "double_decrement" else merged
    st = _sites(keys, k, rc, ref, mutant)
    keep = np.ones(U, bool)
    samples = np.zeros(S, SAMPLE_DT)
    for s, c, a, b in work:                                      # step 1
        if s == ALL:
            for sc, pos, row in st:
                if sc == c and a <= pos <= b:
                    keep[row] = False
    rows_all = int((~keep).sum())
    touched = np.zeros(U, bool)
    masked_here = set()

    def lower(row):
        if mutant != "counts_not_lowered":
            counts[row] = max(counts[row] - 1, 0)
    for s, c, a, b in work:                                      # step 2
        if s == ALL:
            continue
        for sc, pos, row in st:
            if sc == c and a <= pos <= b and keep[row]:
                samples["sites_in_regions"][s] += 1
                if var[row, s] not in (0, GAP):
                    samples["cells_masked"][s] += 1
                    var[row, s] = GAP
                    touched[row] = True
                    masked_here.add((row, s))
                    lower(row)
                elif mutant == "double_decrement" and (row, s) in masked_here:
                    lower(row)
    present = ((var != 0) & (var != GAP)).sum(1)
    emptied = touched & keep & (present == 0)
    if mutant != "empty_rows_kept":                              # step 3
        keep &= ~emptied
    info = np.zeros(1, INFO_DT)[0]
    info["sites"], info["rows_in"], info["rows_all_samples"] = len(st), U, rows_all
    info["rows_emptied"], info["rows_out"], info["n_intervals_merged"] = int(emptied.sum()), int(keep.sum()), len(merged)
    return {"keys": np.asarray(keys)[keep], "var": var[keep], "counts": counts[keep].astype(np.uint64), "samples": samples, "info": info, "kept": keep}


def mask_loops(keys, var, counts, k, rc, ref, intervals):
    """the same in plain loops over positions, without merging: a set of (sample, chromosome, position) and a set of (chromosome, position)"""
    own, everybody = set(), set()
    for s, c, a, b in intervals:
        for x in range(a, b + 1):
            (everybody if s == ALL else own).add((c, x) if s == ALL else (s, c, x))
    ints = MM.key_ints(keys)
    seen = {}
    for c, (_, seq) in enumerate(ref):
        for pos, split, _ in MM.chrom_windows(bytes(seq), k, rc):
            seen.setdefault(split, []).append((c, pos))
    out_keys, out_var, out_counts = [], [], []
    for r in range(len(var)):
        at = seen.get(ints[r], [])
        cells, count = [int(x) for x in var[r]], int(counts[r])
        if len(at) == 1:
            c, pos = at[0]
            if (c, pos) in everybody:
                continue
            lost = 0
            for s in range(len(cells)):
                if (s, c, pos) in own and cells[s] not in (0, GAP):
                    cells[s] = GAP
                    lost += 1
            count = max(count - lost, 0)
            if lost and all(x in (0, GAP) for x in cells):
                continue
        out_keys.append(r), out_var.append(cells), out_counts.append(count)
    S = var.shape[1]
    return np.asarray(keys)[out_keys], np.array(out_var, np.uint8).reshape(len(out_var), S), np.array(out_counts, np.uint64)


# ---- files
class BadLine(ValueError):
    def __init__(self, line, what):
        super().__init__(f"line {line}: {what}")
        self.line, self.what = line, what


def _number(field):
    """an unsigned decimal number that fits 32 bits, or None"""
    if not field or not all(48 <= ch <= 57 for ch in field) or len(field) > 10 or int(field) > 0xFFFFFFFF:
        return None
    return int(field)


def _lines(text):
    for no, line in enumerate(text.split(b"\n"), 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line.strip(b" \t") or line.startswith(b"#"):
            continue
        yield no, line.split(b"\t")


def read_regions(text, names, chrom_ids, chrom_lens):
    """a regions file -> [(sample, chrom, start, end)] 0-based inclusive, in the file's order"""
    out, header = [], True
    for no, f in _lines(text):
        if header:
            header = False
            continue
        if len(f) < 4:
            raise BadLine(no, "fewer than four fields")
        name, chrom = f[0].decode(errors="replace"), f[1].decode(errors="replace")
        if name not in names:
            raise BadLine(no, f"unknown sample {name}")
        if chrom not in chrom_ids:
            raise BadLine(no, f"unknown chromosome {chrom}")
        a, b = _number(f[2]), _number(f[3])
        if a is None or b is None:
            raise BadLine(no, "start or end is no number")
        c = chrom_ids.index(chrom)
        if a < 1:
            raise BadLine(no, "start below 1")
        if b < a:
            raise BadLine(no, "end before start")
        if b > int(chrom_lens[c]):
            raise BadLine(no, f"end past chromosome {chrom}")
        out.append((names.index(name), c, a - 1, b - 1))
    return out


def read_bed(text, chrom_ids, chrom_lens, mutant=None):
    """a BED file -> [(ALL, chrom, start, end)] 0-based inclusive, in the file's order"""
    out = []
    for no, f in _lines(text):
        if len(f) < 3:
            raise BadLine(no, "fewer than three fields")
        chrom = f[0].decode(errors="replace")
        if chrom not in chrom_ids:
            raise BadLine(no, f"unknown chromosome {chrom}")
        a, b = _number(f[1]), _number(f[2])
        if a is None or b is None:
            raise BadLine(no, "start or end is no number")
        c = chrom_ids.index(chrom)
        if b <= a:
            raise BadLine(no, "end not after start")
        if b > int(chrom_lens[c]):
            raise BadLine(no, f"end past chromosome {chrom}")
        out.append((ALL, c, a, min(b, int(chrom_lens[c]) - 1) if mutant == "bed_end_inclusive" else b - 1))
    return out


def summary_text(res, names, intervals):
    merged = merge_intervals(intervals)
    lines = ["sample\tintervals\tinterval_bases\tsites_in_regions\tcells_masked"]
    for s, n in enumerate(names):
        own = [x for x in merged if x[0] == s]
        lines.append("\t".join([n, str(len(own)), str(sum(b - a + 1 for _, _, a, b in own)), str(int(res["samples"]["sites_in_regions"][s])),
                                str(int(res["samples"]["cells_masked"][s]))]))
    everybody = [x for x in merged if x[0] == ALL]
    lines.append(f"all_samples_intervals\t{len(everybody)}")
    lines.append(f"all_samples_bases\t{sum(b - a + 1 for _, _, a, b in everybody)}")
    for f in ("sites", "rows_in", "rows_all_samples", "rows_emptied", "rows_out"):
        lines.append(f"{f}\t{int(res['info'][f])}")
    return "\n".join(lines) + "\n"
