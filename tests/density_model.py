"""Model of skx_array_snp_density / skh_density (`ska density`): dense-SNP regions per sample along a reference.  numpy only, built on map_model,
on an exported array (keys, variants [U, S]).

Definition (restated in include/skx.h).
Reference and windows.  The reference is a FASTA file of C chromosomes.  Its windows are `ska map`'s (map_model.chrom_windows): runs of ACGT in
    either case, N splitting runs, and the end-of-record quirk (a run that starts less than k + 1 letters before the end of its record gives
    none); each window has the position of its middle base, its canonical split k-mer and its is_rc.
Sites.  A window is a site when its split k-mer is a row of the array and that split k-mer occurs exactly once among all windows of the
    reference.  The repeated windows are the ones `ska map --repeat-mask` masks; they are never sites, so every row is the row of at most one site.
Cells.  For site x and sample s the cell is the array's byte for (row, s), passed through RC_IUPAC when is_rc; the 0 byte counts as '-'.
Classes.  With r = the reference's middle base, upper-cased, a cell is missing when it is '-'; ambiguous when it is present and none of A, C,
    G, T; snp when it is one of A, C, G, T and != r; otherwise it matches.  callable = matching + snp, so missing + ambiguous + callable = sites
    for every sample.
Dense SNPs.  Per (sample, chromosome) take the SNP positions p_0 < p_1 < ...; SNP i is dense when some j with j <= i <= j + T - 1 has
    p_{j+T-1} - p_j < W: i is one of T consecutive SNPs that lie inside W consecutive reference positions.  (The sliding-window form,
    dense_sliding below: SNP i is dense when some stretch [a, a + W) of the chromosome holds p_i and at least T SNPs.)
Regions.  A region is a maximal run of consecutive dense SNPs of one (sample, chromosome): sample, chromosome, start = first position, end =
    last position (0-based here), snps = their number.  Regions never span chromosomes.
Bins.  Chromosome c has ceil(len_c / W) bins of W positions; per bin, summed over samples, snps and dense_snps.
Per sample.  sites, callable, ambiguous, missing, snps, dense_snps, regions and region_bases (the sum of end - start + 1).
Whole call.  windows, repeat_windows (windows whose split k-mer occurs more than once) and sites.
Everything is an integer.  1 <= W <= 2^31, 2 <= T <= 65 535; the defaults W = 1000, T = 5 are a convention, not a calibration.

Texts (positions 1-based, inclusive).  <PREFIX>.density.regions.tsv: sample, chromosome, start, end, length, snps, a line per region ascending
by (sample, chromosome, start).  <PREFIX>.density.summary.tsv: a line per sample: the eight counts and snps_outside = snps - dense_snps.
<PREFIX>.density.bins.tsv: chromosome, start, end, snps, dense_snps; a chromosome's last bin ends at its length.  <PREFIX>.density.snps.tsv
(--snps): sample, chromosome, position, ref (upper-cased), alt (on the reference's strand), dense (1 or 0), ascending by (sample, position in the
concatenated reference).  --masked-aln: `ska map`'s alignment (no ambig mask, repeat mask on) with, in each sample's line, every byte of a
region [start, end] that is not '-' overwritten with 'N'.

`mutant=` switches on one deliberate mistake (MUTANTS); tests/test_density_model.py shows by running them that each is caught."""
import numpy as np

import map_model as MM

MUTANTS = (
    "repeats_kept",        # windows whose split k-mer occurs again in the reference are sites too
    "ambig_as_snp",        # an ambiguous cell counts as a SNP
    "window_inclusive",    # p_{j+T-1} - p_j <= W
    "span_chromosomes",    # a sample's SNP positions are taken along the concatenated reference: runs cross chromosome boundaries
    "no_rc_iupac",         # the cells of windows on the other strand are not passed through RC_IUPAC
    "ref_case_sensitive",  # the reference's middle base is compared as it is written
)

GAP = ord("-")
REGION_DT = np.dtype([(f, "<u4") for f in ("sample", "chrom", "start", "end", "snps")])
SAMPLE_DT = np.dtype([(f, "<u8") for f in ("sites", "callable", "ambiguous", "missing", "snps", "dense_snps", "regions", "region_bases")])
BIN_DT = np.dtype([("snps", "<u4"), ("dense_snps", "<u4")])
INFO_DT = np.dtype([(f, "<u8") for f in ("windows", "repeat_windows", "sites", "n_chrom", "n_bins", "n_snps", "n_regions")])
DENSE_BIT = 62
CODE = "ACTG"                                            # a record's two low bits
_RC = MM._rc_table(None)
_ACGT = np.zeros(256, bool)
for _c in b"ACGT":
    _ACGT[_c] = True


def sites(keys, k, rc, ref, mutant=None):
    """-> (windows, repeat_windows, [(chrom, pos, row, is_rc, repeated)] of the hit windows that are sites, in reference order)"""
    row_of = {key: r for r, key in enumerate(MM.key_ints(keys))}
    wins = [MM.chrom_windows(bytes(seq), k, rc) for _, seq in ref]
    count = {}
    for ws in wins:
        for _, split, _ in ws:
            count[split] = count.get(split, 0) + 1
    out, windows, repeats = [], 0, 0
    for c, ws in enumerate(wins):
        for pos, split, is_rc in ws:
            windows += 1
            repeated = count[split] > 1
            repeats += repeated
            row = row_of.get(split)
            if row is None or (repeated and mutant != "repeats_kept"):
                continue
            out.append((c, pos, row, is_rc, repeated))
    return windows, repeats, out


def dense_flags(p, W, T, inclusive=False):
    """p ascending positions of one (sample, chromosome) -> bool per SNP: one of T consecutive SNPs less than W apart"""
    p = np.asarray(p, np.int64)
    n = len(p)
    dense = np.zeros(n, bool)
    if n < T:
        return dense
    span = p[T - 1:] - p[:n - T + 1]
    q = span <= W if inclusive else span < W
    d = np.zeros(n + 1, np.int64)
    js = np.flatnonzero(q)
    np.add.at(d, js, 1)
    np.add.at(d, js + T, -1)
    return np.cumsum(d[:n]) > 0


def dense_sliding(p, W, T):
    """the sliding-window form in plain loops: SNP i is dense when some stretch [a, a + W) of reference positions holds p[i] and at least T SNPs"""
    out = []
    for pi in p:
        found = False
        for a in range(pi - W + 1, pi + 1):
            if sum(1 for x in p if a <= x < a + W) >= T:
                found = True
                break
        out.append(found)
    return out


def runs(dense):
    """[(first, last)] index pairs of the maximal runs of True"""
    out, i, n = [], 0, len(dense)
    while i < n:
        if dense[i]:
            j = i
            while j + 1 < n and dense[j + 1]:
                j += 1
            out.append((i, j))
            i = j + 1
        else:
            i += 1
    return out


def density(keys, var, k, rc, ref, W=1000, T=5, mutant=None):
    """-> dict: info (INFO_DT record), samples (SAMPLE_DT [S]), regions (REGION_DT), bins (BIN_DT), chrom_ids, chrom_lens, snps (uint64), snp_ref (uint8)"""
    assert mutant is None or mutant in MUTANTS, mutant
    assert 1 <= W <= 1 << 31 and 2 <= T <= 65535
    var = np.asarray(var, np.uint8)
    S = var.shape[1]
    seqs = [bytes(s) for _, s in ref]
    lens = [len(s) for s in seqs]
    offs = [0] + list(np.cumsum(lens))
    windows, repeats, st = sites(keys, k, rc, ref, mutant)
    nbin = [(n + W - 1) // W for n in lens]
    binoff = [0] + list(np.cumsum(nbin))
    samples = np.zeros(S, SAMPLE_DT)
    bins = np.zeros(binoff[-1], BIN_DT)
    regions, snps, snp_ref = [], [], []
    if st and S:
        chrom = np.array([x[0] for x in st], np.int64)
        pos = np.array([x[1] for x in st], np.int64)
        strand = np.array([x[3] for x in st], bool)
        cells = var[np.array([x[2] for x in st], np.int64)]
        cells = np.where(cells == 0, np.uint8(GAP), cells)
        if mutant != "no_rc_iupac":
            cells = np.where(strand[:, None], _RC[cells], cells)
        r = np.array([seqs[c][p] if mutant == "ref_case_sensitive" else seqs[c][p] & 0xDF for c, p, *_ in st], np.uint8)
        missing = cells == GAP
        plain = _ACGT[cells]
        ambiguous = ~missing & ~plain
        snp = plain & (cells != r[:, None])
        if mutant == "ambig_as_snp":
            snp |= ambiguous
        samples["callable"], samples["ambiguous"], samples["missing"], samples["snps"] = plain.sum(0), ambiguous.sum(0), missing.sum(0), snp.sum(0)
        xcat = pos + np.array(offs, np.int64)[chrom]
        for s in range(S):
            at = np.flatnonzero(snp[:, s])
            order = at[np.argsort(xcat[at], kind="stable")]
            dense = np.zeros(len(order), bool)
            groups = [order] if mutant == "span_chromosomes" else [order[chrom[order] == c] for c in range(len(ref))]
            done = 0
            for g in groups:
                if not len(g):
                    continue
                p = xcat[g] if mutant == "span_chromosomes" else pos[g]
                d = dense_flags(p, W, T, inclusive=mutant == "window_inclusive")
                dense[done:done + len(g)] = d
                done += len(g)
                for i0, i1 in runs(d):
                    c0 = int(chrom[g[i0]])
                    regions.append((s, c0, int(xcat[g[i0]]) - offs[c0], int(xcat[g[i1]]) - offs[c0], i1 - i0 + 1))
            samples["dense_snps"][s] = int(dense.sum())
            for i, d in zip(order, dense):
                c = int(chrom[i])
                b = binoff[c] + int(pos[i]) // W
                bins["snps"][b] += 1
                bins["dense_snps"][b] += int(d)
                base = chr(int(cells[i, s]))
                code = CODE.index(base) if base in CODE else 0
                snps.append((s << 34) | (int(xcat[i]) << 2) | code | (int(d) << DENSE_BIT))
                snp_ref.append(seqs[c][int(pos[i])] & 0xDF)
    regions = np.array(regions, REGION_DT) if regions else np.zeros(0, REGION_DT)
    for g in regions:
        samples["regions"][g["sample"]] += 1
        samples["region_bases"][g["sample"]] += int(g["end"]) - int(g["start"]) + 1
    samples["sites"] = len(st)
    info = np.zeros(1, INFO_DT)[0]
    info["windows"], info["repeat_windows"], info["sites"] = windows, repeats, len(st)
    info["n_chrom"], info["n_bins"], info["n_snps"], info["n_regions"] = len(ref), len(bins), len(snps), len(regions)
    return {"info": info, "samples": samples, "regions": regions, "bins": bins, "chrom_ids": [i for i, _ in ref], "chrom_lens": np.array(lens, np.uint64),
            "snps": np.array(snps, np.uint64), "snp_ref": np.array(snp_ref, np.uint8)}


# ---- texts
def regions_text(res, names):
    lines = ["sample\tchromosome\tstart\tend\tlength\tsnps"]
    for g in res["regions"]:
        a, b = int(g["start"]), int(g["end"])
        lines.append("\t".join([names[g["sample"]], res["chrom_ids"][g["chrom"]], str(a + 1), str(b + 1), str(b - a + 1), str(int(g["snps"]))]))
    return "\n".join(lines) + "\n"


def summary_text(res, names):
    lines = ["sample\tsites\tcallable\tambiguous\tmissing\tsnps\tdense_snps\tregions\tregion_bases\tsnps_outside"]
    for n, q in zip(names, res["samples"]):
        lines.append("\t".join([n] + [str(int(q[f])) for f in SAMPLE_DT.names] + [str(int(q["snps"]) - int(q["dense_snps"]))]))
    return "\n".join(lines) + "\n"


def bins_text(res, W):
    lines = ["chromosome\tstart\tend\tsnps\tdense_snps"]
    b = 0
    for i, n in zip(res["chrom_ids"], res["chrom_lens"]):
        n = int(n)
        for at in range(0, n, W):
            lines.append("\t".join([i, str(at + 1), str(min(at + W, n)), str(int(res["bins"]["snps"][b])), str(int(res["bins"]["dense_snps"][b]))]))
            b += 1
    assert b == len(res["bins"])
    return "\n".join(lines) + "\n"


def snps_text(res, names):
    offs = [0] + [int(x) for x in np.cumsum(res["chrom_lens"])]
    lines = ["sample\tchromosome\tposition\tref\talt\tdense"]
    for v, r in zip(res["snps"].tolist(), res["snp_ref"].tolist()):
        s, x = (v >> 34) & 0xFFFFFFF, (v >> 2) & 0xFFFFFFFF
        c = max(j for j in range(len(offs) - 1) if offs[j] <= x)
        lines.append("\t".join([names[s], res["chrom_ids"][c], str(x - offs[c] + 1), chr(r), CODE[v & 3], str((v >> DENSE_BIT) & 1)]))
    return "\n".join(lines) + "\n"


def masked_alignment(keys, var, names, k, rc, ref, res):
    """`ska map`'s alignment (repeat mask on) with the regions of res overwritten by 'N' where the line holds no '-' -> bytes"""
    aln = MM.MapModel(keys, var, names, k, rc, ref).alignment(ambig_mask=False, repeat_mask=True)
    offs = [0] + [int(x) for x in np.cumsum(res["chrom_lens"])]
    for g in res["regions"]:
        seg = aln[g["sample"], offs[g["chrom"]] + int(g["start"]):offs[g["chrom"]] + int(g["end"]) + 1]
        seg[seg != GAP] = ord("N")
    return b"".join(b">" + n.encode() + b"\n" + aln[s].tobytes() + b"\n" for s, n in enumerate(names))


def texts(keys, var, names, k, rc, ref, W=1000, T=5, snps=False, mutant=None):
    """-> {file suffix: text} as `ska density` writes them; ref: [(id, bytes)] with the id cut at its first white space"""
    res = density(keys, var, k, rc, ref, W, T, mutant)
    out = {".density.regions.tsv": regions_text(res, list(names)), ".density.summary.tsv": summary_text(res, list(names)), ".density.bins.tsv": bins_text(res, W)}
    if snps:
        out[".density.snps.tsv"] = snps_text(res, list(names))
    return out
