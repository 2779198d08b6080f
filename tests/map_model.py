"""Test-only model of `ska map`, written from the definition of its output and not from the reference's sequential writer:

  windows     every run of clean letters (ACGT, either case) of a chromosome gives one window per k letters, in the reference's
              2-bit code (A=0, C=1, T=2, G=3, first base in the high bits); a run that starts less than k + 1 letters before the
              end of its record gives none (the reference's iterator, which the oracle's comments call the split_kmer.rs:89 quirk)
  split k-mer the window without its middle base; with `rc` the smaller of it and its reverse complement's, `is_rc` when the
              reverse complement's is the smaller one
  mapped cell the array's cell of that split k-mer, through RC_IUPAC when `is_rc`
  alignment   per sample '-' everywhere; then the reference byte at every x that has a present (non-'-') mapped position p of the
              same chromosome with |x - p| <= half; then the middle bases ('N' for ambiguous ones with ambig_mask); then 'N' at the
              repeat coordinates that are not '-'
  repeats     windows whose split k-mer occurs more than once; [pos - half, pos + half] + chrom_offset, merged through last_end,
              where chrom_offset grows by the length of the last chromosome that had a window (so chromosomes without windows
              shift the coordinates of later repeats: the reference's quirk)
  text        >name / sequence lines, or VCF 4.4 lines as the oracle's ora_ref_write_aln / ora_ref_write_vcf print them

There is no term for stale writer state at a chromosome change: tests/test_map_model.py shows that none is needed.
`mutant=` switches on one deliberate mistake (MUTANTS); the tests use them to show that their inputs reach the edge each stands for."""
import numpy as np

from lo_model import windows as kmer_windows, rc as rc_int

MUTANTS = (
    "right_flank_short",       # the right flank radius is half - 1
    "left_flank_short",        # the left flank radius is half - 1
    "gap_cells_present",       # '-' cells count as present
    "flanks_over_middle",      # flanks win over middle bases
    "no_rc_iupac",             # rc_iupac is left out
    "rc_iupac_km_fixed",       # rc_iupac maps K -> K and M -> M
    "repeat_overwrites_gaps",  # the repeat mask also overwrites '-'
    "repeat_true_offsets",     # repeat coordinates use true chromosome offsets
    "ambig_mask_ignored",      # ambig_mask is ignored
)

GAP = ord("-")
_RC_PAIRS = {"A": "T", "B": "V", "C": "G", "D": "H", "G": "C", "H": "D", "K": "M", "M": "K", "N": "N", "R": "Y", "S": "S", "T": "A",
             "V": "B", "W": "W", "Y": "R"}


def _rc_table(mutant):
    t = np.full(256, GAP, np.uint8)                        # anything that is no IUPAC code -> '-'
    for a, b in _RC_PAIRS.items():
        if mutant == "rc_iupac_km_fixed" and a in "KM":
            b = a
        t[ord(a)] = t[ord(a.lower())] = ord(b)
    return t


_UNAMBIG = np.zeros(256, bool)
for _c in b"ACGTUacgtu-":
    _UNAMBIG[_c] = True
_UNAMBIG[GAP | 0x20] = True


def key_ints(keys):
    """the oracle's exported keys (lo, hi) as Python ints"""
    return [(int(h) << 64) | int(l) for l, h in zip(keys["lo"], keys["hi"])]


def chrom_windows(seq, k, rc):
    """[(pos of the middle base, split k-mer, is_rc)] of one chromosome"""
    bad = set(seq) - set(b"ACGTNacgtn")
    if bad:
        raise ValueError("the model covers references of ACGTN in either case only: %r" % bytes(sorted(bad)))
    half = (k - 1) // 2
    low = (1 << (2 * half)) - 1
    out = []
    text = seq.decode()
    n = len(text)
    a = 0
    while a < n:
        if text[a] in "Nn":
            a += 1
            continue
        b = a
        while b < n and text[b] not in "Nn":
            b += 1
        if a + k < n:                                       # the iterator's end-of-record test, made where a run starts
            for i, w in enumerate(kmer_windows(text[a:b], k)):
                split = ((w >> (2 * (half + 1))) << (2 * half)) | (w & low)
                is_rc = False
                if rc:
                    r = rc_int(w, k)
                    rsplit = ((r >> (2 * (half + 1))) << (2 * half)) | (r & low)
                    if split > rsplit:
                        split, is_rc = rsplit, True
                out.append((a + i + half, split, is_rc))
        a = b
    return out


class MapModel:
    """keys, variants[rows][S], names: the array as exported; ref: [(id, bytes)] with the id cut at its first white space;
    windows_from: another model of the same reference, k and rc, whose windows are taken over"""

    def __init__(self, keys, variants, names, k, rc, ref, mutant=None, windows_from=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.k, self.rc, self.half, self.mutant = k, rc, (k - 1) // 2, mutant
        self.names = list(names)
        self.ids = [i for i, _ in ref]
        self.seqs = [bytes(s) for _, s in ref]
        self.lens = [len(s) for s in self.seqs]
        self.offs = [0] + list(np.cumsum(self.lens))[:-1]
        self.total = sum(self.lens)
        self.refcat = np.frombuffer(b"".join(self.seqs), np.uint8)
        variants = np.asarray(variants, np.uint8)
        self.S = variants.shape[1]
        row_of = {key: r for r, key in enumerate(key_ints(keys))}
        self.win = windows_from.win if windows_from is not None else [chrom_windows(s, k, rc) for s in self.seqs]      # per chromosome
        m_chrom, m_pos, m_rc, rows = [], [], [], []
        for c, ws in enumerate(self.win):
            for pos, split, is_rc in ws:
                r = row_of.get(split)
                if r is not None:
                    m_chrom.append(c), m_pos.append(pos), m_rc.append(is_rc), rows.append(r)
        self.m_chrom, self.m_pos = np.array(m_chrom, np.int64), np.array(m_pos, np.int64)
        self.m_rc = np.array(m_rc, bool)
        cells = variants[np.array(rows, np.int64)] if rows else np.zeros((0, self.S), np.uint8)
        if mutant != "no_rc_iupac" and len(rows):
            cells = np.where(self.m_rc[:, None], _rc_table(mutant)[cells], cells)
        self.cells = cells                                                    # [mapped][S]

    # ---- repeat coordinates
    def repeat_coords(self):
        count = {}
        for ws in self.win:
            for _, split, _ in ws:
                count[split] = count.get(split, 0) + 1
        half = self.half
        coords = []
        last_chrom = last_end = chrom_offset = 0
        for c, ws in enumerate(self.win):
            for pos, split, _ in ws:
                if c > last_chrom:
                    chrom_offset += self.lens[last_chrom]
                    last_chrom = c
                off = self.offs[c] if self.mutant == "repeat_true_offsets" else chrom_offset
                if count[split] < 2:
                    continue
                start, end = pos - half + off, pos + half + off
                coords.extend(range(start if (start > last_end or start == 0) else last_end + 1, end + 1))
                last_end = end
        return np.array(coords, np.int64)

    # ---- alignment
    def present(self, s):
        """mask over the mapped positions: those that count as present for sample s"""
        if self.mutant == "gap_cells_present":
            return np.ones(len(self.m_pos), bool)
        return self.cells[:, s] != GAP

    def alignment(self, ambig_mask=False, repeat_mask=False):
        """uint8 [S][total]"""
        if self.mutant == "ambig_mask_ignored":
            ambig_mask = False
        half = self.half
        left = half - 1 if self.mutant == "left_flank_short" else half
        right = half - 1 if self.mutant == "right_flank_short" else half
        rep = self.repeat_coords() if repeat_mask else np.zeros(0, np.int64)
        out = np.full((self.S, self.total), GAP, np.uint8)
        mid_x = self.m_pos + np.array(self.offs, np.int64)[self.m_chrom] if len(self.m_pos) else self.m_pos
        for s in range(self.S):
            o = out[s]
            pres = self.present(s)
            real = self.cells[:, s] != GAP
            base = self.cells[:, s].copy()
            if ambig_mask:
                base[~_UNAMBIG[base]] = ord("N")
            if self.mutant == "flanks_over_middle":
                o[mid_x[real]] = base[real]
            for c in range(len(self.seqs)):
                p = self.m_pos[pres & (self.m_chrom == c)]
                if not len(p):
                    continue
                n = self.lens[c]
                d = np.zeros(n + 1, np.int64)
                np.add.at(d, np.maximum(p - left, 0), 1)
                np.add.at(d, np.minimum(p + right, n - 1) + 1, -1)
                cov = np.cumsum(d[:n]) > 0
                seg = o[self.offs[c]:self.offs[c] + n]
                seg[cov] = self.refcat[self.offs[c]:self.offs[c] + n][cov]
            if self.mutant != "flanks_over_middle":
                o[mid_x[real]] = base[real]
            if len(rep):
                hit = rep if self.mutant == "repeat_overwrites_gaps" else rep[o[rep] != GAP]
                o[hit] = ord("N")
        return out

    # ---- text
    def write_aln(self, ambig_mask=False, repeat_mask=False):
        aln = self.alignment(ambig_mask, repeat_mask)
        return b"".join(b">" + n.encode() + b"\n" + aln[s].tobytes() + b"\n" for s, n in enumerate(self.names))

    def write_vcf(self, ambig_mask=False, repeat_mask=False):
        aln = self.alignment(ambig_mask, repeat_mask)
        out = ["##fileformat=VCFv4.4\n"]
        out += ["##contig=<ID=%s>\n" % i for i in self.ids]
        out.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + "".join("\t" + n for n in self.names) + "\n")
        chrom_of = np.repeat(np.arange(len(self.seqs)), self.lens)
        for idx in np.flatnonzero((aln != self.refcat[None, :]).any(axis=0)):
            c = int(chrom_of[idx])
            ref_base = int(self.refcat[idx])
            alts, gts = [], []
            for m in aln[:, idx].tolist():
                if m == ref_base:
                    gts.append("0")
                elif m == GAP:
                    gts.append(".")
                else:
                    a = chr(m) if chr(m) in "ACGT" else "N"
                    if a not in alts:
                        alts.append(a)
                    gts.append(str(alts.index(a) + 1))
            r = chr(ref_base) if chr(ref_base) in "ACGT" else "N"
            out.append("%s\t%d\t.\t%s\t%s\t.\t.\t.\tGT\t%s\n" % (self.ids[c], idx - self.offs[c] + 1, r, ",".join(alts) or ".", "\t".join(gts)))
        return "".join(out).encode()

    def text(self, fmt="aln", ambig_mask=False, repeat_mask=False):
        return (self.write_vcf if fmt == "vcf" else self.write_aln)(ambig_mask, repeat_mask)
