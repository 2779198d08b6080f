"""`ska density` on the CPU: the model (tests/density_model.py) against (1) the oracle's `ska map` of the same reference at k = 9, 17, 31 and 41,
(2) the sliding-window restatement of "dense" in plain loops, (3) a hand-worked example at k = 9, (4) the invariant missing + ambiguous +
callable = sites -- and (5) its mutants, each of which must fail at least one of the four, shown by running it.  The host's texts and the masked
alignment (skh_density_text, skh_density_mask_alignment: no device) are held against the model's through ctypes.  The references of (1) are
the committed ones under tests/golden/input, which are upper-case already."""
import functools
import os

import numpy as np
import pytest

import density_model as DM
import map_model as MM
import ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT = os.path.join(ROOT, "tests", "golden", "input")
KEY_DT = np.dtype([("lo", "<u8"), ("hi", "<u8")])
SAMPLES = ("test_1", "test_2", "N_test_1", "N_test_2", "test_2_rc")
KS = (9, 17, 31, 41)
REFS = ("test_ref.fa", "test_ref_two_chrom.fa", "test_ref_two_chrom_repeats.fa")


def _fasta(name):
    """[(id, sequence)] of a committed input"""
    out = []
    for block in open(os.path.join(INPUT, name), "rb").read().split(b">")[1:]:
        head, _, rest = block.partition(b"\n")
        out.append((head.split()[0].decode(), rest.replace(b"\n", b"").replace(b"\r", b"")))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_world(k):
    oa = ora.Array.build([(n, os.path.join(INPUT, n + ".fa"), None) for n in SAMPLES], k=k, rc=True)
    keys, var, _ = oa.export()
    return oa, keys, var


# ---- (1) the oracle's `ska map`
def _check_map(mutant=None):
    """per sample: the model's SNP positions, which never lie on the middle of a repeated window, plus the middles of repeated windows at which
    the alignment differs = the alignment's positions that are one of A, C, G, T and differ from the upper-cased reference"""
    ok, differences, on_repeats = True, 0, 0
    for k in KS:
        oa, keys, var = _oracle_world(k)
        for name in REFS:
            ref = _fasta(name)
            assert all(s == s.upper() and set(s) <= set(b"ACGTN") for _, s in ref)
            aln = oa.map(os.path.join(INPUT, name)).split(b"\n")
            assert [l[1:].decode() for l in aln[0::2] if l] == list(SAMPLES)
            refcat = np.frombuffer(b"".join(s for _, s in ref), np.uint8)
            offs = np.concatenate([[0], np.cumsum([len(s) for _, s in ref])])
            wins = [MM.chrom_windows(s, k, True) for _, s in ref]
            count = {}
            for ws in wins:
                for _, split, _ in ws:
                    count[split] = count.get(split, 0) + 1
            rep_mid = {int(offs[c]) + pos for c, ws in enumerate(wins) for pos, split, _ in ws if count[split] > 1}
            res = DM.density(keys, var, k, True, ref, 1000, 5, mutant)
            model = [set() for _ in SAMPLES]
            for v in res["snps"].tolist():
                model[(v >> 34) & 0xFFFFFFF].add((v >> 2) & 0xFFFFFFFF)
            for s, line in enumerate(aln[1::2][:len(SAMPLES)]):
                got = np.frombuffer(line, np.uint8)
                assert len(got) == len(refcat)
                diff = set(np.flatnonzero(DM._ACGT[got] & (got != refcat)).tolist())
                ok &= not (model[s] & rep_mid) and (model[s] | (rep_mid & diff)) == diff
                differences += len(diff)
                on_repeats += len(rep_mid & diff)
            ok &= np.array_equal(res["samples"]["missing"] + res["samples"]["ambiguous"] + res["samples"]["callable"], res["samples"]["sites"])
    assert differences > 0 and on_repeats > 0                 # (the samples differ from the references, on repeated windows too)
    return bool(ok)


# ---- (2) the sliding-window form
def _check_sliding(mutant=None):
    rng = np.random.default_rng(5)
    ok = True
    for W, T in ((1, 2), (2, 2), (5, 2), (5, 3), (9, 4), (12, 3), (12, 13)):
        for n in (0, 1, T - 1, T, T + 1, 25):
            p = np.sort(rng.choice(60, size=min(n, 60), replace=False)).tolist()
            ok &= DM.dense_flags(p, W, T, inclusive=mutant == "window_inclusive").tolist() == DM.dense_sliding(p, W, T)
    return bool(ok)


# ---- (3) a hand-worked example at k = 9, W = 12, T = 3
A = b"TGGCCAAAATGTGG"                                                            # 14 letters in front of the N: middles 4 .. 9
B = b"TGGGGTCTGACTGATGTAATAGACCCCAAAAGGGCGTCCTTTCGTGTGGCTAGGTGCCCCGTATGCGGCC"    # 70 letters behind it: middles 19 .. 80 of c1
C1 = A + b"N" + B                                                                # 85 letters
REP = B[40:52]                                                                   # c1 55 .. 66: the windows with middles 59 .. 62 lie inside
C2 = b"GGGCTCCTCAGGAACTCTCATTAAG" + b"cgatcttgatagcta" + b"TAGGTCTG" + REP + b"TATTAC"      # 66 letters, 25 .. 39 in lower case, REP at 48 .. 59
HAND_REF = [("c1", C1), ("c2", C2)]
HAND_W, HAND_T = 12, 3
HAND_NAMES = ["s0", "s1", "s2"]
# (chromosome, position, sample) -> what the sample has there as the reference's strand reads it: o another base, '-', N
HAND_CELLS = {
    (0, 20, 0): "o", (0, 25, 0): "o", (0, 31, 0): "o",        # 31 - 20 = 11 = W - 1: dense
    (0, 45, 0): "o", (0, 50, 0): "o", (0, 57, 0): "o",        # 57 - 45 = 12 = W: not dense
    (0, 60, 0): "o",                                          # on a repeated window: no site (else 50, 57, 60 would be a run)
    (0, 20, 1): "o", (0, 24, 1): "o", (0, 31, 1): "o", (0, 40, 1): "o", (0, 42, 1): "o",      # 20-24-31 and 31-40-42 qualify, 24-31-40 does not: the runs touch in 31
    (1, 30, 1): "o",                                          # in the lower-case stretch
    (0, 79, 2): "o", (0, 80, 2): "o", (1, 4, 2): "o",         # 10 apart along the concatenated reference, but two SNPs on c1 and one on c2
    (1, 10, 2): "N", (1, 11, 2): "-", (1, 12, 2): "-",
}
RC = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "-": "-"}


def _other(base):
    return "ACGT"[("ACGT".index(base) + 1) % 4]


def _hand_array():
    """a row for every split k-mer of the reference; every cell the reference's own base, but for HAND_CELLS; stored through RC_IUPAC where the
    window's canonical split k-mer is the reverse complement's"""
    wins = [MM.chrom_windows(s, 9, True) for _, s in HAND_REF]
    assert [w[0] for w in wins[0]] == list(range(4, 10)) + list(range(19, 81)) and [w[0] for w in wins[1]] == list(range(4, 62))
    count = {}
    for ws in wins:
        for _, split, _ in ws:
            count[split] = count.get(split, 0) + 1
    assert [[w[0] for w in ws if count[w[1]] > 1] for ws in wins] == [[59, 60, 61, 62], [52, 53, 54, 55]] and max(count.values()) == 2
    assert {w[2] for ws in wins for w in ws} == {False, True}                     # both strands
    assert {w[2] for c, ws in enumerate(wins) for w in ws if (c, w[0], 0) in HAND_CELLS or (c, w[0], 1) in HAND_CELLS} == {False, True}
    rows = {}
    for c, ws in enumerate(wins):
        for pos, split, is_rc in ws:
            x = chr(HAND_REF[c][1][pos]).upper()
            cells = []
            for s in range(3):
                v = HAND_CELLS.get((c, pos, s), "X")
                v = {"X": x, "o": _other(x)}.get(v, v)
                cells.append(ord(RC[v] if is_rc else v))
            rows.setdefault(split, cells)                     # (a repeated split k-mer keeps its first window's cells)
    splits = sorted(rows, key=lambda v: (v * 2654435761) % 1000003)              # (the rows in no particular order)
    keys = np.array([(v & ((1 << 64) - 1), v >> 64) for v in splits], KEY_DT)
    var = np.array([rows[v] for v in splits], np.uint8)
    return keys, var


HAND_INFO = dict(windows=126, repeat_windows=8, sites=118, n_chrom=2, n_bins=8 + 6, n_snps=15, n_regions=2)
HAND_SAMPLES = [(118, 118, 0, 0, 6, 3, 1, 12), (118, 118, 0, 0, 6, 5, 1, 23), (118, 115, 1, 2, 3, 0, 0, 0)]
HAND_REGIONS = [(0, 0, 20, 31, 3), (1, 0, 20, 42, 5)]
HAND_BINS = [(0, 0), (2, 2), (4, 4), (3, 2), (2, 0), (0, 0), (2, 0), (0, 0), (1, 0), (0, 0), (1, 0), (0, 0), (0, 0), (0, 0)]
HAND_REGIONS_TEXT = "sample\tchromosome\tstart\tend\tlength\tsnps\ns0\tc1\t21\t32\t12\t3\ns1\tc1\t21\t43\t23\t5\n"
HAND_SUMMARY_TEXT = ("sample\tsites\tcallable\tambiguous\tmissing\tsnps\tdense_snps\tregions\tregion_bases\tsnps_outside\n"
                     "s0\t118\t118\t0\t0\t6\t3\t1\t12\t3\ns1\t118\t118\t0\t0\t6\t5\t1\t23\t1\ns2\t118\t115\t1\t2\t3\t0\t0\t0\t3\n")
HAND_BINS_HEAD = "chromosome\tstart\tend\tsnps\tdense_snps\nc1\t1\t12\t0\t0\nc1\t13\t24\t2\t2\n"
HAND_BINS_EDGES = ["c1\t85\t85\t0\t0", "c2\t1\t12\t1\t0", "c2\t61\t66\t0\t0"]


def _check_hand(mutant=None):
    keys, var = _hand_array()
    res = DM.density(keys, var, 9, True, HAND_REF, HAND_W, HAND_T, mutant)
    ok = {f: int(res["info"][f]) for f in DM.INFO_DT.names} == HAND_INFO
    ok &= [tuple(int(x) for x in q) for q in res["samples"]] == HAND_SAMPLES
    ok &= [tuple(int(x) for x in g) for g in res["regions"]] == HAND_REGIONS
    ok &= [tuple(int(x) for x in b) for b in res["bins"]] == HAND_BINS
    t = DM.texts(keys, var, HAND_NAMES, 9, True, HAND_REF, HAND_W, HAND_T, snps=True, mutant=mutant)
    ok &= t[".density.regions.tsv"] == HAND_REGIONS_TEXT and t[".density.summary.tsv"] == HAND_SUMMARY_TEXT
    ok &= t[".density.bins.tsv"].startswith(HAND_BINS_HEAD) and all(l in t[".density.bins.tsv"].split("\n") for l in HAND_BINS_EDGES)
    snps = t[".density.snps.tsv"].split("\n")
    x, y = chr(C1[20]), chr(C2[30]).upper()
    ok &= f"s0\tc1\t21\t{x}\t{_other(x)}\t1" in snps and f"s1\tc2\t31\t{y}\t{_other(y)}\t0" in snps and f"s0\tc1\t58\t{chr(C1[57])}\t{_other(chr(C1[57]))}\t0" in snps
    return bool(ok)


def test_oracle_map():
    assert _check_map()


def test_sliding_window_form():
    assert _check_sliding()
    assert DM.dense_flags([0, 11, 12], 12, 2).tolist() == [True, True, True] and DM.dense_flags([0, 12], 12, 2).tolist() == [False, False]
    assert DM.dense_flags([3], 1, 2).tolist() == [False] and DM.dense_flags([], 5, 2).tolist() == []


def test_hand_worked_example():
    assert _check_hand()
    keys, var = _hand_array()
    res = DM.density(keys, var, 9, True, HAND_REF, HAND_W, HAND_T)
    plain = [v & ~(1 << DM.DENSE_BIT) for v in res["snps"].tolist()]
    assert len(plain) == 15 and sorted(plain) == plain and sum(v >> DM.DENSE_BIT for v in res["snps"].tolist()) == 8
    at_13 = DM.density(keys, var, 9, True, HAND_REF, 13, HAND_T)                  # one position more and the run of exactly W is dense too: s0's
    assert [tuple(int(x) for x in g) for g in at_13["regions"]] == [(0, 0, 20, 57, 6), (1, 0, 20, 42, 5)]      # six SNPs are consecutive and all dense, one region
    none = DM.density(keys, var, 9, True, HAND_REF, HAND_W, 7)                    # T larger than any sample's SNPs
    assert len(none["regions"]) == 0 and not none["samples"]["dense_snps"].any() and int(none["info"]["n_snps"]) == 15


def test_invariant_and_empty_inputs():
    keys, var = _hand_array()
    for W, T in ((1, 2), (12, 3), (1 << 31, 65535)):
        q = DM.density(keys, var, 9, True, HAND_REF, W, T)["samples"]
        assert np.array_equal(q["missing"] + q["ambiguous"] + q["callable"], q["sites"]) and (q["dense_snps"] <= q["snps"]).all()
    res = DM.density(np.zeros(0, KEY_DT), np.zeros((0, 3), np.uint8), 9, True, HAND_REF, HAND_W, HAND_T)
    assert int(res["info"]["sites"]) == 0 and int(res["info"]["windows"]) == 126 and not any(res["samples"][f].any() for f in DM.SAMPLE_DT.names)
    assert len(res["bins"]) == 14 and not res["bins"]["snps"].any()
    single = DM.density(keys, var, 9, False, HAND_REF, HAND_W, HAND_T)            # one strand: no window is reverse-complemented
    assert not any(x[3] for x in DM.sites(keys, 9, False, HAND_REF)[2]) and int(single["info"]["windows"]) == 126


@pytest.mark.parametrize("mutant", DM.MUTANTS)
def test_every_mutant_is_caught(mutant):
    results = {"map": _check_map(mutant), "sliding": _check_sliding(mutant), "hand": _check_hand(mutant)}
    assert not all(results.values()), (mutant, results)


# ---- the host's texts and the masked alignment, through ctypes (no device)
def test_host_texts_equal_the_model():
    import skx_engine as E
    keys, var = _hand_array()
    worlds = [(keys, var, HAND_NAMES, 9, HAND_REF, W, T) for W, T in ((HAND_W, HAND_T), (13, 3), (1, 2), (40, 2))]
    _, okeys, ovar = _oracle_world(17)
    worlds.append((okeys, ovar, list(SAMPLES), 17, _fasta("test_ref_two_chrom_repeats.fa"), 50, 2))
    for keys, var, names, k, ref, W, T in worlds:
        res = DM.density(keys, var, k, True, ref, W, T)
        want = DM.texts(keys, var, names, k, True, ref, W, T, snps=True)
        got = {".density.regions.tsv": E.density_text(E.DENSITY_REGIONS, res, names, W), ".density.summary.tsv": E.density_text(E.DENSITY_SUMMARY, res, names, W),
               ".density.bins.tsv": E.density_text(E.DENSITY_BINS, res, names, W), ".density.snps.tsv": E.density_text(E.DENSITY_SNPS, res, names, W)}
        assert got == want, (k, W, T)
        plain = MM.MapModel(keys, var, names, k, True, ref).write_aln(repeat_mask=True)
        masked = DM.masked_alignment(keys, var, names, k, True, ref, res)
        assert E.density_mask_alignment(plain, res, names) == masked
        if len(res["regions"]):
            assert masked != plain and masked.count(b"N") > plain.count(b"N")
    assert (E.DENSITY_REGION_DT, E.DENSITY_SAMPLE_DT, E.DENSITY_BIN_DT, E.DENSITY_INFO_DT) == (DM.REGION_DT, DM.SAMPLE_DT, DM.BIN_DT, DM.INFO_DT)


def test_host_texts_refuse_what_does_not_fit():
    import skx_engine as E
    keys, var = _hand_array()
    res = DM.density(keys, var, 9, True, HAND_REF, HAND_W, HAND_T)
    for call, words in ((lambda: E.density_text(7, res, HAND_NAMES, HAND_W), "bad arguments"),
                        (lambda: E.density_text(E.DENSITY_BINS, res, HAND_NAMES, 0), "window"),
                        (lambda: E.density_text(E.DENSITY_BINS, res, HAND_NAMES, 10), "not those of this window"),
                        (lambda: E.density_text(E.DENSITY_REGIONS, res, HAND_NAMES[:1], HAND_W), "not there"),
                        (lambda: E.density_text(E.DENSITY_SNPS, dict(res, snps=None), HAND_NAMES, HAND_W), "not asked for"),
                        (lambda: E.density_mask_alignment(b">s0\nACGT\n", res, HAND_NAMES), "not the alignment")):
        with pytest.raises(E.EngineError) as ei:
            call()
        assert ei.value.code == E.EINVAL and words in str(ei.value), str(ei.value)
