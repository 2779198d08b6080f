"""`ska screen` on the CPU: the model (tests/screen_model.py) against (1) the oracle's `ska map` of the same panel, (2) the oracle's
`weed --reverse` and the per-sample k-mer counts that are left, (3) a hand-worked example at k = 9, (4) a cell-by-cell restatement in plain loops
-- and (5) its mutants, each of which must fail at least one of the four, shown by running it.  The panels of (1) and (2) are the committed
references under tests/golden/input, which are upper-case already."""
import functools
import os

import numpy as np
import pytest

import map_model as MM
import ora
import screen_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUT = os.path.join(ROOT, "tests", "golden", "input")
KEY_DT = np.dtype([("lo", "<u8"), ("hi", "<u8")])
SAMPLES = ("test_1", "test_2", "N_test_1", "N_test_2", "test_2_rc")
KS = (9, 17, 31)


def _fasta(name):
    """[(id, sequence)] of a committed input"""
    out = []
    for block in open(os.path.join(INPUT, name), "rb").read().split(b">")[1:]:
        head, _, rest = block.partition(b"\n")
        out.append((head.split()[0].decode(), rest.replace(b"\n", b"").replace(b"\r", b"")))
    return out


@functools.lru_cache(maxsize=None)
def _panels():
    two = _fasta("test_ref_two_chrom.fa")
    mixed = ([("ref", _fasta("test_ref.fa")[0][1])] + _fasta("weed.fa") + [("n1", _fasta("N_test_1.fa")[0][1]), ("back", _fasta("test_2_rc.fa")[0][1])]
             + [(i + "_again", s) for i, s in _fasta("test_ref_two_chrom_repeats.fa")])
    for panel in (two, mixed):
        assert all(s == s.upper() and set(s) <= set(b"ACGTN") for _, s in panel)
    return {"two_chrom": two, "mixed": mixed}


def _oracle_array(k):
    return ora.Array.build([(n, os.path.join(INPUT, n + ".fa"), None) for n in SAMPLES], k=k, rc=True)


def _write(path, panel):
    with open(path, "wb") as f:
        for i, s in panel:
            f.write(b">" + i.encode() + b" some description\n" + s + b"\n")
    return str(path)


@functools.lru_cache(maxsize=None)
def _oracle_world(k):
    oa = _oracle_array(k)
    keys, var, _ = oa.export()
    return oa, keys, var


# ---- (1) the oracle's `ska map`
def _map_differences(tmp, k, name):
    """per record and sample: the positions of the oracle's alignment that are neither '-' nor the reference byte"""
    oa, _, _ = _oracle_world(k)
    panel = _panels()[name]
    aln = oa.map(_write(os.path.join(tmp, f"{name}_{k}.fa"), panel)).split(b"\n")
    assert [l[1:].decode() for l in aln[0::2] if l] == list(SAMPLES)
    out = np.zeros((len(panel), len(SAMPLES)), np.int64)
    for s, line in enumerate(aln[1::2]):
        at = 0
        for r, (_, seq) in enumerate(panel):
            got = np.frombuffer(line[at:at + len(seq)], np.uint8)
            out[r, s] = int(((got != ord("-")) & (got != np.frombuffer(seq, np.uint8))).sum())
            at += len(seq)
        assert at == len(line)
    return out


def _check_map(tmp, mutant=None):
    ok, differences = True, 0
    for k in KS:
        _, keys, var = _oracle_world(k)
        for name, panel in _panels().items():
            want = _map_differences(tmp, k, name)
            _, counts = SM.screen(keys, var, k, True, panel, mutant)
            ok &= np.array_equal(counts[:, :, 0].astype(np.int64) - counts[:, :, 1], want)
            differences += int(want.sum())
    assert differences > 0                                  # (the samples do differ from the panel somewhere)
    return ok


# ---- (2) the oracle's `weed --reverse` + per-sample k-mer counts
def _check_weed(tmp, mutant=None):
    ok = True
    for k in (17, 31):
        _, keys, var = _oracle_world(k)
        panel = [("ref", _fasta("test_ref.fa")[0][1])]
        splits = [w[1] for w in MM.chrom_windows(panel[0][1], k, True)]
        assert len(set(splits)) == len(splits) > 0          # no repeated split k-mer: a window a row
        weeded = _oracle_array(k)
        weeded.weed(_write(os.path.join(tmp, f"weed_{k}.fa"), panel), reverse=True, min_freq=0.0, filter_type=ora.FILTER_NONE)
        left = weeded.export()[1]
        per_sample = ((left != ord("-")) & (left != 0)).sum(axis=0)
        assert 0 < per_sample.min() and weeded.nrows < len(var)
        _, counts = SM.screen(keys, var, k, True, panel, mutant)
        ok &= counts[0, :, 0].tolist() == per_sample.tolist()
    return ok


# ---- (3) a hand-worked example at k = 9
A = b"ACGGTCATTGCA"                        # 12 letters: 4 windows
B = b"AAGACCGTAA" + b"N" + b"GCATCGGATTC"   # runs of 10 and 11 letters around an N: 2 + 3 windows
SHORT = b"ACGTTGCAT"                        # k letters: no window (the iterator asks for k + 1 where a run starts)
D = A[:10]                                  # 2 windows, the split k-mers of A's first two
HAND_PANEL = [("A", A), ("B", B), ("short", SHORT), ("D", D)]
RC = {"A": "T", "C": "G", "G": "C", "T": "A", "Y": "R", "N": "N", "-": "-"}


def _other(base):
    return "ACGT"[("ACGT".index(base) + 1) % 4]


def _hand_array():
    """three samples; rows: A's windows 0, 1, 2 (not 3), B's windows 0 and 3 (not 1, 2, 4).  The cells are written as the panel's strand sees
    them (X = the record's own middle base, o = another base) and stored through RC_IUPAC where the window's canonical split k-mer is the reverse
    complement's"""
    wa, wb = MM.chrom_windows(A, 9, True), MM.chrom_windows(B, 9, True)
    assert [w[0] for w in wa] == [4, 5, 6, 7] and [w[0] for w in wb] == [4, 5, 15, 16, 17] and MM.chrom_windows(SHORT, 9, True) == []
    assert [w[1] for w in MM.chrom_windows(D, 9, True)] == [w[1] for w in wa[:2]]
    assert len({w[1] for w in wa + wb}) == 9
    seen = [(A, wa[0], "XX-"), (A, wa[1], "XoY"), (A, wa[2], "X-X"), (B, wb[0], "XXX"), (B, wb[3], "NX-")]
    assert {w[2] for _, w, _ in seen} == {False, True}      # both strands among the hit windows
    keys, var = np.zeros(len(seen), KEY_DT), np.zeros((len(seen), 3), np.uint8)
    for i, (seq, (pos, split, is_rc), cells) in enumerate(seen):
        keys[i] = (split & ((1 << 64) - 1), split >> 64)
        x = chr(seq[pos])
        for s, c in enumerate(cells):
            c = {"X": x, "o": _other(x)}.get(c, c)
            var[i, s] = ord(RC[c] if is_rc else c)
    order = np.array([3, 0, 4, 2, 1])                       # (the rows in no particular order)
    return keys[order], var[order]


HAND_RECORDS = [(12, 4, 3), (22, 5, 2), (9, 0, 0), (10, 2, 2)]
HAND_COUNTS = [[[3, 3, 0], [2, 1, 0], [2, 1, 1]],          # A: s1 has another base at window 1 and a gap at 2, s2 a gap at 0 and a Y at 1
               [[2, 1, 1], [2, 2, 0], [1, 1, 0]],          # B: s0 has an N at window 3, s2 a gap there
               [[0, 0, 0], [0, 0, 0], [0, 0, 0]],
               [[2, 2, 0], [2, 1, 0], [1, 0, 1]]]          # D: A's windows 0 and 1 again
# C = 0.5, I = 0.6.  A needs found >= 2 and passes for s0 alone (s1, s2: match 1 < ceil(1.2)); B needs ceil(2.5) = 3 found: nobody; short has no
# window; D needs 1: s0 passes, s1 has match 1 < 2, s2 match 0 < ceil(0.6) = 1
HAND_TEXTS = {
    ".screen.tsv": "record\tlength\twindows\tsample\tfound\tmatch\tambig\tsnp\tcover\tidentity\n"
                   "A\t12\t4\ts0\t3\t3\t0\t0\t0.7500\t1.0000\n"
                   "D\t10\t2\ts0\t2\t2\t0\t0\t1.0000\t1.0000\n",
    ".screen.summary.tsv": "record\tlength\twindows\trows_hit\tsamples_passing\n"
                           "A\t12\t4\t3\t1\nB\t22\t5\t2\t0\nshort\t9\t0\t0\t0\nD\t10\t2\t2\t1\n",
    ".screen.matrix.tsv": "record\ts0\ts1\ts2\nA\t1\t0\t0\nB\t0\t0\t0\nshort\t0\t0\t0\nD\t1\t0\t0\n",
}


def _check_hand(mutant=None):
    keys, var = _hand_array()
    records, counts = SM.screen(keys, var, 9, True, HAND_PANEL, mutant)
    ok = [tuple(int(x) for x in r) for r in records] == HAND_RECORDS and counts.tolist() == HAND_COUNTS
    ok &= SM.texts(keys, var, ["s0", "s1", "s2"], 9, True, HAND_PANEL, 0.5, 0.6, matrix=True, mutant=mutant) == HAND_TEXTS
    return bool(ok)


# ---- (4) cell by cell in plain loops
def _check_slow(mutant=None):
    ok = True
    worlds = [(9, True, _hand_array(), HAND_PANEL)] + [(k, True, _oracle_world(k)[1:], _panels()["mixed"]) for k in (9, 17)]
    for k, rc, (keys, var), panel in worlds:
        records, counts = SM.screen(keys, var, k, rc, panel, mutant)
        srec, scounts = SM.screen_slow(keys, var, k, rc, panel)
        ok &= [[int(x) for x in r] for r in records] == srec and counts.tolist() == scounts
    return bool(ok)


def test_oracle_map(tmp_path):
    assert _check_map(str(tmp_path))


def test_oracle_weed_reverse(tmp_path):
    assert _check_weed(str(tmp_path))


def test_hand_worked_example():
    assert _check_hand()
    keys, var = _hand_array()
    records, counts = SM.screen(keys, var, 9, True, HAND_PANEL)
    ok = SM.passes(records, counts, 0.5, 0.6)
    assert ok.tolist() == [[True, False, False], [False] * 3, [False] * 3, [True, False, False]]
    assert SM.passes(records, counts, 0.0, 0.0).tolist() == [[True] * 3, [True] * 3, [False] * 3, [True] * 3]     # found >= 1 is always asked
    assert SM.passes(records, counts, 1.0, 1.0).tolist() == [[False] * 3, [False] * 3, [False] * 3, [True, False, False]]
    assert sorted(SM.texts(keys, var, ["s0", "s1", "s2"], 9, True, HAND_PANEL)) == [".screen.summary.tsv", ".screen.tsv"]      # no matrix unless asked


def test_cell_by_cell():
    assert _check_slow()


def test_single_strand_has_no_reverse_windows():
    keys, var = _hand_array()
    windows = SM.record_windows(HAND_PANEL, 9, False)
    assert not any(w[2] for ws in windows for w in ws)
    records, _ = SM.screen(keys, var, 9, False, HAND_PANEL)
    assert [int(r["windows"]) for r in records] == [4, 5, 0, 2]


@pytest.mark.parametrize("mutant", SM.MUTANTS)
def test_every_mutant_is_caught(tmp_path, mutant):
    results = {"map": _check_map(str(tmp_path), mutant), "weed": _check_weed(str(tmp_path), mutant), "hand": _check_hand(mutant), "slow": _check_slow(mutant)}
    assert not all(results.values()), (mutant, results)
