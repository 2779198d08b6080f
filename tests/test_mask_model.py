"""`ska mask` on the CPU: the model (tests/mask_model.py) against (1) the oracle's `ska map` of the masked array at k = 9, 17, 31 and 41, (2) the
oracle's `ska weed` for a BED interval, (3) the oracle's delete_samples for intervals that cover the whole reference, (4) a hand-worked example at
k = 9, (5) a restatement in plain loops over positions, (6) idempotence -- and (7) its mutants, each of which must fail at least one of these,
shown by running it.  The host's readers and its summary text (skh_mask_read_regions, skh_mask_read_bed, skh_mask_text: no device) are held
against the model's through ctypes, every refusal with its line number and every truncation of a good file.

(1) in full: `ska map` writes, besides a window's middle base, the reference's own letters over the window's two arms wherever the middle is
present.  So a masked position does not always read '-': next to a window that is still present it reads the reference's letter.  What is
checked is therefore: away from every masked cell (more than (k-1)/2 positions) the line is unchanged, repeated windows included; at a masked
cell the line holds '-' or the reference's own letter, never the sample's differing base; and where every window within (k-1)/2 positions is a
masked site, it holds '-'."""
import functools
import os
import re

import numpy as np
import pytest

import map_model as MM
import mask_model as KM
import ora
import test_density_model as TM

ALL = KM.ALL
KEY_DT = TM.KEY_DT
INPUT = TM.INPUT


def _counts(var):
    return ((var != 0) & (var != KM.GAP)).sum(1).astype(np.uint64)


def _windows(ref, k, rc=True):
    wins = [MM.chrom_windows(bytes(s), k, rc) for _, s in ref]
    count = {}
    for ws in wins:
        for _, split, _ in ws:
            count[split] = count.get(split, 0) + 1
    return wins, count


# ---- (1) the oracle's `ska map`
@functools.lru_cache(maxsize=None)
def _map_world(k, name):
    oa, keys, var = TM._oracle_world(k)
    ref = TM._fasta(name)
    path = os.path.join(INPUT, name)
    lines = oa.map(path).split(b"\n")[1::2][:len(TM.SAMPLES)]
    return keys, var, ref, path, [np.frombuffer(l, np.uint8) for l in lines]


def _map_intervals(ref, S):
    """per sample two intervals on the first chromosome and one that ends on the last position of the last, and an ALL interval"""
    out = []
    n0, c_last, n_last = len(ref[0][1]), len(ref) - 1, len(ref[-1][1])
    for s in range(S):
        a = (5 + 7 * s) % (n0 - 12)
        out += [(s, 0, a, a + 4), (s, 0, a + 3, a + 9), (s, c_last, n_last - 6 - s, n_last - 1)]
    out.append((ALL, 0, n0 // 2, n0 // 2 + 3))
    return out


def _check_map(mutant=None):
    ok, masked_snps, kept_flank = True, 0, 0
    for k in TM.KS:
        half = (k - 1) // 2
        for name in TM.REFS:
            keys, var, ref, path, before = _map_world(k, name)
            S = var.shape[1]
            iv = _map_intervals(ref, S)
            res = KM.mask(keys, var, _counts(var), k, True, ref, iv, mutant)
            masked = ora.Array.from_rows(k, True, list(TM.SAMPLES), res["keys"], res["var"], res["counts"])
            after = [np.frombuffer(l, np.uint8) for l in masked.map(path).split(b"\n")[1::2][:S]]
            offs = np.concatenate([[0], np.cumsum([len(s) for _, s in ref])])
            refcat = np.frombuffer(b"".join(s for _, s in ref), np.uint8)
            wins, count = _windows(ref, k)
            row_of = set(MM.key_ints(keys))
            hit = [(int(offs[c]) + pos, c, pos, count[split] == 1) for c, ws in enumerate(wins) for pos, split, _ in ws if split in row_of]
            merged = KM.merge_intervals(iv)
            for s in range(S):
                mine = [(c, a, b) for q, c, a, b in merged if q in (s, ALL)]
                inside = lambda c, pos: any(c == c2 and a <= pos <= b for c2, a, b in mine)
                cells = np.array([x for x, c, pos, site in hit if site and inside(c, pos)], np.int64)
                near = np.zeros(len(refcat) + 1, np.int64)
                np.add.at(near, np.maximum(cells - half, 0), 1)
                np.add.at(near, np.minimum(cells + half, len(refcat) - 1) + 1, -1)
                near = np.cumsum(near[:-1]) > 0
                ok &= np.array_equal(after[s][~near], before[s][~near])                        # unchanged elsewhere, repeated windows included
                ok &= bool(((after[s][cells] == KM.GAP) | (after[s][cells] == refcat[cells])).all())
                was_snp = cells[(before[s][cells] != refcat[cells]) & (before[s][cells] != KM.GAP)]
                masked_snps += len(was_snp)
                kept_flank += int((after[s][cells] == refcat[cells]).sum())
                others = np.array([x for x, c, pos, site in hit if not (site and inside(c, pos))], np.int64)
                d = np.zeros(len(refcat) + 1, np.int64)
                np.add.at(d, np.maximum(others - half, 0), 1)
                np.add.at(d, np.minimum(others + half, len(refcat) - 1) + 1, -1)
                alone = np.cumsum(d[:-1]) == 0                                                  # positions no other hit window reaches
                ok &= bool((after[s][cells[alone[cells]]] == KM.GAP).all())
    assert masked_snps > 0 and kept_flank > 0
    return bool(ok)


# ---- (2) the oracle's `ska weed` for a BED interval; (3) its delete_samples for intervals over the whole reference
def _unique_world(k, S, seed, n=400, rc=True):
    """a reference without repeated windows and an array whose rows are exactly its windows' split k-mers, cells at random"""
    rng = np.random.default_rng(seed)
    while True:
        ref = [("c1", bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n))), ("c2", bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n // 2)))]
        wins, count = _windows(ref, k, rc)
        if max(count.values()) == 1:
            break
    splits = [w[1] for ws in wins for w in ws]
    order = rng.permutation(len(splits))
    keys = np.array([(splits[j] & ((1 << 64) - 1), splits[j] >> 64) for j in order], KEY_DT)
    var = np.frombuffer(b"-ACGTN", np.uint8)[rng.integers(0, 6, size=(len(splits), S))]
    var[(var == KM.GAP).all(1), 0] = ord("A")                                                  # no row without a present cell
    return ref, keys, np.ascontiguousarray(var), [f"s{i}" for i in range(S)]


def _check_weed(mutant=None, tmp=None):
    ok = True
    for k, rc in ((9, True), (31, True), (41, True), (17, False)):
        half = (k - 1) // 2
        ref, keys, var, names = _unique_world(k, 4, seed=k, rc=rc)
        for c, a, b in ((0, 30, 31), (0, 100, 180), (1, half, half + 40), (1, len(ref[1][1]) - half - 30, len(ref[1][1]) - half - 1)):
            bed = f"{ref[c][0]}\t{a}\t{b + 1}\n".encode()
            iv = KM.read_bed(bed, [i for i, _ in ref], [len(s) for _, s in ref], mutant)
            res = KM.mask(keys, var, _counts(var), k, rc, ref, iv, mutant)
            path = os.path.join(tmp, f"weed_{k}_{c}_{a}.fa")
            with open(path, "wb") as f:
                f.write(b">w\n" + ref[c][1][a - half:b + half + 1] + b"\n")
            o = ora.Array.from_rows(k, rc, names, keys, var)
            o.weed(path, min_freq=0.0)
            okeys, ovar, ocounts = o.export()
            ok &= np.array_equal(okeys, res["keys"]) and np.array_equal(ovar, res["var"]) and np.array_equal(ocounts, res["counts"])
            ok &= int(res["info"]["rows_all_samples"]) == b - a + 1 and int(res["info"]["rows_emptied"]) == 0
    return bool(ok)


def _check_delete(mutant=None):
    ok, emptied = True, 0
    for k in (9, 31):
        keys, var, ref, _, _ = _map_world(k, "test_ref_two_chrom_repeats.fa")
        names = list(TM.SAMPLES)
        for gone in ((0,), (1, 4), (0, 1, 2, 3)):
            iv = [(s, c, 0, len(seq) - 1) for s in gone for c, (_, seq) in enumerate(ref)]
            res = KM.mask(keys, var, _counts(var), k, True, ref, iv, mutant)
            o = ora.Array.from_rows(k, True, names, keys, var)
            o.delete_samples([names[s] for s in gone])
            okeys, ovar, ocounts = o.export()
            wins, count = _windows(ref, k)
            site = {split for ws in wins for _, split, _ in ws if count[split] == 1}
            rest = [s for s in range(len(names)) if s not in gone]
            m_site = np.array([x in site for x in MM.key_ints(res["keys"])], bool)
            o_site = np.array([x in site for x in MM.key_ints(okeys)], bool)
            # at site rows: the oracle's rows, with the deleted samples' cells missing
            ok &= np.array_equal(res["keys"][m_site], okeys[o_site]) and np.array_equal(res["var"][m_site][:, rest], ovar[o_site])
            ok &= np.array_equal(res["counts"][m_site], ocounts[o_site]) and bool((res["var"][m_site][:, list(gone)] == KM.GAP).all())
            # rows that are no site keep their cells, the deleted samples' too, and their counts
            k_site = np.array([x in site for x in MM.key_ints(keys)], bool)
            ok &= np.array_equal(res["keys"][~m_site], keys[~k_site]) and np.array_equal(res["var"][~m_site], var[~k_site])
            ok &= np.array_equal(res["counts"][~m_site], _counts(var)[~k_site])
            emptied += int(res["info"]["rows_emptied"])
            ok &= int(res["info"]["rows_out"]) == int(res["info"]["rows_in"]) - int(res["info"]["rows_emptied"])
    assert emptied > 0
    return bool(ok)


# ---- (4) a hand-worked example at k = 9 on test_density_model's two chromosomes (c1: middles 4 .. 9 and 19 .. 80, 59 .. 62 repeated; c2: middles
# 4 .. 61, 52 .. 55 repeated; 85 and 66 letters; s2 holds N at c2:10 and '-' at c2:11 and c2:12, every other cell is present)
HAND_INTERVALS = [
    (0, 0, 76, 84),                                    # ends on c1's last position, past its last window (80): 5 sites
    (1, 0, 20, 25), (1, 0, 23, 30), (1, 0, 31, 33), (1, 0, 20, 25),      # overlapping, touching, given twice: c1 20 .. 33, 14 sites
    (2, 1, 10, 12),                                    # three sites, one present cell (the N)
    (0, 0, 57, 63),                                    # 59 .. 62 are repeated windows: 57, 58, 63
    (ALL, 1, 50, 56),                                  # 52 .. 55 are repeated windows: the rows of 50, 51, 56 go
    (1, 1, 49, 51),                                    # 50 and 51 are gone already: 49
    (0, 1, 11, 11), (1, 1, 11, 11),                    # with s2's '-' there, the row of c2:11 is left without a present cell
]
HAND_SAMPLES = [(9, 9), (16, 16), (3, 1)]
HAND_INFO = dict(sites=118, rows_in=122, rows_all_samples=3, rows_emptied=1, rows_out=118, n_intervals_merged=8)
HAND_SUMMARY = ("sample\tintervals\tinterval_bases\tsites_in_regions\tcells_masked\n"
                "s0\t3\t17\t9\t9\ns1\t3\t18\t16\t16\ns2\t1\t3\t3\t1\n"
                "all_samples_intervals\t1\nall_samples_bases\t7\nsites\t118\nrows_in\t122\nrows_all_samples\t3\nrows_emptied\t1\nrows_out\t118\n")


def _check_hand(mutant=None):
    keys, var = TM._hand_array()
    counts = _counts(var)
    res = KM.mask(keys, var, counts, 9, True, TM.HAND_REF, HAND_INTERVALS, mutant)
    ok = [tuple(int(x) for x in q) for q in res["samples"]] == HAND_SAMPLES
    ok &= {f: int(res["info"][f]) for f in KM.INFO_DT.names} == HAND_INFO
    ok &= KM.summary_text(res, TM.HAND_NAMES, HAND_INTERVALS) == HAND_SUMMARY
    # the counts of the rows that stay: 3 less the cells lost
    wins, count = _windows(TM.HAND_REF, 9)
    lost = {}
    for s, c, a, b in KM.merge_intervals(HAND_INTERVALS):
        for pos, split, _ in wins[c]:
            if s != ALL and a <= pos <= b and count[split] == 1:
                lost.setdefault(split, set()).add(s)
    for key, cells, n in zip(MM.key_ints(res["keys"]), res["var"], res["counts"]):
        ok &= int(n) == int(((cells != KM.GAP) & (cells != 0)).sum())
        ok &= all(cells[s] == KM.GAP for s in lost.get(key, ()))
    return bool(ok)


# ---- (5) the plain loops; (6) idempotence
def _check_loops(mutant=None):
    ok = True
    keys, var = TM._hand_array()
    worlds = [(keys, var, 9, TM.HAND_REF, HAND_INTERVALS)]
    k17, v17, ref17, _, _ = _map_world(17, "test_ref_two_chrom_repeats.fa")
    worlds.append((k17, v17, 17, ref17, _map_intervals(ref17, v17.shape[1])))
    for keys, var, k, ref, iv in worlds:
        counts = _counts(var)
        counts[::7] += 2                                        # (stored counts need not be the present cells)
        res = KM.mask(keys, var, counts, k, True, ref, iv, mutant)
        lk, lv, lc = KM.mask_loops(keys, var, counts, k, True, ref, iv)
        ok &= np.array_equal(lk, res["keys"]) and np.array_equal(lv, res["var"]) and np.array_equal(lc, res["counts"])
    return bool(ok)


def test_oracle_map():
    assert _check_map()


def test_oracle_weed_for_a_bed_interval(tmp_path):
    assert _check_weed(tmp=str(tmp_path))


def test_whole_reference_intervals_are_delete_samples_at_site_rows():
    assert _check_delete()


def test_hand_worked_example():
    assert _check_hand()
    assert KM.merge_intervals(HAND_INTERVALS) == [(0, 0, 57, 63), (0, 0, 76, 84), (0, 1, 11, 11), (1, 0, 20, 33), (1, 1, 11, 11), (1, 1, 49, 51), (2, 1, 10, 12),
                                                  (ALL, 1, 50, 56)]
    keys, var = TM._hand_array()
    none = KM.mask(keys, var, _counts(var), 9, True, TM.HAND_REF, [])
    assert np.array_equal(none["var"], var) and int(none["info"]["rows_out"]) == 122 and not none["samples"]["sites_in_regions"].any()
    everything = KM.mask(keys, var, _counts(var), 9, True, TM.HAND_REF, [(ALL, 0, 0, 84), (ALL, 1, 0, 65)])
    assert int(everything["info"]["rows_all_samples"]) == 118 and int(everything["info"]["rows_out"]) == 4      # the four repeated split k-mers stay
    empty = KM.mask(np.zeros(0, KEY_DT), np.zeros((0, 3), np.uint8), np.zeros(0, np.uint64), 9, True, TM.HAND_REF, HAND_INTERVALS)
    assert int(empty["info"]["sites"]) == 0 and int(empty["info"]["rows_out"]) == 0


def test_plain_loops():
    assert _check_loops()


def test_masking_twice_is_masking_once():
    keys, var = TM._hand_array()
    k17, v17, ref17, _, _ = _map_world(17, "test_ref_two_chrom_repeats.fa")
    for keys, var, k, ref, iv in ((keys, var, 9, TM.HAND_REF, HAND_INTERVALS), (k17, v17, 17, ref17, _map_intervals(ref17, v17.shape[1]))):
        once = KM.mask(keys, var, _counts(var), k, True, ref, iv)
        twice = KM.mask(once["keys"], once["var"], once["counts"], k, True, ref, iv)
        assert np.array_equal(twice["keys"], once["keys"]) and np.array_equal(twice["var"], once["var"]) and np.array_equal(twice["counts"], once["counts"])
        assert not twice["samples"]["cells_masked"].any() and int(twice["info"]["rows_all_samples"]) == 0 and int(twice["info"]["rows_emptied"]) == 0


@pytest.mark.parametrize("mutant", KM.MUTANTS)
def test_every_mutant_is_caught(mutant, tmp_path):
    results = {"weed": _check_weed(mutant, str(tmp_path)), "delete": _check_delete(mutant), "hand": _check_hand(mutant), "loops": _check_loops(mutant)}
    if all(results.values()):
        results["map"] = _check_map(mutant)
    assert not all(results.values()), (mutant, results)


# ---- the host's readers and its text, through ctypes (no device)
NAMES = ["s0", "s1", "a sample"]
IDS, LENS = ["c1", "c2"], [85, 66]
GOOD_REGIONS = (b"sample\tchromosome\tstart\tend\tlength\tsnps\n"
                b"s0\tc1\t21\t32\t12\t3\n"
                b"# a comment\r\n"
                b"\r\n"
                b"s1\tc1\t21\t43\t23\t5\r\n"
                b"a sample\tc2\t66\t66\n"
                b" \t \n"
                b"s0\tc2\t1\t1\textra\tcolumns\tare\tignored\n"
                b"s1\tc1\t85\t85")
GOOD_BED = (b"c1\t0\t85\n"
            b"#track name=phage\n"
            b"c2\t10\t11\tname\t0\t+\r\n"
            b"\n"
            b"c2\t65\t66\n"
            b"c1\t20\t40")
BAD_REGIONS = [(b"h\ns0\tc1\t5\n", 2, "fewer than four fields"), (b"h\n\ns9\tc1\t1\t2\n", 3, "unknown sample s9"), (b"h\ns0\tc3\t1\t2\n", 2, "unknown chromosome c3"),
               (b"h\ns0\tc1\t1\t2\ns0\tc1\tx\t2\n", 3, "no number"), (b"h\ns0\tc1\t1\t-2\n", 2, "no number"), (b"h\ns0\tc1\t1\t2.0\n", 2, "no number"),
               (b"h\ns0\tc1\t\t2\n", 2, "no number"), (b"h\ns0\tc1\t1\t99999999999\n", 2, "no number"), (b"h\ns0\tc1\t0\t2\n", 2, "start below 1"),
               (b"h\n#x\ns0\tc1\t5\t4\n", 3, "end before start"), (b"h\ns0\tc1\t80\t86\n", 2, "end past chromosome c1"), (b"h\ns0\tc2\t1\t67\r\n", 2, "end past chromosome c2"),
               (b"h\nS0\tc1\t1\t2\n", 2, "unknown sample S0"), (b"h\ns0 \tc1\t1\t2\n", 2, "unknown sample s0 ")]
BAD_BED = [(b"c1\t5\n", 1, "fewer than three fields"), (b"c1\t1\t2\nc9\t1\t2\n", 2, "unknown chromosome c9"), (b"c1\tone\t2\n", 1, "no number"),
           (b"c1\t-1\t2\n", 1, "no number"), (b"\n\nc1\t5\t5\n", 3, "end not after start"), (b"c1\t6\t5\n", 1, "end not after start"),
           (b"c1\t0\t86\n", 1, "end past chromosome c1"), (b"c2\t0\t66\nc2\t0\t67\n", 2, "end past chromosome c2"), (b"c1 1 2\n", 1, "fewer than three fields")]


def _both(read_model, read_host, text):
    """the model's and the host's answer to one text: ("ok", intervals) or ("bad", line number, what)"""
    import skx_engine as E
    try:
        want = ("ok", [tuple(int(x) for x in q) for q in read_model(text)])
    except KM.BadLine as e:
        want = ("bad", e.line, e.what)
    try:
        got = ("ok", [tuple(int(x) for x in q) for q in read_host(text)])
    except E.EngineError as e:
        assert e.code == E.EINVAL, str(e)
        m = re.search(r"mask: (regions|bed) line (\d+): (.*)$", str(e))
        assert m, str(e)
        got = ("bad", int(m.group(2)), m.group(3))
    return want, got


def test_host_readers_equal_the_model():
    import skx_engine as E
    regions = (lambda t: KM.read_regions(t, NAMES, IDS, LENS), lambda t: E.mask_read_regions(t, NAMES, IDS, LENS))
    bed = (lambda t: KM.read_bed(t, IDS, LENS), lambda t: E.mask_read_bed(t, IDS, LENS))
    want, got = _both(*regions, GOOD_REGIONS)
    assert got == want == ("ok", [(0, 0, 20, 31), (1, 0, 20, 42), (2, 1, 65, 65), (0, 1, 0, 0), (1, 0, 84, 84)])
    want, got = _both(*bed, GOOD_BED)
    assert got == want == ("ok", [(ALL, 0, 0, 84), (ALL, 1, 10, 10), (ALL, 1, 65, 65), (ALL, 0, 20, 39)])
    for (rm, rh), good, bad in ((regions, GOOD_REGIONS, BAD_REGIONS), (bed, GOOD_BED, BAD_BED)):
        for text, line, what in bad:
            want, got = _both(rm, rh, text)
            assert want[0] == got[0] == "bad" and want[1] == got[1] == line and what in want[2] and got[2].startswith(want[2]), (text, want, got)
        outcomes = set()
        for n in range(len(good) + 1):                          # every truncation of a good file: the same intervals or the same line refused
            want, got = _both(rm, rh, good[:n])
            assert want[0] == got[0] and want[1] == got[1] and (want[0] == "ok" or got[2].startswith(want[2])), (n, want, got)
            outcomes.add(want[0] if want[0] == "ok" else want[2].split(" ")[0])
        assert len(outcomes) >= 3, outcomes
    for rm, rh in (regions, bed):                               # nothing, a header alone, comments alone
        for text in (b"", b"sample\tchromosome\tstart\tend\n" if rm is regions[0] else b"\n", b"# nothing\n\n"):
            assert _both(rm, rh, text) == (("ok", []), ("ok", []))
    assert E.MASK_INTERVAL_DT == KM.INTERVAL_DT and E.MASK_SAMPLE_DT == KM.SAMPLE_DT and E.MASK_INFO_DT == KM.INFO_DT and E.MASK_ALL_SAMPLES == ALL


def test_host_summary_equals_the_model():
    import skx_engine as E
    keys, var = TM._hand_array()
    res = KM.mask(keys, var, _counts(var), 9, True, TM.HAND_REF, HAND_INTERVALS)
    assert E.mask_text(res["samples"], res["info"], HAND_INTERVALS, TM.HAND_NAMES) == HAND_SUMMARY
    none = KM.mask(keys, var, _counts(var), 9, True, TM.HAND_REF, [])
    assert E.mask_text(none["samples"], none["info"], [], TM.HAND_NAMES) == KM.summary_text(none, TM.HAND_NAMES, [])
    long_names = ["n" * 700, "s1", "s2"]
    assert E.mask_text(res["samples"], res["info"], HAND_INTERVALS, long_names) == KM.summary_text(res, long_names, HAND_INTERVALS)
    for iv in ([(3, 0, 1, 2)], [(0, 0, 5, 4)]):
        with pytest.raises(E.EngineError) as ei:
            E.mask_text(res["samples"], res["info"], iv, TM.HAND_NAMES)
        assert ei.value.code == E.EINVAL and "skh_mask_text" in str(ei.value)


def test_reference_records():
    import skx_engine as E
    ids, lens = E.reference_records(os.path.join(INPUT, "test_ref_two_chrom.fa"))
    ref = TM._fasta("test_ref_two_chrom.fa")
    assert ids == [i for i, _ in ref] and lens.tolist() == [len(s) for _, s in ref]
