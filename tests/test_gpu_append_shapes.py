"""MergeSkaDict<u64>::append on the device (append_kernel<COUNT_ONLY, HI> in skx_append.hip) at its key-shape, split and fill edges.

The kernel has two forms (HI: rem = 2 (k - 1) - logQ >= 32 hash bits below the block bits), part bits for the A = 2^(logQ - logB) row blocks
that share a region, a persistent launch with start counters and reader meetings, 1 024-word chunks with a fill test on the last one, and
an overflow exit the host answers with a finer split.  The host picks logQ from the number of rows (append_pass: the coarsest split with
mean + 6 sigma + 32 <= 6 016 ranks, that is a mean of 5 537 rows a block at most; logQ >= max(logB, 2 (k - 1) - 50)) and logB from the longest
sample (region_layout: ceil(log2(ceil(length / 4 900)))), so every shape below is reached by sizes alone and ASSERTED from the pass's own
debug line -- a case that lands elsewhere fails, it is not relabelled.  Row counts stay 15 % and more away from the count at which logQ
would change (which is why the unrelated samples are 37 000 bases long: 39 000 x 2^n rows are 12 % under the next split's threshold), except
where the case IS the edge (blocks filled to their rank capacity).

Every case, bit for bit and three ways: the engine's array, the CPU oracle's (ora.Array.from_dicts) and the engine's through sorted
dictionaries (SKX_KNOBS=sorted_dicts: union + assemble) -- keys, cells, counts, sample_kmers, names, nkmers; then a filtered alignment straight
from the pieces of a fresh merge (plen / perm / nrank as `ska align` reads them) and an unfiltered export of a fresh merge.  No tolerances."""
import re

import numpy as np
import pytest
from conftest import set_knob, del_knob

import ora
from test_gpu_parity import as_map, build_both, oracle_dict, rand_records

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
LINE = re.compile(r"\[skx\] append: logQ=(\d+) \(x(\d+) per region\) cap=(\d+) slots=(\d+) rows~(\d+) -> (ok|overflow)")
MAX_MEAN = 5537                   # rows a block: the largest mean with mean + 6 sqrt(mean + 1) + 32 <= 6 016
L = 37_000                        # logB 3 (eight regions of 4 625 words); n unrelated samples: 0.835 of the rows at which logQ goes up


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def genome(rng, length):
    return ACGT[rng.integers(0, 4, size=length)]


def related(rng, length, n, snps, cut=2):
    anc = genome(rng, length)
    out = []
    for _ in range(n):
        s = anc.copy()
        pos = rng.integers(0, length, size=snps)
        s[pos] = ACGT[rng.integers(0, 4, size=snps)]
        b = s.tobytes()
        step = (length + cut - 1) // cut
        out.append([b[i:i + step] for i in range(0, length, step)])
    return out


def unrel(rng, length, n):
    return [[genome(rng, length).tobytes()] for _ in range(n)]


def identical(rng, length, n):
    b = genome(rng, length).tobytes()
    return [[b[:length // 2], b[length // 2:]] for _ in range(n)]


def append_lines(err):
    return [(int(q), int(a), int(c), int(s), int(r), how) for q, a, c, s, r, how in LINE.findall(err)]


def rows_of(arr):
    """an export in key order: (lo, hi, cells [rows, samples], counts) -- numpy throughout (a million rows through a dict take seconds)"""
    keys, var, counts = arr.export()
    o = np.lexsort((keys["lo"], keys["hi"]))
    return keys["lo"][o], keys["hi"][o], var[o], counts[o]


def same_rows(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def columns(aln):
    return sorted(zip(*aln.decode().splitlines()[1::2]))


def engine_merge(E, samples, k, rc, names):
    return E.DictSet.build([E.record_stream(r) for r in samples], k, rc).merge(names)


def merge_with_lines(E, capfd, samples, k, rc, names):
    capfd.readouterr()
    ga = engine_merge(E, samples, k, rc, names)
    lines = append_lines(capfd.readouterr().err)
    return ga, lines, E.default_context().merge_path()


def check_parity(E, samples, k, rc, ga, monkeypatch, sorted_too=True):
    """ga (a fresh merge) against the oracle and the sorted path; then the filtered alignment and the unfiltered export of fresh merges"""
    names = [f"s{i}" for i in range(len(samples))]
    oa = ora.Array.from_dicts([oracle_dict(r, k, rc) for r in samples], names)
    want = rows_of(oa)
    assert ga.names == oa.names and ga.nkmers == oa.nkmers
    got = rows_of(ga)
    assert same_rows(got, want)
    if len(want[0]) <= 50_000:
        assert as_map(*ga.export()) == as_map(*oa.export())
    assert list(ga.sample_kmers()) == [int(x) for x in (want[2] != ord("-")).sum(axis=0)]
    if sorted_too:
        set_knob(monkeypatch, "sorted_dicts", 1)
        gs = engine_merge(E, samples, k, rc, names)
        assert E.default_context().merge_path().startswith("sorted:")
        del_knob(monkeypatch, "sorted_dicts")
        assert gs.names == oa.names and gs.nkmers == oa.nkmers and same_rows(rows_of(gs), want)
        assert list(gs.sample_kmers()) == list(ga.sample_kmers())
    # the kept rows straight from the pieces (rank bound from plen, pieces_stats_kernel, pieces_rows_kernel<kept>)
    g = engine_merge(E, samples, k, rc, names).align(filter_type=E.FILTER_NO_CONST, min_freq=0.9)
    assert same_rows(rows_of(engine_merge(E, samples, k, rc, names)), want)          # pieces_rows_kernel<all> first on a fresh merge
    assert columns(g) == columns(oa.align(filter_type=ora.FILTER_NO_CONST, min_freq=0.9))      # (last: the oracle filters in place)
    return want


def check_shape(E, capfd, monkeypatch, samples, k, rc, logQ, A, rem, sorted_too=True):
    """one merge with the shape asserted from the pass's debug line, then check_parity"""
    monkeypatch.setenv("SKX_DEBUG", "1")
    names = [f"s{i}" for i in range(len(samples))]
    ga, lines, path = merge_with_lines(E, capfd, samples, k, rc, names)
    with capfd.disabled():
        print(f"\n    k={k} rc={int(rc)} S={len(samples)} want logQ={logQ} A={A} rem={rem} {'HI' if rem >= 32 else '!HI'}: {lines} path={path}", flush=True)
    assert path == "append64"
    assert len(lines) == 1 and lines[0][5] == "ok"
    got_logQ, got_A, cap, slots, rows, _ = lines[0]
    assert (got_logQ, got_A) == (logQ, A)
    assert 2 * (k - 1) - got_logQ == rem                                  # and with it the kernel's form: HI = rem >= 32
    assert cap % 128 == 0 and cap <= 6016 and slots <= 8192
    check_parity(E, samples, k, rc, ga, monkeypatch, sorted_too)
    return lines[0]


# id: (k, rc, samples(rng), logQ, A, rem)
SHAPES = {
    # ---- the HI / !HI seam, rem = 0, a single block
    "k17_hi_lower_edge_lowb0_one_block": (17, True, lambda r: related(r, 4000, 5, 3), 0, 1, 32),
    "k17_lo_upper_edge": (17, True, lambda r: related(r, 9000, 5, 3), 1, 1, 31),
    "k19_seam_xmap_hi": (19, True, lambda r: related(r, 60_000, 5, 20), 4, 1, 32),
    "k19_seam_xmap_lo": (19, True, lambda r: related(r, 120_000, 5, 20), 5, 1, 31),
    # (lowb = 18 in a single block would be k = 26, which no dictionary takes -- k is odd: the two shapes next to it)
    "k25_lowb16_one_block": (25, True, lambda r: related(r, 4000, 5, 3), 0, 1, 48),
    "k27_lowb18_four_blocks_one_region": (27, True, lambda r: related(r, 4000, 5, 3), 2, 4, 50),
    "k5_rem0_one_key_per_block": (5, False, lambda r: unrel(r, 700_000, 2), 8, 1, 0),
    "k7_short_hash": (7, True, lambda r: related(r, 30_000, 3, 20), 3, 1, 9),
    "k9_short_hash": (9, True, lambda r: related(r, 30_000, 3, 20), 3, 1, 13),
    # ---- part bits, start counters, reader meetings
    "k21_ladder_A2": (21, True, lambda r: unrel(r, L, 2), 4, 2, 36),
    "k21_ladder_A4": (21, True, lambda r: unrel(r, L, 4), 5, 4, 35),
    "k21_ladder_A8": (21, True, lambda r: unrel(r, L, 8), 6, 8, 34),
    "k21_ladder_A16": (21, True, lambda r: unrel(r, L, 16), 7, 16, 33),
    "k21_ladder_A32": (21, True, lambda r: unrel(r, L, 32), 8, 32, 32),
    "k23_lowb7_A4": (23, True, lambda r: unrel(r, L, 4), 5, 4, 39),
    "k27_lowb15_A4": (27, True, lambda r: unrel(r, L, 4), 5, 4, 47),
    "k29_lowb18_A8": (29, True, lambda r: unrel(r, L, 4), 6, 8, 50),
    "k15_lo_keep_test_A2": (15, True, lambda r: unrel(r, L, 2), 4, 2, 24),
    "k15_lo_keep_test_A4": (15, True, lambda r: unrel(r, L, 4), 5, 4, 23),
    "k21_resync_280_samples": (21, True, lambda r: related(r, L, 280, 5), 4, 2, 36),
    "k15_resync_280_samples": (15, True, lambda r: related(r, L, 280, 5), 4, 2, 24),
    # ---- full blocks, rounds, wave counts
    "k25_blocks_at_rank_capacity": (25, True, lambda r: unrel(r, 350_000, 2), 7, 1, 41),
    "k21_two_rounds_lo": (21, True, lambda r: related(r, 1_300_000, 3, 40), 9, 1, 31),
    **{f"k21_S{s}": (21, True, (lambda r, s=s: related(r, 20_000, s, 5)), 3, 1, 37) for s in (1, 2, 15, 16, 17, 33)},
    **{f"k{k}_identical_{s}": (k, True, (lambda r, s=s: identical(r, 30_000, s)), 3, 1, 2 * (k - 1) - 3) for k in (21, 15) for s in (16, 32, 64)},
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_append_shape(E, case, capfd, monkeypatch):
    k, rc, make, logQ, A, rem = SHAPES[case]
    samples = make(np.random.default_rng(sum(case.encode()) * 1000 + k))
    _, _, cap, slots, _, _ = check_shape(E, capfd, monkeypatch, samples, k, rc, logQ, A, rem)
    if case == "k25_blocks_at_rank_capacity":
        assert (cap, slots) == (6016, 8192)
    if case.endswith("short_hash"):
        assert cap < 6016 and slots < 8192
    if case == "k21_two_rounds_lo":                                       # one workgroup a CU: 512 row blocks take two rounds
        import torch
        assert torch.cuda.get_device_properties(0).multi_processor_count * 2 == 1 << logQ


def test_append_k5_canonical_keys_leave_half_the_regions_empty(E, capfd, monkeypatch):
    """k = 5 with rc: the 256 regions are the 256 hash values and canonical keys use about half of them, so the used ones hold twice the mean
    and overflow their fixed capacity -- the batch is extracted again and sorted.  Kept as a parity case, with the path the debug output names."""
    monkeypatch.setenv("SKX_DEBUG", "1")
    samples = unrel(np.random.default_rng(55), 700_000, 2)
    capfd.readouterr()
    ga, oa = build_both(E, samples, 5, True)
    err = capfd.readouterr().err
    path = E.default_context().merge_path()
    with capfd.disabled():
        print(f"\n    k=5 rc=1: {append_lines(err)} path={path}", flush=True)
    assert path.startswith("sorted: the dictionaries are sorted") and "[skx] merge: sorted: the dictionaries are sorted" in err
    assert ga.names == oa.names and ga.nkmers == oa.nkmers and same_rows(rows_of(ga), rows_of(oa))
    assert as_map(*ga.export()) == as_map(*oa.export())


FILLS = [1, 2, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4096]


@pytest.mark.parametrize("k,rem", [(21, 38), (15, 26)])
def test_append_region_fills_around_the_chunk(E, k, rem, capfd, monkeypatch):
    """logB = 0: every sample is its region 0, read in chunks of 1 024 words -- fills of one word, of n x 1 024 exactly (no partial chunk: no
    fill test at all), one more and one less, and around the 128 words of one load.  One clean record of w + k - 1 bases has w windows (w = 1:
    k bases and an N -- a record that ENDS in a clean run of exactly k gives nothing, split_kmer.rs:89); the samples share nothing, so the
    oracle's count of a sample is its fill (asserted: a seed that repeated a split k-mer would not hit n x 1 024).
    Together 13 699 rows: four row blocks reading the one region (A = 4, no XCD map)."""
    rng = np.random.default_rng(2100 + k)
    samples = [[genome(rng, w + k - 1).tobytes() + (b"N" if w == 1 else b"")] for w in FILLS]
    assert [len(oracle_dict(r, k, True)) for r in samples] == FILLS
    check_shape(E, capfd, monkeypatch, samples, k, True, 2, 4, rem)


@pytest.mark.parametrize("k,rem", [(21, 37), (15, 25)])
def test_append_empty_regions_and_many_short_records(E, k, rem, capfd, monkeypatch):
    """logB = 3 beside ordinary samples: a sample of one record of k + 1 bases (two words: six regions and more have their one, empty, chunk) and
    a sample cut into 60 records of about 650 bases (a window short at every cut)."""
    rng = np.random.default_rng(3100 + k)
    n = 35_000                                                            # (logB 3 still; with the extras below 17 % under 8 x 5 537 rows)
    samples = related(rng, n, 4, 10)
    whole = b"".join(samples[3])
    cuts = sorted(int(x) for x in rng.choice(np.arange(200, n - 200), size=59, replace=False))
    samples[3] = [whole[a:b] for a, b in zip([0] + cuts, cuts + [n])]
    assert len(samples[3]) == 60
    samples.append([whole[5000:5000 + k + 1]])
    assert len(oracle_dict(samples[4], k, True)) == 2
    samples.append(samples[0][:1] + rand_records(rng, 2, 400))            # a sample that holds part of the rows only
    check_shape(E, capfd, monkeypatch, samples, k, True, 3, 1, rem)


@pytest.mark.parametrize("k,logQ,A,rem", [(21, 3, 1, 37), (31, 10, 128, 50)])
def test_append_repeats_inside_the_capacity(E, k, logQ, A, rem, capfd, monkeypatch):
    """Samples that are one repeat (every word of a load in one row block: the queue of kept words takes 127 + 128), ambiguity where the copies
    differ, palindromic middles -- small enough for the regions' fixed capacity, so the batch stays on the append path (asserted)."""
    rng = np.random.default_rng(7 + k)
    samples = related(rng, 30_000, 20, 15, cut=3)
    unit = genome(rng, k + 9).tobytes()
    samples += [[b"A" * 700, unit * 8], [b"AT" * 300 + samples[0][0][:3000]], [b"ACGT" * 150]]
    var = bytearray(unit * 50)
    for p in range(k // 2, len(var), len(unit)):
        var[p] = b"ACGT"[(p // len(unit)) % 4]                           # the same flanks around different middle bases: folded into ambiguity codes
    samples.append([bytes(var)])
    check_shape(E, capfd, monkeypatch, samples, k, True, logQ, A, rem)


# ---- the retry loop of append_pass: SKX_KNOBS=append_coarse=N starts N steps coarser than the split the probe asks for, so that row blocks
# overflow (CTL_FAIL: ranks clamped, nothing stored beyond cap) and the host comes back one step finer, four attempts in all
@pytest.mark.parametrize("k", [21, 15])
@pytest.mark.parametrize("coarse,n,natural", [(1, 4, 5), (2, 8, 6)])
def test_append_overflow_is_retried_one_split_finer(E, k, coarse, n, natural, capfd, monkeypatch):
    monkeypatch.setenv("SKX_DEBUG", "1")
    samples = unrel(np.random.default_rng(4100 + k + n), L, n)
    names = [f"s{i}" for i in range(n)]
    g0, lines0, path0 = merge_with_lines(E, capfd, samples, k, True, names)
    assert path0 == "append64" and [(x[0], x[5]) for x in lines0] == [(natural, "ok")]
    set_knob(monkeypatch, "append_coarse", coarse)
    g1, lines1, path1 = merge_with_lines(E, capfd, samples, k, True, names)
    del_knob(monkeypatch, "append_coarse")
    with capfd.disabled():
        print(f"\n    k={k} S={n} append_coarse={coarse}: {lines1} path={path1}", flush=True)
    assert path1 == "append64"
    assert [(x[0], x[5]) for x in lines1] == [(natural - coarse + i, "overflow") for i in range(coarse)] + [(natural, "ok")]
    assert lines1[-1] == lines0[0]
    want = check_parity(E, samples, k, True, g1, monkeypatch, sorted_too=False)
    assert same_rows(rows_of(g0), want)                                   # keys and cells; the rank order inside the pieces is not compared


@pytest.mark.parametrize("k", [21, 15])
def test_append_that_keeps_overflowing_takes_the_sorted_path(E, k, capfd, monkeypatch):
    monkeypatch.setenv("SKX_DEBUG", "1")
    samples = unrel(np.random.default_rng(5100 + k), L, 32)
    names = [f"s{i}" for i in range(32)]
    set_knob(monkeypatch, "append_coarse", 5)
    ga, lines, path = merge_with_lines(E, capfd, samples, k, True, names)
    del_knob(monkeypatch, "append_coarse")
    with capfd.disabled():
        print(f"\n    k={k} S=32 append_coarse=5: {lines} path={path}", flush=True)
    assert [(x[0], x[5]) for x in lines] == [(3 + i, "overflow") for i in range(4)]
    assert path.startswith("sorted: row blocks kept overflowing")
    oa = ora.Array.from_dicts([oracle_dict(r, k, True) for r in samples], names)
    assert ga.names == oa.names and ga.nkmers == oa.nkmers and same_rows(rows_of(ga), rows_of(oa))
    assert list(ga.sample_kmers()) == [int(x) for x in (oa.export()[1] != ord("-")).sum(axis=0)]
