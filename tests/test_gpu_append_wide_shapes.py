"""MergeSkaDict<u128>::append on the device (append_wide_kernel<COUNT_ONLY, QS, PD> in skx_append_wide.inc, k = 33..63) at its shift, split,
fill and table edges.

The kernel has five forms, chosen from rem = 2 (k - 1) - logQ (launch_append_wide_t: QS = (122 - rem) >> 5 picks the dword pairs of the key
shift, PD = (rem + 4) >> 5 the dword that holds the part bits, which start at bit pb = (rem + 4) & 31 of it and straddle into the next dword
where pb + log2(A) > 32), a table of 16-byte entries {E_lo, E_hi} claimed by a 64-bit CAS on E_hi and published by a store of E_lo, a fill test
written out once per load of a 512-word chunk, a persistent launch with rounds and reader meetings, and an overflow exit the host answers
with a finer split.  The host's rules, restated here from the code, give every shape below by sizes alone:
  * region_layout (skx_dictset.cpp, `per_region = wide ? 3200 : 4900` and the `need` / `logB` lines under it): logB = ceil(log2(ceil(longest
    sample in bytes / 3 200))) for the lengths used here;
  * append_pass (skx_merge.cpp, `min_logQ = max(logB, bits - 113)` and the `while (... ranks_need(...) > append_max_cap(wide)) logQ++` loop):
    the coarsest split whose blocks hold mean + 6 sqrt(mean + 1 + relvar mean^2) + 32 ranks (ranks_need) within APPEND_WIDE_MAX_CAP = 3 072.  With
    relvar = 0 that is a mean of 2 726 rows a block at most (2 726 + 6 sqrt(2 727) + 32 = 3 071.3; 2 727 gives 3 072.4) -- the only derived number
    of this file; the sketch's relvar (estimate_rows) adds about one rank at these sizes;
  * append_split: A = 2^(logQ - logB) row blocks read every region, cap = the ranks rounded up to 128, slots = the power of two that is a
    third above cap, 4 096 at most.
Every shape is ASSERTED from the pass's own SKX_DEBUG line (logQ, A, rem and from rem the triple QS, PD, pb; cap % 128 == 0, cap <= 3 072, slots
<= 4 096, one line, `ok`, path append128): a case that lands elsewhere fails and gets new sizes, it is not relabelled.  Row counts stay 15 % away
from the count at which logQ would change except where the case is the edge or its inputs are fixed (noted at the case).

Every case, bit for bit (check_parity of test_gpu_append_shapes.py): the engine's array against the CPU oracle's and against the engine's through
sorted dictionaries (SKX_KNOBS=sorted_dicts) -- keys, cells, counts, sample_kmers, names, nkmers; then a filtered alignment from the pieces of a
fresh merge and an unfiltered export of a fresh merge.  No tolerances, no measured times.

The built keys of the last part: H (hmix_w / hunmix_w in skx_device.h, three rounds on k - 1-bit halves, constants in make_wide_hash) is a
bijection with a known inverse, restated here in Python integers and held against the engine (the rows of a .skf it writes stand in the order of H).  Hash
values are chosen, inverted and written as records of their own.  That works with rc = False only, where every 2 (k - 1)-bit value is a split
k-mer; a canonical key would have to be searched for.  A record is upper arm, a middle base, lower arm and an N: k clean bases followed by an
N are exactly one window (a record that ENDS in a clean run of exactly k gives nothing, and a base of padding on either side would add two
windows more), and the oracle's dictionary of every record is asserted to hold exactly the intended key, which pins the base code and the arm
order without assuming them."""
import re

import numpy as np
import pytest
from conftest import set_knob, del_knob

import ora
from test_gpu_parity import as_map, build_both, oracle_dict, rand_records
from test_gpu_append_shapes import check_parity, engine_merge, genome, identical, related, rows_of, same_rows, unrel

pytestmark = pytest.mark.gpu

LINE = re.compile(r"\[skx\] append \(128-bit keys\): logQ=(\d+) \(x(\d+) per region\) cap=(\d+) slots=(\d+) rows~(\d+) -> (ok|overflow) \[sized by ")
MAX_MEAN = 2726                   # rows a block: the largest mean with mean + 6 sqrt(mean + 1) + 32 <= 3 072 (ranks_need, APPEND_WIDE_MAX_CAP)
L = 18_500                        # logB 3 (eight regions); n = 2^m unrelated samples: 2 308 rows a block, 0.847 of MAX_MEAN


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def wide_lines(err):
    return [(int(q), int(a), int(c), int(s), int(r), how) for q, a, c, s, r, how in LINE.findall(err)]


def form_of(k, logQ):
    """(rem, QS, PD, pb) as launch_append_wide_t and the kernel derive them"""
    rem = 2 * (k - 1) - logQ
    return rem, (122 - rem) >> 5, (rem + 4) >> 5, (rem + 4) & 31


def merge_with_lines(E, capfd, samples, k, rc, names):
    capfd.readouterr()
    ga = engine_merge(E, samples, k, rc, names)
    lines = wide_lines(capfd.readouterr().err)
    return ga, lines, E.default_context().merge_path()


def check_shape(E, capfd, monkeypatch, samples, k, rc, logQ, A, rem, QS, PD, pb, sorted_too=True):
    """one merge with the shape asserted from the pass's debug line, then check_parity"""
    monkeypatch.setenv("SKX_DEBUG", "1")
    names = [f"s{i}" for i in range(len(samples))]
    ga, lines, path = merge_with_lines(E, capfd, samples, k, rc, names)
    got = (lines[0][0], lines[0][1]) + form_of(k, lines[0][0]) if lines else None
    with capfd.disabled():
        print(f"\n    k={k} rc={int(rc)} S={len(samples)} want (logQ, A, rem, QS, PD, pb)={(logQ, A, rem, QS, PD, pb)} got {got}: {lines} path={path}", flush=True)
    assert path == "append128"
    assert len(lines) == 1 and lines[0][5] == "ok"
    got_logQ, got_A, cap, slots, rows, _ = lines[0]
    assert (got_logQ, got_A) == (logQ, A)
    assert form_of(k, got_logQ) == (rem, QS, PD, pb)                      # the kernel's instantiation and where the part bits start
    assert (QS, PD) in ((0, 3), (0, 2), (1, 2), (1, 1), (2, 1))
    assert cap % 128 == 0 and cap <= 3072 and slots <= 4096
    check_parity(E, samples, k, rc, ga, monkeypatch, sorted_too)
    return lines[0]


# ---- 1. every instantiation and both seams (rem 59 | 60: PD 1 | 2 and QS 1; rem 58 | 59: QS 2 | 1; rem 90 | 91: QS 1 | 0; rem 91 | 92: PD 2 | 3),
# with one reader a region (A = 1: the part mask is 0) and with several; the ladder A = 2..32 at k = 33, where the part bits start a dword at
# A = 2 (pb = 0) and straddle two dwords from A = 4 on (pb + log2(A) = 33); the straddle PD 2 -> 3 at rem 91; the clamp rem = 113 of k = 63,
# whose 2^11 row blocks are nearly or wholly empty -- once with 256 readers a region and once (110 000 bases: logB 6, A = 32) as the persistent
# launch, one workgroup a CU and eight rounds.
# id: (k, rc, samples(rng), logQ, A, rem, QS, PD, pb)
SHAPES = {
    "k33_ladder_A2_pb0": (33, True, lambda r: unrel(r, L, 2), 4, 2, 60, 1, 2, 0),
    "k33_ladder_A4_straddle": (33, True, lambda r: unrel(r, L, 4), 5, 4, 59, 1, 1, 31),
    "k33_ladder_A8_straddle": (33, True, lambda r: unrel(r, L, 8), 6, 8, 58, 2, 1, 30),
    "k33_ladder_A16_straddle": (33, True, lambda r: unrel(r, L, 16), 7, 16, 57, 2, 1, 29),
    "k33_ladder_A32_straddle": (33, True, lambda r: unrel(r, L, 32), 8, 32, 56, 2, 1, 28),
    "k49_rem92_A2_pb0": (49, True, lambda r: unrel(r, L, 2), 4, 2, 92, 0, 3, 0),
    "k49_rem91_A4_straddle": (49, True, lambda r: unrel(r, L, 4), 5, 4, 91, 0, 2, 31),
    "k47_rem90_A4_lowb0": (47, True, lambda r: unrel(r, 2300, 4), 2, 4, 90, 1, 2, 30),
    # one reader a region at the same rem (related samples: rows ~ length + 15 effective SNPs x k a sample)
    "k33_rem60_one_reader": (33, True, lambda r: related(r, 32_000, 5, 20), 4, 1, 60, 1, 2, 0),
    "k33_rem59_one_reader": (33, True, lambda r: related(r, 64_000, 5, 20), 5, 1, 59, 1, 1, 31),
    "k33_rem58_one_reader": (33, True, lambda r: related(r, 128_000, 5, 20), 6, 1, 58, 2, 1, 30),
    "k49_rem92_one_reader": (49, False, lambda r: related(r, 32_000, 5, 20), 4, 1, 92, 0, 3, 0),
    "k49_rem91_one_reader": (49, False, lambda r: related(r, 64_000, 5, 20), 5, 1, 91, 0, 2, 31),
    "k47_rem90_one_reader": (47, True, lambda r: related(r, 7000, 5, 5), 2, 1, 90, 1, 2, 30),
    # the clamp
    "k63_rem113_A256": (63, True, lambda r: unrel(r, L, 4), 11, 256, 113, 0, 3, 21),
    "k63_rem113_persistent_rounds": (63, True, lambda r: unrel(r, 110_000, 2), 11, 32, 113, 0, 3, 21),
    # ---- 3. blocks at rank capacity: 2 x 169 600 rows in 2^7 blocks are a mean of 2 650, 0.97 of MAX_MEAN (the case IS the edge)
    "k33_blocks_at_rank_capacity": (33, True, lambda r: unrel(r, 169_632, 2), 7, 2, 57, 2, 1, 29),
    "k41_blocks_at_rank_capacity": (41, True, lambda r: unrel(r, 169_640, 2), 7, 2, 73, 1, 2, 13),
    # ---- 4. waves and samples: fewer samples than waves, a wave's second sample, a third; 20 000 bases are 2 496 rows a block for one sample
    # (0.92 of MAX_MEAN: the length is fixed), and with 15 effective SNPs a sample 15 samples and more have 1.25 x the rows of a 2^3 split and
    # at most 0.85 of a 2^4 one: two readers a region, started and met together
    **{f"k33_S{s}": (33, True, (lambda r, s=s: related(r, 20_000, s, 5)), 3, 1, 61, 1, 2, 1) for s in (1, 2)},
    **{f"k33_S{s}": (33, True, (lambda r, s=s: related(r, 20_000, s, 20)), 4, 2, 60, 1, 2, 0) for s in (15, 16, 17, 33)},
    # every wave brings the same keys at once: all inserts race, all later look-ups hit
    **{f"k33_identical_{s}": (33, True, (lambda r, s=s: identical(r, L, s)), 3, 1, 61, 1, 2, 1) for s in (16, 32, 64)},
    # the meeting at a wave's 16th sample (S >= 272), four readers a region: 18 468 + 280 x 3.75 x 33 = 53 000 rows, 0.61 of a 2^5 split
    "k33_resync_280_samples": (33, True, lambda r: related(r, L, 280, 5), 5, 4, 59, 1, 1, 31),
}
STRADDLES = {c for c in SHAPES if c.endswith("_straddle")}


@pytest.mark.parametrize("case", list(SHAPES))
def test_wide_append_shape(E, case, capfd, monkeypatch):
    k, rc, make, logQ, A, rem, QS, PD, pb = SHAPES[case]
    if case in STRADDLES:
        assert A >= 4 and pb + A.bit_length() - 1 > 32                    # the part bits reach into the next dword
    samples = make(np.random.default_rng(sum(case.encode()) * 1000 + k))
    _, _, cap, slots, _, _ = check_shape(E, capfd, monkeypatch, samples, k, rc, logQ, A, rem, QS, PD, pb)
    if case.endswith("blocks_at_rank_capacity"):
        assert (cap, slots) == (3072, 4096)
    if case.startswith("k63_rem113"):
        import torch
        assert (1 << logQ) > torch.cuda.get_device_properties(0).multi_processor_count


def test_the_cases_visit_every_instantiation_and_both_seams():
    """host arithmetic only, so that a resized case cannot silently drop a form"""
    forms = {(c[6], c[7]) for c in SHAPES.values()}
    assert forms == {(0, 3), (0, 2), (1, 2), (1, 1), (2, 1)}
    for rem in (58, 59, 60, 90, 91, 92, 113):
        assert {c[4] == 1 for c in SHAPES.values() if c[5] == rem} >= ({True, False} if rem != 113 else {False}), rem
    assert {c[4] for n, c in SHAPES.items() if "ladder" in n} == {2, 4, 8, 16, 32}
    assert any(c[5] == 91 and c[4] >= 4 for n, c in SHAPES.items() if n in STRADDLES)
    for k, _, _, logQ, _, rem, QS, PD, pb in SHAPES.values():
        assert form_of(k, logQ) == (rem, QS, PD, pb)


# ---- 2. region fills around the chunk and around every load of it
FILLS = sorted({1, 2} | {64 * r + 1 for r in range(8)} | {64 * r + 64 for r in range(8)} | {511, 512, 513, 1023, 1024, 1025, 2048})


@pytest.mark.parametrize("k,rem,QS,PD,pb", [(33, 62, 1, 2, 2), (47, 90, 1, 2, 30)])
def test_wide_append_region_fills_around_the_chunk_and_its_loads(E, k, rem, QS, PD, pb, capfd, monkeypatch):
    """logB = 0: every sample is its region 0, read in chunks of 512 words, eight loads of 64 -- fills of one and two words, for every load r of
    a chunk the fills 64 r + 1 (its first lane alone) and 64 r + 64 (all of it, nothing of the next: the test `fill_left - 64 r > lane` of each of
    the eight assembly texts at both ends), n x 512 exactly (full_chunk: no fill test at all), one more and one less.  One clean record of
    w + k - 1 bases has w windows (w = 1: k bases and an N); the samples share nothing, so the oracle's count of a sample is its fill (asserted).
    Together 10 250 rows: four row blocks reading the one region (A = 4), 2 562 rows each -- 0.94 of MAX_MEAN: the fills are fixed."""
    assert sum(FILLS) == 10250 and sum(FILLS) < 4 * MAX_MEAN
    rng = np.random.default_rng(2100 + k)
    samples = [[genome(rng, w + k - 1).tobytes() + (b"N" if w == 1 else b"")] for w in FILLS]
    assert [len(oracle_dict(r, k, True)) for r in samples] == FILLS
    check_shape(E, capfd, monkeypatch, samples, k, True, 2, 4, rem, QS, PD, pb)


@pytest.mark.parametrize("k,rem,QS,PD,pb", [(33, 61, 1, 2, 1), (47, 89, 1, 2, 29)])
def test_wide_append_empty_regions_and_many_short_records(E, k, rem, QS, PD, pb, capfd, monkeypatch):
    """logB = 3 beside ordinary samples: a sample of one record of k + 1 bases (two words: six regions and more have their one, empty, chunk) and
    a sample cut into 60 short records (a window short at every cut).  14 000 bases + 4 x 7.5 x k + the extras: at most 0.77 of 8 x MAX_MEAN."""
    rng = np.random.default_rng(3100 + k)
    n = 14_000
    samples = related(rng, n, 4, 10)
    whole = b"".join(samples[3])
    cuts = sorted(int(x) for x in rng.choice(np.arange(200, n - 200), size=59, replace=False))
    samples[3] = [whole[a:b] for a, b in zip([0] + cuts, cuts + [n])]
    assert len(samples[3]) == 60
    samples.append([whole[5000:5000 + k + 1]])
    assert len(oracle_dict(samples[4], k, True)) == 2
    samples.append(samples[0][:1] + rand_records(rng, 2, 400))            # a sample that holds part of the rows only
    check_shape(E, capfd, monkeypatch, samples, k, True, 3, 1, rem, QS, PD, pb)


@pytest.mark.parametrize("k,logQ,A", [(33, 4, 1), (41, 4, 1), (63, 11, 128)])
def test_wide_append_repeats_ambiguity_and_palindromes(E, k, logQ, A, capfd, monkeypatch):
    """Samples that are one repeat (every word of a load in one row block: the queue of kept words takes 127 + 64), ambiguity where the copies
    differ, palindromic middles -- small enough for the regions' fixed capacity, so the batch stays on the append path (asserted).  26 000 bases
    (logB 4) + 20 x 11.25 x k + the extras: 0.77 (k = 33) and 0.81 (k = 41) of 16 x MAX_MEAN."""
    rng = np.random.default_rng(7 + k)
    samples = related(rng, 26_000, 20, 15, cut=3)
    unit = genome(rng, k + 9).tobytes()
    samples += [[b"A" * 700, unit * 8], [b"AT" * 300 + samples[0][0][:3000]], [b"ACGT" * 150]]
    var = bytearray(unit * 50)
    for p in range(k // 2, len(var), len(unit)):
        var[p] = b"ACGT"[(p // len(unit)) % 4]                           # the same flanks around different middle bases: folded into ambiguity codes
    samples.append([bytes(var)])
    check_shape(E, capfd, monkeypatch, samples, k, True, logQ, A, *form_of(k, logQ))


# ---- 3. the retry loop of append_pass for wide keys: SKX_KNOBS=append_coarse=N starts N steps coarser, so that row blocks overflow (CTL_FAIL in
# slow_batch: ranks clamped, rank1 > cap dropped, total > stride) and the host comes back one step finer, four attempts in all
@pytest.mark.parametrize("k", [33, 41])
@pytest.mark.parametrize("coarse,n,natural", [(1, 4, 5), (2, 8, 6)])
def test_wide_append_overflow_is_retried_one_split_finer(E, k, coarse, n, natural, capfd, monkeypatch):
    monkeypatch.setenv("SKX_DEBUG", "1")
    samples = unrel(np.random.default_rng(4100 + k + n), L, n)
    names = [f"s{i}" for i in range(n)]
    g0, lines0, path0 = merge_with_lines(E, capfd, samples, k, True, names)
    assert path0 == "append128" and [(x[0], x[5]) for x in lines0] == [(natural, "ok")]
    assert natural - coarse >= 3                                          # logB
    set_knob(monkeypatch, "append_coarse", coarse)
    g1, lines1, path1 = merge_with_lines(E, capfd, samples, k, True, names)
    del_knob(monkeypatch, "append_coarse")
    with capfd.disabled():
        print(f"\n    k={k} S={n} append_coarse={coarse}: {lines1} path={path1}", flush=True)
    assert path1 == "append128"
    assert [(x[0], x[5]) for x in lines1] == [(natural - coarse + i, "overflow") for i in range(coarse)] + [(natural, "ok")]
    assert lines1[-1] == lines0[0]
    want = check_parity(E, samples, k, True, g1, monkeypatch, sorted_too=False)
    assert same_rows(rows_of(g0), want)                                   # keys and cells; the rank order inside the pieces is not compared


@pytest.mark.parametrize("k", [33, 41])
def test_wide_append_that_keeps_overflowing_takes_the_sorted_path(E, k, capfd, monkeypatch):
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


# ---- 5. built keys: what no genome gives
M64 = (1 << 64) - 1
HASH_C = (0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93, 0xC2B2AE3D27D4EB4F)   # make_wide_hash
CODE = b"ACTG"                                                           # base codes 0..3 (asserted through the oracle for every record)


def _round(v, c, hb):
    return ((v * c) & M64) >> (64 - hb)                                   # hround64


def hmix_w(x, k):
    hb = k - 1
    left, right = x >> hb, x & ((1 << hb) - 1)
    left ^= _round(right, HASH_C[0], hb)
    right ^= _round(left, HASH_C[1], hb)
    left ^= _round(right, HASH_C[2], hb)
    return (left << hb) | right


def hunmix_w(x, k):
    hb = k - 1
    left, right = x >> hb, x & ((1 << hb) - 1)
    left ^= _round(right, HASH_C[2], hb)
    right ^= _round(left, HASH_C[1], hb)
    left ^= _round(right, HASH_C[0], hb)
    return (left << hb) | right


def key_record(key, k, mid):
    """the record whose one window is the split k-mer `key` (upper arm << (k - 1) | lower arm) around the middle base `mid`"""
    h = (k - 1) // 2
    arm = lambda v: bytes(CODE[(v >> (2 * (h - 1 - i))) & 3] for i in range(h))
    return arm(key >> (k - 1)) + bytes([mid]) + arm(key & ((1 << (k - 1)) - 1)) + b"N"


def key_int(q):
    return (int(q["hi"]) << 64) | int(q["lo"])


def test_hash_restatement_is_a_bijection():
    rng = np.random.default_rng(1)
    for k in range(33, 64, 2):
        for _ in range(50):
            x = int.from_bytes(rng.bytes(16), "little") & ((1 << (2 * (k - 1))) - 1)
            assert hunmix_w(hmix_w(x, k), k) == x and hmix_w(hunmix_w(x, k), k) == x and hmix_w(x, k) < 1 << (2 * (k - 1))


@pytest.mark.parametrize("k", [35, 41, 63])
@pytest.mark.parametrize("rc", [False, True])
def test_hash_restatement_orders_the_engine_rows(E, k, rc, tmp_path):
    """the rows of a fresh merge are held in the order of H (Array.export sorts them by key; the .skf the engine writes keeps the array's row
    order and the oracle reads it in file order): under the restated H the file's keys must ascend strictly"""
    samples = related(np.random.default_rng(900 + k), 6000, 3, 10)
    ga, oa = build_both(E, samples, k, rc)
    assert E.default_context().merge_path() == "append128"
    ga.save(str(tmp_path / "h.skf"))
    keys = [key_int(q) for q in ora.Array.load(str(tmp_path / "h.skf")).export()[0]]
    hs = [hmix_w(x, k) for x in keys]
    assert len(hs) > 6000 and all(a < b for a, b in zip(hs, hs[1:]))
    assert any(a > b for a, b in zip(keys, keys[1:]))                     # (and that is not the order of the keys themselves)
    assert as_map(*ga.export()) == as_map(*oa.export())


N_CARRIERS = 32                   # samples 0..31 carry the built keys: s and s + 16 are one wave's first and second sample


def built_groups(rng, k, logQ):
    """[(family, [hash values])]: every group shares its top 24 hash bits and more, so it is one row block and one part for any logQ <= 24.
    E_lo holds the nlo = rem - 63 lowest hash bits (above its 14 rank bits), E_hi the 63 above them; the home slot is the log2(slots) <= 12
    bits under the block bits."""
    bits = 2 * (k - 1)
    rem = bits - logQ
    nlo = rem - 63
    assert nlo >= 2 and logQ <= 24 and bits - 36 >= 30
    fresh = lambda nb=bits: int.from_bytes(rng.bytes(16), "little") & ((1 << nb) - 1)
    lowmask = (1 << nlo) - 1
    out = []
    for _ in range(200):                                                  # low-bit twins: the bit directly above the 14 rank bits where rem = 113
        h = fresh()
        out.append(("low_bit", [h, h ^ 1]))
    for _ in range(100):                                                  # E_hi twins: only the highest key bit of E_lo differs
        h = fresh()
        out.append(("ehi_top", [h, h ^ (1 << (nlo - 1))]))
    for n, name in ((3, "ehi_three"), (4, "ehi_four")):                   # three and four keys to one E_hi
        for _ in range(60):
            h = fresh() & ~lowmask
            lows = set()
            while len(lows) < n:
                lows.add(fresh(nlo))
            out.append((name, [h | x for x in sorted(lows)]))
    for _ in range(200):                                                  # E_lo twins: only the lowest bit of E_hi differs
        h = fresh()
        out.append(("elo", [h, h ^ (1 << nlo)]))
    def one_home(prefix36, n):
        lows = set()
        while len(lows) < n:
            lows.add(fresh(bits - 36))
        return [(prefix36 << (bits - 36)) | x for x in sorted(lows)]
    for n, groups in ((9, 60), (12, 60), (40, 20)):                       # more keys to one home slot than the eight bytes the look-up reads
        for _ in range(groups):
            out.append((f"home{n}", one_home(fresh(36), n)))
    for top2, n in ((0, 9), (1, 12), (2, 40)):                            # home bits all ones for any logQ in 2..24: probing runs into the pad
        out.append((f"home{n}_last_slot", one_home((top2 << 34) | ((1 << 34) - 1), n)))
    keys = [h for _, g in out for h in g]
    assert len(set(keys)) == len(keys)
    return out


def place_groups(rng, groups, k, samples):
    """each key as its own record, asserted through the oracle; group g: placement g % 3 from sample s = (g // 3) % 16 --
    0: all keys in sample s (lanes of one insert batch race for one E_hi / one home);
    1: alternating in s and s + 1 (two waves race; the loser waits for E_lo);
    2: alternating in s and s + 16 (the same wave later: the look-up reads the first key's entry, misses, and the insert loop walks on);
    and every key once more, with a middle base of its own, in sample s + 8 or (s + 24) % 32 (another wave: found again or inserted first, one
    row either way)."""
    for g, (_, hs) in enumerate(groups):
        s = (g // 3) % 16
        step = (0, 1, 16)[g % 3]
        for i, h in enumerate(hs):
            key = hunmix_w(h, k)
            assert hmix_w(key, k) == h
            for smp in (s + step * (i % 2), (s + 8 + 16 * (i % 2)) % N_CARRIERS):
                rec = key_record(key, k, CODE[int(rng.integers(0, 4))])
                d = oracle_dict([rec], k, False)
                assert len(d) == 1 and key_int(d.export()[0][0]) == key
                samples[smp].append(rec)


# k: (bases of the ancestor, SNPs a sample, logQ) -- 3 541 built keys + the ancestor + 0.75 x SNPs x k rows a sample:
#   k = 35: 9 000 + 2 520 + 3 541 = 15 060 rows, 0.69 of 8 x MAX_MEAN and 1.38 of 4 x; the longest sample stays under 25 600 bytes (logB <= 3 = logQ):
#           rem = 65, the smallest with two key bits in E_lo
#   k = 41: 24 000 + 4 920 + 3 541 = 32 460 rows, 0.74 of 16 x MAX_MEAN;  k = 63: the clamp, rem = 113
BUILT = {35: (9000, 3, 3), 41: (24_000, 5, 4), 63: (24_000, 5, 11)}


def built_samples(k):
    length, snps, logQ = BUILT[k]
    rng = np.random.default_rng(8000 + k)
    samples = related(rng, length, N_CARRIERS, snps)
    groups = built_groups(rng, k, logQ)
    place_groups(rng, groups, k, samples)
    return samples, groups


@pytest.mark.parametrize("k", [63, 41, 35])
def test_wide_append_built_keys(E, k, capfd, monkeypatch):
    """The split is sized by the count-only launch here (SKX_KNOBS=probe_launch: append_wide_kernel<true, QS, PD> over every block of a 2^4 or 2^5
    split, the first 64 of 2^11 at k = 63), which counts the built keys as the rows they are -- the keys of a group share the 18 hash bits under
    the region bits that index the split sketch, so the sketch takes a group for one row: the test below."""
    logQ = BUILT[k][2]
    samples, groups = built_samples(k)
    monkeypatch.setenv("SKX_DEBUG", "1")
    set_knob(monkeypatch, "probe_launch", 1)
    names = [f"s{i}" for i in range(len(samples))]
    ga, lines, path = merge_with_lines(E, capfd, samples, k, False, names)
    rem, QS, PD, pb = form_of(k, logQ)
    with capfd.disabled():
        fam = {}
        for name, hs in groups:
            fam[name] = fam.get(name, 0) + 1
        print(f"\n    k={k} built keys {fam} want (logQ, rem, QS, PD, pb)={(logQ, rem, QS, PD, pb)}: {lines} path={path}", flush=True)
    assert path == "append128" and len(lines) == 1 and lines[0][5] == "ok"
    assert lines[0][0] == logQ and logQ <= 24 and rem >= 65               # the groups were built for this split
    assert lines[0][2] % 128 == 0 and lines[0][2] <= 3072 and lines[0][3] <= 4096
    want = check_parity(E, samples, k, False, ga, monkeypatch)
    del_knob(monkeypatch, "probe_launch")
    # every built key is a row of its own (the oracle's rows were compared above; this pins that the inputs are what the docstrings say)
    have = set((int(h) << 64) | int(l) for l, h in zip(want[0], want[1]))
    assert all(hunmix_w(h, k) in have for _, hs in groups for h in hs)


def test_wide_append_built_keys_that_the_sketch_takes_for_one_row(E, capfd, monkeypatch):
    """the same samples at k = 35 sized by the sketch: it sees about 770 of the 3 541 built keys, the blocks of the split it asks for overflow, and
    the pass comes back finer -- any number of `overflow` lines before the `ok`; the array is the oracle's"""
    k = 35
    samples, groups = built_samples(k)
    monkeypatch.setenv("SKX_DEBUG", "1")
    names = [f"s{i}" for i in range(len(samples))]
    ga, lines, path = merge_with_lines(E, capfd, samples, k, False, names)
    with capfd.disabled():
        print(f"\n    k={k} built keys, sized by the sketch: {lines} path={path}", flush=True)
    assert path == "append128" and lines and lines[-1][5] == "ok" and all(x[5] == "overflow" for x in lines[:-1])
    assert [x[0] for x in lines] == list(range(lines[0][0], lines[0][0] + len(lines)))
    check_parity(E, samples, k, False, ga, monkeypatch)


def test_wide_append_more_keys_to_the_last_slot_than_the_pad_holds(E, capfd, monkeypatch):
    """80 keys whose home bits are all ones: the table's last slot and the 64 of the pad hold 65.  The block fails at every split (the home bits
    stay all ones), so any number of `overflow` lines and either final path is accepted: the call returns and the array is the oracle's."""
    k = 41
    rng = np.random.default_rng(8800)
    samples = related(rng, 24_000, 20, 5)
    bits = 2 * (k - 1)
    lows = set()
    while len(lows) < 80:
        lows.add(int.from_bytes(rng.bytes(8), "little") & ((1 << (bits - 36)) - 1))
    for i, x in enumerate(sorted(lows)):
        key = hunmix_w((((3 << 34) | ((1 << 34) - 1)) << (bits - 36)) | x, k)
        rec = key_record(key, k, CODE[i % 4])
        d = oracle_dict([rec], k, False)
        assert len(d) == 1 and key_int(d.export()[0][0]) == key
        samples[i % 5].append(rec)
    monkeypatch.setenv("SKX_DEBUG", "1")
    names = [f"s{i}" for i in range(len(samples))]
    ga, lines, path = merge_with_lines(E, capfd, samples, k, False, names)
    with capfd.disabled():
        print(f"\n    k={k} 80 keys to the last slot: {lines} path={path}", flush=True)
    assert path == "append128" or path.startswith("sorted:")
    oa = ora.Array.from_dicts([oracle_dict(r, k, False) for r in samples], names)
    assert ga.names == oa.names and ga.nkmers == oa.nkmers and same_rows(rows_of(ga), rows_of(oa))
    assert list(ga.sample_kmers()) == [int(x) for x in (oa.export()[1] != ord("-")).sum(axis=0)]
