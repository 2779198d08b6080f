"""The split sketch: the append pass sized from bitmaps the extraction kernel fills, instead of from a count-only launch of the append kernel.

extract_kernel / extract_wide_kernel (scatter form, fixed-capacity regions) set, for every word of a *sketch region* (every 256th bucket from
2^10 buckets a sample on, every 64th from 2^8, every bucket below), one of M = 2^18 bits (128-bit keys: the 18 hash bits below the word's bucket bits; 64-bit keys: a
multiplicative hash of H's low 32 bits cut to the bits below the bucket bits -- sketch_index64, and why, below), in the bitmap copy of their XCD; sketch_count_kernel counts the zero bits Z of the OR of the copies and append_pass takes n = -M ln(Z / M) rows a region (M = 2^m: linear
counting), sums the regions and sizes its row blocks from that.  SKX_KNOBS=probe_launch=1 forces the count-only launch, which also serves
dictsets without a sketch and a sketch more than half full.  The pass's SKX_DEBUG line says which of the two sized it and what the estimate was.

The estimator's own error, computed here from the formula and not from what the engine prints: n distinct keys are n balls in M bins, and
Var(n^) = M (e^t - t - 1) with t = n / M (Whang et al. 1990); independent regions add their variances.  The allowed error of the summed
estimate is six of these sigmas (+ 0.05 for the one decimal the debug line prints).  test_an_ideal_bitmap_stays_inside_the_bound needs no GPU:
it hashes the oracle's keys with numpy and checks that the inputs chosen here keep an ideal bitmap inside that bound.

Shapes: the three the sketch was specified with (24 related and 24 unrelated samples of 200 kbp, 3 samples of 2 kbp -- all of them below 2^8
buckets, so every bucket is sketched and the truth is the array's row count), one with 2^9 buckets (3 x 1.3 Mbp: 8 sketch regions, the truth
is the rows whose bucket is a multiple of 64; also the `parts` mapping of fewer than eight samples with 64 tiles and more), one with 2^10
(2 x 2.6 Mbp: 4 sketch regions, every 256th bucket -- the rule of the 5 Mbp shape) and small ones
around them: tiles staged in two rounds with a partial last tile, one sample alone, 128-bit keys, a sample that is one repeat, a hash too short
for a sketch, a sketch filled beyond its threshold and the retry after an underestimate."""
import math
import re

import numpy as np
import pytest
from conftest import set_knob, del_knob

import ora
from test_gpu_parity import oracle_dict
from test_gpu_append_shapes import LINE, genome, related, unrel, rows_of, same_rows

gpu = pytest.mark.gpu

M_BITS = 18                       # SKETCH_M (skx_device.h)
M = 1 << M_BITS
MAX_FILL = 0.5                    # SKETCH_MAX_FILL
MAX_MEAN = 5537                   # rows a block of the 64-bit pass: the largest mean with mean + 6 sqrt(mean + 1) + 32 <= 6 016
SIZED = re.compile(r"-> (?:ok|overflow) \[sized by ([^\]]*)\]")
SKETCH = re.compile(r"the sketch: ([0-9.]+) rows in (\d+) sketch regions, fill ([0-9.]+)")


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


# ---- the layout rules of the engine, restated (region_layout, sketch_step_log, make_hash_params / hmix) -------------------------------
def log_buckets(longest, k):
    per_region, base = (3200, 11) if k > 31 else (4900, 10)
    need = max(0, math.ceil(math.log2(-(-longest // per_region))))
    return min(need if need <= base else max(base, need - 5), 2 * (k - 1), 13)


def sketch_step(logB):
    return 8 if logB >= 10 else 6 if logB >= 8 else 0


def hash64(keys, k):
    """H of the 2 (k - 1)-bit split k-mers (k <= 31): the two-round Feistel mix of skx_device.h on 32-bit halves"""
    hb = k - 1
    x = keys.astype(np.uint64)
    left, right = (x >> np.uint64(hb)).astype(np.uint32), (x & np.uint64((1 << hb) - 1)).astype(np.uint32)
    left ^= (right * np.uint32(0x9E3779B1)) >> np.uint32(32 - hb)
    right ^= (left * np.uint32(0x85EBCA6B)) >> np.uint32(32 - hb)
    return (left.astype(np.uint64) << np.uint64(hb)) | right.astype(np.uint64)


def region_rows(keys_lo, k, logB, naive=False):
    """exact rows per sketch region, and the (region, bit) of every row in one -- k <= 31"""
    bits, step = 2 * (k - 1), sketch_step(logB)
    h = hash64(keys_lo, k)
    bucket = (h >> np.uint64(bits - logB)).astype(np.int64) if logB else np.zeros(len(h), dtype=np.int64)
    low = (h & np.uint64(0xFFFFFFFF)).astype(np.uint32) * np.uint32(0x9E3779B1)                   # sketch_index64
    idx = ((low >> np.uint32(min(32, bits - logB) - M_BITS)) & np.uint32(M - 1)).astype(np.int64)
    if naive:                                                                                       # the bits below the bucket bits
        idx = ((h >> np.uint64(bits - logB - M_BITS)) & np.uint64(M - 1)).astype(np.int64)
    take = (bucket & ((1 << step) - 1)) == 0
    region = bucket[take] >> step
    return np.bincount(region, minlength=1 << (logB - step)), region, idx[take]


def wide_bucket_rows(lo, hi, k, logB):
    """exact rows per bucket for 128-bit keys (k > 31): the upper half of the three-round mix on 64-bit halves"""
    hb = k - 1
    mask, sh = np.uint64((1 << hb) - 1), np.uint64(64 - hb)
    left = ((hi.astype(np.uint64) << sh) | (lo.astype(np.uint64) >> np.uint64(hb))) & mask
    right = lo.astype(np.uint64) & mask
    left ^= (right * np.uint64(0x9E3779B97F4A7C15)) >> sh
    right ^= (left * np.uint64(0xD6E8FEB86659FD93)) >> sh
    left ^= (right * np.uint64(0xC2B2AE3D27D4EB4F)) >> sh
    return np.bincount((left >> np.uint64(hb - logB)).astype(np.int64), minlength=1 << logB)


def six_sigma(rows_per_region):
    t = np.asarray(rows_per_region, dtype=np.float64) / M
    return 6.0 * math.sqrt(float(np.sum(M * (np.exp(t) - t - 1.0))))


# ---- the inputs: made once, with the oracle's array ------------------------------------------------------------------------------------
ESTIMATE = {
    # id: (k, samples(rng), row blocks: log2, per region)
    # (k = 31: 2^10 row blocks at least -- a table entry has room for 50 hash bits; the unrelated samples need them for their 4.8 M rows)
    "related_24x200k": (31, lambda r: related(r, 200_000, 24, 40), 10, 16),
    "unrelated_24x200k": (31, lambda r: unrel(r, 200_000, 24), 10, 16),
    "tiny_3x2k": (31, lambda r: related(r, 2_000, 3, 3, cut=1), 10, 1024),
    "every_64th_bucket_3x1300k": (31, lambda r: related(r, 1_300_000, 3, 60), 10, 2),
    "every_256th_bucket_2x2600k": (31, lambda r: related(r, 2_600_000, 2, 60), 10, 1),
    "two_staging_rounds_2x30k": (31, lambda r: related(r, 30_000, 2, 10), 10, 128),
    # (k = 21: the split follows from the rows alone -- 8 regions, 295 000 rows: 2^6 blocks of 4 600)
    "unrelated_8x37k_k21": (21, lambda r: unrel(r, 37_000, 8), 6, 8),
}
_made = {}


def made(case):
    """(k, samples, names, oracle rows in key order, longest sample)"""
    if case not in _made:
        k, make = ESTIMATE[case][:2] if case in ESTIMATE else OTHER[case]
        samples = make(np.random.default_rng(sum(case.encode()) * 7 + k))
        names = [f"s{i}" for i in range(len(samples))]
        oa = ora.Array.from_dicts([oracle_dict(r, k, True) for r in samples], names)
        _made[case] = (k, samples, names, rows_of(oa), max(sum(len(x) + 1 for x in r) for r in samples))
    return _made[case]


def merge(E, capfd, samples, k, names):
    """a fresh build and merge: (array, [(logQ, A, cap, slots, rows, how)], [sized by ...], merge path)"""
    capfd.readouterr()
    ga = E.DictSet.build([E.record_stream(r) for r in samples], k, True).merge(names)
    err = capfd.readouterr().err
    wide = LINE.pattern.replace("append:", r"append(?: \(128-bit keys\))?:")
    lines = [(int(q), int(a), int(c), int(s), int(r), how) for q, a, c, s, r, how in re.findall(wide, err)]
    return ga, lines, SIZED.findall(err), E.default_context().merge_path(), err


def truth_of(case):
    k, _, _, want, longest = made(case)
    logB = log_buckets(longest, k)
    if k > 31:
        assert sketch_step(logB) == 0                                    # (wide keys: only shapes with every bucket sketched)
        return logB, wide_bucket_rows(want[0], want[1], k, logB)
    return logB, region_rows(want[0], k, logB)[0]


@pytest.mark.parametrize("case", list(ESTIMATE))
def test_an_ideal_bitmap_stays_inside_the_bound(case):
    """no GPU: the oracle's keys hashed with numpy into ideal bitmaps -- the linear-counting estimate of these very inputs lies within six sigma
    of the formula, region by region and summed (so a failure of the GPU test below is the engine's, not the inputs')"""
    k, _, _, want, longest = made(case)
    logB = log_buckets(longest, k)
    rows, region, idx = region_rows(want[0], k, logB)
    assert len(rows) == 1 << (logB - sketch_step(logB)) and (sketch_step(logB) or rows.sum() == len(want[0]))
    set_bits = np.bincount(np.unique(region * M + idx) // M, minlength=len(rows))
    assert set_bits.max() / M <= MAX_FILL
    est = -M * np.log((M - set_bits) / M)
    print(f"\n    {case}: logB={logB} regions={len(rows)} rows={int(rows.sum())} ideal estimate={est.sum():.1f} "
          f"error={est.sum() - rows.sum():+.1f} allowed={six_sigma(rows):.1f}", flush=True)
    assert abs(est.sum() - rows.sum()) <= six_sigma(rows)
    assert all(abs(e - n) <= six_sigma([n]) for e, n in zip(est, rows))


def test_the_bits_below_the_bucket_bits_would_undercount_related_samples():
    """no GPU: why the 64-bit keys hash their index.  H's upper half is L ^ f(R): two split k-mers with one lower arm whose upper arms differ in
    a base near the middle one (a SNP makes them) differ in L's low bits alone, which the 18 bits below the bucket bits do not reach -- one bit
    for two rows, and an estimate beyond six sigma below the truth.  sketch_index64 on the same rows is inside (the test above)."""
    k, _, _, want, longest = made("tiny_3x2k")
    logB = log_buckets(longest, k)
    rows, region, idx = region_rows(want[0], k, logB, naive=True)
    set_bits = np.bincount(np.unique(region * M + idx) // M, minlength=len(rows))
    est = -M * np.log((M - set_bits) / M)
    print(f"\n    tiny_3x2k, bits below the bucket bits: rows={int(rows.sum())} estimate={est.sum():.1f} allowed={six_sigma(rows):.1f}", flush=True)
    assert rows.sum() - est.sum() > six_sigma(rows)


@gpu
@pytest.mark.parametrize("case", list(ESTIMATE))
def test_estimate_against_truth_and_same_array_either_way(E, case, capfd, monkeypatch):
    """the sketch's rows against the exact count in the sketch regions, within the estimator's own six sigma; then the same samples with the
    count-only launch forced: one array, the oracle's, and the same split (these shapes lie 15 % and more from a row count at which it changes)"""
    monkeypatch.setenv("SKX_DEBUG", "1")
    k, samples, names, want, _ = made(case)
    logQ, A = ESTIMATE[case][2:]
    logB, rows = truth_of(case)
    ga, lines, sized, path, _ = merge(E, capfd, samples, k, names)
    assert path == "append64" and len(lines) == 1 and lines[0][5] == "ok" and len(sized) == 1
    m = SKETCH.fullmatch(sized[0])
    assert m, sized
    est, nreg, fill = float(m.group(1)), int(m.group(2)), float(m.group(3))
    allowed = six_sigma(rows) + 0.05
    with capfd.disabled():
        print(f"\n    {case}: logB={logB} {lines[0]} sketch estimate={est} in {nreg} regions (fill {fill}), exact={int(rows.sum())}, "
              f"error={est - rows.sum():+.1f}, allowed={allowed:.1f}", flush=True)
    assert nreg == 1 << (logB - sketch_step(logB))
    assert abs(est - rows.sum()) <= allowed
    assert fill <= MAX_FILL
    set_knob(monkeypatch, "probe_launch", 1)
    gp, plines, psized, ppath, _ = merge(E, capfd, samples, k, names)
    del_knob(monkeypatch, "probe_launch")
    with capfd.disabled():
        print(f"    {case}: probe launch {plines} [{psized}]", flush=True)
    assert ppath == "append64" and len(plines) == 1 and plines[0][5] == "ok"
    assert psized == ["the probe launch: SKX_KNOBS=probe_launch"]
    assert (lines[0][0], lines[0][1]) == (logQ, A) and lines[0][0] - plines[0][0] == 0          # the same split, and the one the row count asks for
    assert ga.names == gp.names == names and ga.nkmers == gp.nkmers == len(want[0])
    got, gotp = rows_of(ga), rows_of(gp)
    assert same_rows(got, want) and same_rows(gotp, want) and same_rows(got, gotp)
    assert list(ga.sample_kmers()) == list(gp.sample_kmers()) == [int(x) for x in (want[2] != ord("-")).sum(axis=0)]


# ---- the cases around them ---------------------------------------------------------------------------------------------------------------
def saturating(rng):
    """unrelated samples of 4 899 bases (4 900 with the record's end: one region, the smallest logB) until the bitmap is more than MAX_FILL full:
    M ln(1 / (1 - fill)) rows, 4 879 a sample at k = 21, and 3 % over -- 39 samples"""
    n = math.ceil(-M * math.log(1.0 - MAX_FILL) / (4899 - 20) * 1.03)
    return unrel(rng, 4899, n)


def one_repeat(rng):
    s = related(rng, 60_000, 6, 30)
    unit = genome(rng, 70).tobytes()
    return s + [[b"A" * 120_000, unit * 1500], [b"AC" * 50_000 + s[0][0][:5000]]]


OTHER = {
    "saturated": (21, saturating),
    "underestimate": (21, lambda r: unrel(r, 37_000, 4)),
    "one_sample_alone": (31, lambda r: related(r, 800_000, 1, 0)),
    "one_repeat": (31, one_repeat),
    "short_hash": (9, lambda r: related(r, 30_000, 3, 20)),
    "wide_smallest": (41, lambda r: related(r, 3_000, 3, 3, cut=1)),
    "wide_all_rounds": (41, lambda r: related(r, 36_000, 4, 10)),
}


def check_equals_oracle(ga, case):
    _, _, names, want, _ = made(case)
    assert ga.names == names and ga.nkmers == len(want[0]) and same_rows(rows_of(ga), want)
    assert list(ga.sample_kmers()) == [int(x) for x in (want[2] != ord("-")).sum(axis=0)]


@gpu
def test_a_sketch_more_than_half_full_leaves_the_sizing_to_the_probe_launch(E, capfd, monkeypatch):
    monkeypatch.setenv("SKX_DEBUG", "1")
    k, samples, names, want, longest = made("saturated")
    assert log_buckets(longest, k) == 0 and 1.0 - math.exp(-len(want[0]) / M) > MAX_FILL + 0.01
    ga, lines, sized, path, _ = merge(E, capfd, samples, k, names)
    with capfd.disabled():
        print(f"\n    saturated: S={len(samples)} rows={len(want[0])} {lines} {sized} path={path}", flush=True)
    assert path == "append64" and [x[5] for x in lines] == ["ok"]
    m = re.fullmatch(r"the probe launch: the sketch is ([0-9.]+) full", sized[0])
    assert m and abs(float(m.group(1)) - (1.0 - math.exp(-len(want[0]) / M))) < 0.01
    assert lines[0][0] == math.ceil(math.log2(len(want[0]) / MAX_MEAN))      # 2^6 row blocks on the one region
    check_equals_oracle(ga, "saturated")


@gpu
def test_an_underestimate_is_retried_one_split_finer(E, capfd, monkeypatch):
    """SKX_KNOBS=append_coarse=1 starts one step coarser than the sketch asks for: the blocks overflow and the pass comes back at the sketch's split"""
    monkeypatch.setenv("SKX_DEBUG", "1")
    k, samples, names, _, _ = made("underestimate")
    set_knob(monkeypatch, "append_coarse", 1)
    ga, lines, sized, path, _ = merge(E, capfd, samples, k, names)
    del_knob(monkeypatch, "append_coarse")
    with capfd.disabled():
        print(f"\n    underestimate: {lines} {sized} path={path}", flush=True)
    assert path == "append64" and [(x[0], x[5]) for x in lines] == [(4, "overflow"), (5, "ok")]
    assert len(sized) == 2 and all(SKETCH.fullmatch(s) for s in sized)
    check_equals_oracle(ga, "underestimate")


@gpu
def test_one_sample_alone_is_sized_by_its_windows(E, capfd, monkeypatch):
    """fewer than eight samples with 64 tiles and more: the tiles are dealt to the XCDs in ranges (`parts`) and fill the copies of their XCDs; a
    single sample needs no estimate at all (its windows bound its rows), and its array is the oracle's"""
    monkeypatch.setenv("SKX_DEBUG", "1")
    k, samples, names, _, _ = made("one_sample_alone")
    ga, lines, sized, path, _ = merge(E, capfd, samples, k, names)
    assert path == "append64" and [x[5] for x in lines] == ["ok"] and sized == ["one sample"]
    check_equals_oracle(ga, "one_sample_alone")


@gpu
def test_a_sample_that_is_one_repeat_has_no_sketch_and_no_probe(E, capfd, monkeypatch):
    monkeypatch.setenv("SKX_DEBUG", "1")
    k, samples, names, _, _ = made("one_repeat")
    E.default_context().timings(reset=True)
    ga, lines, sized, path, err = merge(E, capfd, samples, k, names)
    assert path.startswith("sorted: the dictionaries are sorted") and lines == [] and sized == [] and "[skx] append" not in err
    assert E.default_context().timings()["append_probe"] == 0
    check_equals_oracle(ga, "one_repeat")


@gpu
def test_a_dictset_without_a_sketch_is_sized_by_the_probe_launch(E, capfd, monkeypatch):
    """k = 9: sixteen hash bits, thirteen below the bucket bits -- fewer than a bitmap's index takes, so the dictset has no sketch"""
    monkeypatch.setenv("SKX_DEBUG", "1")
    k, samples, names, _, _ = made("short_hash")
    ga, lines, sized, path, _ = merge(E, capfd, samples, k, names)
    assert path == "append64" and [x[5] for x in lines] == ["ok"] and sized == ["the probe launch: no sketch"]
    check_equals_oracle(ga, "short_hash")


@gpu
@pytest.mark.parametrize("case", ["wide_smallest", "wide_all_rounds"])
def test_wide_keys_fill_and_use_the_sketch(E, case, capfd, monkeypatch):
    """k = 41 (extract_wide_kernel, append_wide_kernel): a sample shorter than one staging round's 2 048 words but for a few, and tiles of
    all four rounds; every bucket is sketched, so the truth is the row count.  Estimate, split and array as for the 64-bit keys."""
    monkeypatch.setenv("SKX_DEBUG", "1")
    k, samples, names, want, longest = made(case)
    logB, rows = truth_of(case)
    assert rows.sum() == len(want[0]) and len(rows) == 1 << logB
    ga, lines, sized, path, _ = merge(E, capfd, samples, k, names)
    assert path == "append128" and [x[5] for x in lines] == ["ok"] and len(sized) == 1
    m = SKETCH.fullmatch(sized[0])
    assert m, sized
    with capfd.disabled():
        print(f"\n    {case}: {lines} estimate={m.group(1)} in {m.group(2)} regions, exact={len(want[0])}, allowed={six_sigma(rows) + 0.05:.1f}", flush=True)
    assert int(m.group(2)) == 1 << logB
    assert abs(float(m.group(1)) - rows.sum()) <= six_sigma(rows) + 0.05
    set_knob(monkeypatch, "probe_launch", 1)
    gp, plines, psized, ppath, _ = merge(E, capfd, samples, k, names)
    del_knob(monkeypatch, "probe_launch")
    assert ppath == "append128" and psized == ["the probe launch: SKX_KNOBS=probe_launch"] and plines[0][0] - lines[0][0] == 0
    check_equals_oracle(ga, case)
    check_equals_oracle(gp, case)
