"""The stage every pass stands on -- extract_kernel / extract_wide_kernel, the per-region counting sort and the host policy that picks their
shapes -- at its tile, dealing and shape edges.

Every case builds with E.DictSet.build and compares each sample's exported dictionary (lo, hi, middle-base byte, length) bit for bit with the
oracle's, and every case asserts from the build's SKX_DEBUG line (`[skx] build: ...`, csrc/skx_dictset.cpp) that the build took the path the case is
named for; the expected numbers are the ones tests/test_build_plan_policy.py works out.

  A  record ends against the tile, the 16-byte chunk and the stream end: the one place the extraction kernels look at the text a second time
     (split_kmer.rs:89: a clean run of exactly k bases that ends on the record's last base gives no window).  The 36 three-tile streams go
     through one build as a batch of 36 samples -- a workgroup is one (sample, tile), whatever the batch -- and four of them again alone
  B  the dealing of tiles to XCDs (`parts`) for one to seven samples at 63 | 64 | 67 tiles, and the group arithmetic and the prefetch of the
     head of sample s + 8 without it
  C  every extract instantiation: SKX_KNOBS=region_logb puts a 150 kbp sample into the layouts of a 160+ Mbp one
  D  every dedupe launch shape, both HI forms, the 128-bit sort, and the two-shape launch with listed regions
  E  a region beyond its fixed capacity: the exact layout sorted per region, or flat; a region exactly at its capacity, and one word more"""
import re

import numpy as np
import pytest
from conftest import set_knob, del_knob

import ora
from test_build_plan_policy import SHAPES, TILE64, TILE128, capacity, longest_with_capacity
from test_gpu_parity import oracle_dict
from test_gpu_split_sketch import hash64, wide_bucket_rows
from test_gpu_append_shapes import rows_of, same_rows

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
BUILD = re.compile(r"\[skx\] build: n=(\d+) k=(\d+) longest=(\d+) logB=(-?\d+) cap=(\d+) tile=(\d+) tiles_max=(\d+) parts=(\d+) tiles_part=(\d+) "
                   r"extract_hi=(\d) layout=(\w+) largest=(\d+) end=([\w-]+)"
                   r"(?: sort_cap=(\d+) shape=(\d+) typical=(\d+) shape_typ=(\d+) dedupe_hi=(\d)/(\d))?")
BUILD_FIELDS = ("n", "k", "longest", "logB", "cap", "tile", "tiles_max", "parts", "tiles_part", "extract_hi", "layout", "largest", "end",
                "sort_cap", "shape", "typical", "shape_typ", "dedupe_hi", "dedupe_hi_typ")
LISTED = re.compile(r"\[skx\] dedupe: typical region (\d+) words, capacity (\d+); (\d+) of (\d+) regions above the typical launch shape")


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def tile_of(k):
    return TILE128 if k > 31 else TILE64


def bases(rng, n):
    return ACGT[rng.integers(0, 4, size=n)]


def records_of(stream):
    return bytes(stream).split(b"\n")


_oracle = {}


def oracle_export(stream, k, rc, key=None):
    """the oracle's dictionary of a record stream; `key` shares it between the cases that build the same stream"""
    if key is not None and (key, k, rc) in _oracle:
        return _oracle[(key, k, rc)]
    out = oracle_dict(records_of(stream), k, rc).export()
    if key is not None:
        _oracle[(key, k, rc)] = out
    return out


def build_line(err):
    lines = BUILD.findall(err)
    assert len(lines) == 1, err
    return {f: (v if f in ("layout", "end") else int(v) if v != "" else None) for f, v in zip(BUILD_FIELDS, lines[0])}


def build_checked(E, capfd, monkeypatch, streams, k, rc, keys=None):
    """one build: (dictset, its debug line's fields, all of stderr); every sample's dictionary against the oracle's, bit for bit"""
    monkeypatch.setenv("SKX_DEBUG", "1")
    capfd.readouterr()
    ds = E.DictSet.build([bytes(s) for s in streams], k, rc)
    err = capfd.readouterr().err
    line = build_line(err)
    assert (line["n"], line["k"], line["longest"]) == (len(streams), k, max(len(s) for s in streams))
    for i, s in enumerate(streams):
        ok, ob = oracle_export(s, k, rc, keys[i] if keys else None)
        gk, gb = ds.export(i)
        assert len(gk) == len(ok), (k, rc, i, len(gk), len(ok))
        assert np.array_equal(gk["lo"], ok["lo"]) and np.array_equal(gk["hi"], ok["hi"]), (k, rc, i)
        assert np.array_equal(gb, ob), (k, rc, i)
    return ds, line, err + capfd.readouterr().err


def merge_checked(E, streams, k, rc):
    """a fresh build's merge against the oracle's array"""
    names = [f"s{i}" for i in range(len(streams))]
    ga = E.DictSet.build([bytes(s) for s in streams], k, rc).merge(names)
    oa = ora.Array.from_dicts([oracle_dict(records_of(s), k, rc) for s in streams], names)
    assert ga.names == oa.names and ga.nkmers == oa.nkmers
    assert same_rows(rows_of(ga), rows_of(oa))
    return E.default_context().merge_path()


# ---- A: record ends against the tile, the chunk and the stream ----------------------------------------------------------------------------
def end_offsets(k):
    return (-k - 1, -k, -2, -1, 0, 1, 15, 16, 17)


def place_run(s, end, run):
    """a bad base, then a clean run of `run` bases whose last is the record's last: the terminator stands at stream offset `end`"""
    s[end] = ord("\n")
    s[end - run - 1] = ord("N")
    assert not np.isin(s[end - run:end], (ord("N"), ord("\n"))).any()


def record_end_streams(rng, k):
    """three-tile streams, two per offset d: a terminator at T + d for both inner tile starts T, behind a run of exactly k bases at one and of
    k + 1 at the other, and the other way round; then the streams that end at and around a tile start, the last record that run"""
    T = tile_of(k)
    streams = []
    for d in end_offsets(k):
        for first, second in ((k, k + 1), (k + 1, k)):
            s = bases(rng, 3 * T)
            place_run(s, T + d, first)
            place_run(s, 2 * T + d, second)
            s[-1] = ord("\n")
            streams.append(s)
    for length in (2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 15, 2 * T + 16, 2 * T + 17):
        for run, terminated in ((k, False), (k, True), (k + 1, False)):
            s = bases(rng, length)
            last = length - 1 if terminated else length                    # where the run's terminator stands, or would
            s[last - run - 1] = ord("N")
            if terminated:
                s[last] = ord("\n")
            s[T // 2] = ord("\n")                                           # (an ordinary record end inside a tile)
            streams.append(s)
    return streams


@pytest.mark.parametrize("rc", [True, False])
@pytest.mark.parametrize("k", [15, 31, 33, 63])
def test_record_ends_at_tile_chunk_and_stream_edges(E, k, rc, capfd, monkeypatch):
    T = tile_of(k)
    streams = record_end_streams(np.random.default_rng(900 + k), k)
    assert len(streams) == 2 * 9 + 6 * 3 and max(len(s) for s in streams) == 3 * T
    ds, line, _ = build_checked(E, capfd, monkeypatch, streams, k, rc)
    with capfd.disabled():
        print(f"\n    A k={k} rc={int(rc)}: {line}", flush=True)
    # three tiles of 12 288 (8 192) positions; 36 864 bytes are 8 (24 576: 8) regions' worth: ceil(36 864 / 4 900) = 8, ceil(24 576 / 3 200) = 8
    assert (line["tile"], line["tiles_max"], line["logB"], line["parts"]) == (T, 3, 3, 0)
    assert (line["layout"], line["end"]) == ("fixed", "extracted")
    ds.free()
    # ... and each of them alone, as the issue's "one sample of three tiles": the two streams of d = 0 and the stream that ends at the tile start
    for s in (streams[8], streams[9], streams[18 + 3], streams[18 + 4]):
        ds, line, _ = build_checked(E, capfd, monkeypatch, [s], k, rc)
        assert (line["tile"], line["tiles_max"], line["parts"], line["layout"]) == (T, -(-len(s) // T), 0, "fixed")
        ds.free()


# ---- B: dealing ---------------------------------------------------------------------------------------------------------------------------
def random_stream(seed, length):
    """unrelated random bases in two records, `length` bytes with the terminators"""
    s = bases(np.random.default_rng(seed), length)
    s[-1] = ord("\n")
    if length > 100:
        s[length // 3] = ord("\n")
    return s


def dealt_batch(tiles, n, k):
    """the first sample has exactly `tiles` tiles; the others len / 2, one tile + 1, 40 bases, and so on: short"""
    T = tile_of(k)
    lengths = [tiles * T, tiles * T // 2, T + 1, 40 + k, T + 8, 41 + k, 2 * T + 3][:n]
    keys = [("dealt", i, length) for i, length in enumerate(lengths)]
    return [random_stream(7000 + 13 * i + length % 1000, length) for i, length in enumerate(lengths)], keys


# (tiles, n) -> (parts, tiles_part): 8 // n ranges of ceil(tiles / parts) tiles from 64 tiles on, n < 8 (test_build_plan_policy.test_parts_table)
DEALT = {(63, 1): (0, 0), (64, 1): (8, 8), (64, 2): (4, 16), (64, 3): (2, 32), (64, 4): (2, 32), (64, 5): (0, None), (64, 7): (0, None),
         (67, 2): (4, 17), (67, 3): (2, 34)}


@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("tiles,n", list(DEALT))
def test_tiles_dealt_to_xcds(E, tiles, n, k, capfd, monkeypatch):
    streams, keys = dealt_batch(tiles, n, k)
    ds, line, _ = build_checked(E, capfd, monkeypatch, streams, k, True, keys)
    with capfd.disabled():
        print(f"\n    B tiles={tiles} n={n} k={k}: {line}", flush=True)
    parts, tiles_part = DEALT[(tiles, n)]
    assert (line["tile"], line["tiles_max"], line["parts"]) == (tile_of(k), tiles, parts)
    if tiles_part is not None:
        assert line["tiles_part"] == tiles_part
    assert (line["layout"], line["end"]) == ("fixed", "extracted")
    ds.free()


def undealt_batch(n, k):
    """samples under two tiles; sample s + 8 is in turn longer, much shorter (no 4 bytes at a lane's 128-byte stride beyond lane 0), and absent"""
    lengths = [13_000 + 37 * s for s in range(8)] + [15_500, 60 + k, 14_100, 64 + k, 13_500, 15_900, 70 + k, 12_900, 16_000][:max(0, n - 8)]
    lengths = lengths[:n]
    return [random_stream(8000 + 7 * i, length) for i, length in enumerate(lengths)], [("undealt", i, length) for i, length in enumerate(lengths)]


@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("n", [9, 15, 17])
def test_groups_of_eight_and_the_next_samples_head(E, n, k, capfd, monkeypatch):
    streams, keys = undealt_batch(n, k)
    ds, line, _ = build_checked(E, capfd, monkeypatch, streams, k, True, keys)
    with capfd.disabled():
        print(f"\n    B undealt n={n} k={k}: {line}", flush=True)
    assert (line["tile"], line["tiles_max"], line["parts"], line["tiles_part"]) == (tile_of(k), 2, 0, 0)
    assert (line["layout"], line["end"]) == ("fixed", "extracted")
    ds.free()


@pytest.mark.parametrize("k", [31, 41])
def test_the_prefetch_reads_the_head_of_sample_s_plus_8(E, k, capfd, monkeypatch):
    """A workgroup whose tile lies within 20 tiles (10 for 128-bit keys) of its sample's end fetches one dword per 128-byte line of the head of
    sample s + 8 instead: samples 0 and 1 have 22 tiles, sample 8 is shorter than the second lane's line (only lane 0 may read), sample 9 longer
    than a tile"""
    T = tile_of(k)
    lengths = [21 * T + 5, 21 * T - 3] + [50 + k + s for s in range(6)] + [60 + k, 3 * T + 1]
    streams = [random_stream(8500 + i, length) for i, length in enumerate(lengths)]
    ds, line, _ = build_checked(E, capfd, monkeypatch, streams, k, True)
    with capfd.disabled():
        print(f"\n    B prefetch k={k}: {line}", flush=True)
    assert (line["n"], line["tile"], line["tiles_max"], line["parts"], line["tiles_part"]) == (10, T, 22, 0, 0)
    ds.free()


# ---- C: every extract instantiation -------------------------------------------------------------------------------------------------------
# 64-bit keys: (region_logb, k) -> extract_hi; HI <=> 2 (k - 1) >= 28 + logB (test_build_plan_policy.test_extract_hi_threshold); k = 9 has its
# 16 hash bits' top 9 | 10 in both arms (top_from_hl false); k = 5 is clamped to its 8 hash bits
FORCED64 = [(9, 19, 0), (9, 21, 1), (9, 9, 0), (10, 19, 0), (10, 21, 1), (10, 9, 0), (11, 19, 0), (11, 21, 1), (12, 19, 0), (12, 21, 1),
            (13, 21, 0), (13, 23, 1), (13, 5, 0)]
FORCED128 = [(logB, k, 0) for k in (33, 41, 63) for logB in (10, 11, 12, 13)]


def forced_streams():
    return [random_stream(61, 150_000), random_stream(62, 9_000)], [("forced", 0), ("forced", 1)]


@pytest.mark.parametrize("logB,k,hi", FORCED64 + FORCED128)
def test_every_extract_instantiation(E, logB, k, hi, capfd, monkeypatch):
    streams, keys = forced_streams()
    set_knob(monkeypatch, "region_logb", logB)
    ds, line, _ = build_checked(E, capfd, monkeypatch, streams, k, True, keys)
    with capfd.disabled():
        print(f"\n    C region_logb={logB} k={k}: {line}", flush=True)
    want_logB = min(logB, 2 * (k - 1))
    # the capacity follows the forced layout as usual; tiles of 8 192 from 2^12 regions on (and for 128-bit keys)
    assert (line["logB"], line["cap"], line["extract_hi"]) == (want_logB, capacity(150_000, want_logB), hi)
    assert line["tile"] == (TILE128 if k > 31 or want_logB >= 12 else TILE64) and line["tiles_max"] == -(-150_000 // line["tile"])
    ds.free()
    # one merge of the two through the sorted dictionaries of the same layout
    set_knob(monkeypatch, "sorted_dicts", 1)
    path = merge_checked(E, streams, k, True)
    assert path.startswith("sorted:"), path
    err = capfd.readouterr().err
    assert build_line(err)["logB"] == want_logB and build_line(err)["end"] == "per-region"
    del_knob(monkeypatch, "sorted_dicts")
    del_knob(monkeypatch, "region_logb")


# ---- D: every dedupe shape ----------------------------------------------------------------------------------------------------------------
def shape_for(cap):
    return next(s for s in SHAPES if cap <= s)


def dup_stream(seed, length):
    """`length` bytes, one region's worth: 70 % random, then its first 30 % again (the fold has work)"""
    rng = np.random.default_rng(seed)
    rep = (length * 3) // 10
    body = bases(rng, length - rep - 2)
    return np.concatenate([body, [ord("\n")], body[:rep], [ord("\n")]]).astype(np.uint8)


# stream lengths: inside each shape (capacities 1 472, 3 392, 4 032, 4 992, 6 080), at each shape's last capacity and the next one's first
DEDUPE_LENGTHS = [1000, 2600, 3100, 3900, 4800] + [longest_with_capacity(c) for c in SHAPES[:4]] + [longest_with_capacity(c) + 1 for c in SHAPES[:4]] + [4900]


def dedupe_hi_at(sort_cap, k, logB=0):
    lc = (sort_cap - 1).bit_length()
    return int(2 * (k - 1) - logB + 4 - lc >= 32)


@pytest.mark.parametrize("k", [19, 21, 23])
@pytest.mark.parametrize("length", DEDUPE_LENGTHS)
def test_every_dedupe_shape(E, length, k, capfd, monkeypatch):
    streams = [dup_stream(length, length), dup_stream(length + 1, length - 7), random_stream(3, 60 + k)]
    set_knob(monkeypatch, "sorted_dicts", 1)
    ds, line, _ = build_checked(E, capfd, monkeypatch, streams, k, True)
    del_knob(monkeypatch, "sorted_dicts")
    with capfd.disabled():
        print(f"\n    D length={length} k={k}: {line}", flush=True)
    cap = capacity(length, 0)
    sort_cap = -(-cap // 256) * 256
    assert (line["logB"], line["cap"], line["layout"], line["end"]) == (0, cap, "fixed", "per-region")
    assert (line["sort_cap"], line["shape"]) == (sort_cap, shape_for(cap))
    # k = 19 | 21 lie on either side of the HI test up to 4 096 words, 21 | 23 beyond (test_build_plan_policy.test_dedupe_hi_threshold)
    assert line["dedupe_hi"] == dedupe_hi_at(sort_cap, k) == {19: 0, 21: int(sort_cap <= 4096), 23: 1}[k]
    assert line["largest"] == length - 2 * k                                 # every window of both records: the repeat is there to fold
    ds.free()


@pytest.mark.parametrize("k", [41, 63])
@pytest.mark.parametrize("length", [1000, 3100])
def test_the_128_bit_counting_sort(E, length, k, capfd, monkeypatch):
    streams = [dup_stream(length, length), dup_stream(length + 1, length - 7), random_stream(3, 60 + k)]
    set_knob(monkeypatch, "sorted_dicts", 1)
    ds, line, _ = build_checked(E, capfd, monkeypatch, streams, k, True)
    del_knob(monkeypatch, "sorted_dicts")
    with capfd.disabled():
        print(f"\n    D wide length={length} k={k}: {line}", flush=True)
    cap = capacity(length, 0)                                                # 1 472 | 4 032
    assert (line["logB"], line["cap"], line["layout"], line["end"], line["sort_cap"]) == (0, cap, "fixed", "per-region", -(-cap // 256) * 256)
    ds.free()


def poly_a_bucket(k, logB):
    """the region of the window of k A's (its split k-mer is 0 -- A is code 0 -- and the smaller of the two strands)"""
    if logB == 0:
        return 0
    if k > 31:
        return int(np.argmax(wide_bucket_rows(np.zeros(1, np.uint64), np.zeros(1, np.uint64), k, logB)))
    return int(hash64(np.zeros(1, np.uint64), k)[0] >> np.uint64(2 * (k - 1) - logB))


def region_rows(keys, k, logB):
    """distinct split k-mers per region of one sample's dictionary"""
    if k > 31:
        return wide_bucket_rows(keys["lo"], keys["hi"], k, logB)
    return np.bincount((hash64(keys["lo"], k) >> np.uint64(2 * (k - 1) - logB)).astype(np.int64), minlength=1 << logB)


def repeat_stream(seed, total, k, logB, target):
    """`total` bytes: random bases, then a record of m A's -- m - k + 1 windows with one split k-mer, all in one region -- with m such that this
    region holds exactly `target` words.  The random part has no window twice (checked), so its windows per region are its dictionary's keys per
    region, counted with the engine's hash restated in numpy; a base more of A's is a window more in the region and a random window fewer
    somewhere, so the count grows by one or not at all with m and every target is met."""
    genome = bases(np.random.default_rng(seed), total)
    r = poly_a_bucket(k, logB)

    def count(m):
        body = genome[:total - m - 2]
        keys, _ = oracle_dict([body.tobytes()], k, True).export()
        assert len(keys) == len(body) - k + 1
        return int(region_rows(keys, k, logB)[r]) + m - k + 1
    lo, hi = k, total - 2 - 2 * k                                           # (a random part of exactly k bases would have no window: split_kmer.rs:89)
    assert count(lo) < target <= count(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if count(mid) >= target else (mid, hi)
    assert count(hi) == target
    return np.concatenate([genome[:total - hi - 2], [ord("\n")], np.full(hi, ord("A"), np.uint8), [ord("\n")]]).astype(np.uint8)


@pytest.mark.parametrize("spill_grid", [None, 1])
def test_two_shape_launch_lists_the_regions_above_the_typical_shape(E, spill_grid, capfd, monkeypatch):
    """12 000 bytes in 2^2 regions: capacity 3 904 words (8 x 512), the typical region 3 182 (7 x 512: test_build_plan_policy).  A run of A's
    takes one region of each of three samples to 3 700 words: above the typical shape, inside the capacity -- listed, and sorted by the second
    launch; with dedupe_spill_grid=1 that launch takes one listed region at a time"""
    k, total = 31, 12_000
    streams = [repeat_stream(40 + i, total - 9 * i, k, 2, 3700 + i) for i in range(3)] + [random_stream(44, 9_000)]
    set_knob(monkeypatch, "sorted_dicts", 1)
    if spill_grid:
        set_knob(monkeypatch, "dedupe_spill_grid", spill_grid)
    ds, line, err = build_checked(E, capfd, monkeypatch, streams, k, True)
    del_knob(monkeypatch, "dedupe_spill_grid")
    del_knob(monkeypatch, "sorted_dicts")
    with capfd.disabled():
        print(f"\n    D two shapes spill_grid={spill_grid}: {line} {LISTED.findall(err)}", flush=True)
    assert (line["logB"], line["cap"], line["layout"], line["end"], line["largest"]) == (2, 3904, "fixed", "per-region", 3702)
    assert (line["shape"], line["typical"], line["shape_typ"]) == (4096, 3182, 3584)
    listed = LISTED.findall(err)
    assert len(listed) == 1 and (int(listed[0][0]), int(listed[0][1]), int(listed[0][2]), int(listed[0][3])) == (3182, 4096, 3, 16)
    ds.free()


# ---- E: a region beyond its fixed capacity ------------------------------------------------------------------------------------------------
# 12 000 bytes: 2^2 regions of 3 904 words for both key widths (ceil(12 000 / 4 900) = 3, ceil(12 000 / 3 200) = 4; mean 3 001).  The per-region
# sort holds 6 144 words (4 096 for 128-bit keys).  case: (largest region, layout, how a build that sorts ends)
OVERFLOW = {
    "per_region": ({31: 5000, 41: 4000}, "exact", "per-region"),
    "sort_max": ({31: 6144, 41: 4096}, "exact", "per-region"),
    "flat": ({31: 6145, 41: 4097}, "exact", "flat"),
    "far_flat": ({31: 7000, 41: 6000}, "exact", "flat"),
    "at_capacity": ({31: 3904, 41: 3904}, "fixed", "extracted"),
    "capacity_plus_1": ({31: 3905, 41: 3905}, "exact", "per-region"),
}


@pytest.mark.parametrize("k", [31, 41])
@pytest.mark.parametrize("case", list(OVERFLOW))
def test_a_region_beyond_its_fixed_capacity(E, case, k, capfd, monkeypatch):
    targets, layout, end = OVERFLOW[case]
    streams = [repeat_stream(50, 12_000, k, 2, targets[k]), random_stream(51, 8_000)]
    ds, line, _ = build_checked(E, capfd, monkeypatch, streams, k, True)
    with capfd.disabled():
        print(f"\n    E {case} k={k}: {line}", flush=True)
    assert (line["logB"], line["cap"]) == (2, 3904)
    assert (line["layout"], line["largest"], line["end"]) == (layout, targets[k], end)
    ds.free()
    # merged with the ordinary sample: the append pass reads a region filled to its last word; the exact layout merges its sorted dictionaries
    path = merge_checked(E, streams, k, True)
    assert path.startswith("append") if layout == "fixed" else path.startswith("sorted:"), path
