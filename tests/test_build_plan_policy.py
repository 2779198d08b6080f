"""The host policy of the build stage (region_layout, region_capacity in csrc/skx_dictset.cpp; extract_parts, extract_hi, dedupe_shape_words,
dedupe_hi in csrc/skx_device.hip) through skx_debug_build_plan, a test hook of the library: host arithmetic only, no device.

Every expectation below is a number worked here from DESIGN.md and the code's comments, not taken from the hook:
  * regions: a sample's words go into 2^logB regions, logB = need = ceil(log2(ceil(longest / per))) with per = 4 900 windows a region (3 200 for
    128-bit keys) up to the ceiling 2^10 (2^11); longer samples keep the ceiling and their regions grow, until need - 5 passes it (32 row blocks
    a region), from where logB = need - 5 up to 2^13; beyond that the sort-based form takes the batch (logB = -1).  logB <= 2 (k - 1).
  * capacity of a region: mean = (longest >> logB) + 1 words, 20 % + 256 of head-room, rounded up to 64.
  * extraction: tiles of 12 288 positions (8 192 from 2^12 regions on, and for 128-bit keys); fewer than eight samples with 64 tiles and more
    are dealt to 8 // n XCDs each in ranges of ceil(tiles / parts) tiles; HI form when the bucket bits of a packed word ((H << 4) | mask) lie
    in its upper half: bits + 4 - 32 - logB >= 0, bits = 2 (k - 1).
  * dedupe: the capacity rounded up to 256 (512 at least) picks the launch shape 4 x 512 | 7 x 512 | 8 x 512 | 5 x 1 024 | 6 x 1 024 words; the
    typical region (mean + 3.3 sqrt(mean) + 1) may take a smaller one; HI form when the micro-bucket field, ceil(log2(cap)) bits below the
    region's own, and the sub-range field (sb = 4 bits) start at bit 32 or higher: rem_bits + 4 - lc >= 32 and rem_bits + 4 - sb >= 32,
    rem_bits = bits - logB.

tests/test_gpu_extract_edges.py takes its stream lengths from the helpers here."""
import ctypes

import numpy as np
import pytest

import skx_engine as E

FIELDS = ("logB", "cap", "tile", "tiles_max", "parts", "tiles_part", "extract_hi", "sort_cap", "shape", "typical", "shape_typ", "dedupe_hi",
          "dedupe_hi_typ", "flat")
SHAPES = (2048, 3584, 4096, 5120, 6144)          # words of <4,512> <7,512> <8,512> <5,1024> <6,1024>
TILE64, TILE128 = 12288, 8192


def plan(longest, n, k):
    """what a build of n assemblies, the longest a stream of `longest` bytes, is launched with (the hook's fields by name)"""
    lib = E.load_library()
    lib.skx_debug_build_plan.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.skx_debug_build_plan.restype = ctypes.c_int
    out = np.zeros(len(FIELDS), dtype=np.int64)
    assert lib.skx_debug_build_plan(longest, n, k, out.ctypes.data) == 0
    return dict(zip(FIELDS, (int(x) for x in out)))


def capacity(longest, logB):
    """the capacity rule restated: (mean + 20 % + 256) rounded up to 64"""
    mean = (longest >> logB) + 1
    return -(-(mean + mean // 5 + 256) // 64) * 64


def longest_with_capacity(cap, logB=0):
    """the longest stream whose regions have `cap` words at most (cap a multiple of 64)"""
    mean = (cap - 256) * 5 // 6
    while mean + 1 + (mean + 1) // 5 + 256 <= cap:
        mean += 1
    while mean + mean // 5 + 256 > cap:
        mean -= 1
    return ((mean - 1) << logB) + (1 << logB) - 1


# ---- regions ------------------------------------------------------------------------------------------------------------------------------
def test_logB_steps_64bit_keys():
    # need = ceil(log2(ceil(longest / 4 900))): 4 900 -> 0; 4 901 -> 2 regions' worth -> 1; 9 800 -> 1; 9 801 -> 3 -> 2
    for longest, logB in ((1, 0), (4900, 0), (4901, 1), (9800, 1), (9801, 2), (4900 * 512, 9), (4900 * 512 + 1, 10), (4900 * 1024, 10)):
        assert plan(longest, 1, 31)["logB"] == logB, longest
    # the ceiling: 2^10 regions from 4 900 x 1 024 = 5 017 600 on, until need - 5 > 10 <=> need = 16 <=> more than 4 900 x 2^15 = 160 563 200
    for longest, logB in ((5_017_601, 10), (20_000_000, 10), (160_563_200, 10), (160_563_201, 11),
                          (4900 * 65536, 11), (4900 * 65536 + 1, 12),           # need 17: 321 126 401
                          (4900 * 131072, 12), (4900 * 131072 + 1, 13),         # need 18: 642 252 801
                          (4900 * 262144, 13)):                                 # need 18 still: 1 284 505 600
        assert plan(longest, 1, 31)["logB"] == logB, longest
    # need 19: need - 5 = 14 regions' bits are more than the LDS histogram holds -> the sort-based form
    assert plan(4900 * 262144 + 1, 1, 31)["logB"] == -1
    # a short hash: logB <= 2 (k - 1); k = 5 has 8 hash bits, k = 7 has 12
    assert plan(4900 * 512, 1, 5)["logB"] == 8 and plan(4900 * 1024, 1, 5)["logB"] == 8
    assert plan(4900 * 1024, 1, 7)["logB"] == 10 and plan(200_000_000, 1, 7)["logB"] == 11 and plan(700_000_000, 1, 7)["logB"] == 12


def test_region_logb_knob_is_clamped_and_keeps_the_capacity_rule(monkeypatch):
    """SKX_KNOBS=region_logb=N: the layout of a long sample for a short one -- N clamped to the hash bits and to 2^13, capacity by the usual rule"""
    assert plan(150_000, 1, 31)["logB"] == 5                                  # ceil(150 000 / 4 900) = 31 -> 5
    # capacities of 150 000 bases: 2^9: mean 293 + 58 + 256 = 607 -> 640; 2^11: 74 + 14 + 256 = 344 -> 384; 2^12: 37 + 7 + 256 = 300 -> 320;
    # 2^13: 19 + 3 + 256 = 278 -> 320; 2^8 (k = 5: 8 hash bits): 586 + 117 + 256 = 959 -> 960; one region: 150 001 + 30 000 + 256 = 180 257 -> 180 288
    for forced, k, logB, cap, tile in ((9, 31, 9, 640, TILE64),
                                       (11, 31, 11, 384, TILE64), (12, 31, 12, 320, TILE128), (13, 31, 13, 320, TILE128), (20, 31, 13, 320, TILE128),
                                       (13, 5, 8, 960, TILE64), (13, 7, 12, 320, TILE128), (0, 31, 0, 180_288, TILE64), (13, 41, 13, 320, TILE128)):
        monkeypatch.setenv("SKX_KNOBS", f"region_logb={forced}")
        p = plan(150_000, 1, k)
        assert (p["logB"], p["cap"], p["tile"]) == (logB, cap, tile), (forced, k, p)
    monkeypatch.delenv("SKX_KNOBS")
    assert plan(150_000, 1, 31)["logB"] == 5


def test_logB_steps_128bit_keys():
    # 3 200 windows a region, ceiling 2^11 (3 200 x 2 048 = 6 553 600), growth again at need = 17: more than 3 200 x 65 536 = 209 715 200
    for longest, logB in ((3200, 0), (3201, 1), (3200 * 1024, 10), (3200 * 1024 + 1, 11), (3200 * 2048, 11), (3200 * 2048 + 1, 11),
                          (209_715_200, 11), (209_715_201, 12), (3200 * 131072, 12), (3200 * 131072 + 1, 13), (3200 * 262144, 13)):
        assert plan(longest, 1, 41)["logB"] == logB, longest
    assert plan(3200 * 262144 + 1, 1, 41)["logB"] == -1
    assert plan(3200 * 262144 + 1, 1, 33)["logB"] == -1 and plan(3200 * 262144, 1, 63)["logB"] == 13


def test_capacity_at_its_rounding():
    # mean 320: 320 + 64 + 256 = 640, a multiple of 64 as it stands; mean 321: 321 + 64 + 256 = 641 -> 704
    assert plan(319, 1, 31)["cap"] == 640 and plan(320, 1, 31)["cap"] == 704
    # the largest region of the 64-bit policy: mean 4 901 + 980 + 256 = 6 137 -> 6 144, what the per-region sort holds
    assert plan(4900, 1, 31)["cap"] == 6144 and plan(4900 * 1024, 1, 31)["cap"] == 6144
    # 128-bit keys: mean 3 201 + 640 + 256 = 4 097 -> 4 160.  (3 199 bases, mean 3 200: 3 200 + 640 + 256 = 4 096 exactly)
    assert plan(3199, 1, 41)["cap"] == 4096 and plan(3200, 1, 41)["cap"] == 4160
    # the mean is taken after the shift: 9 800 bases in two regions are 4 900 + 1
    assert plan(9800, 1, 31)["cap"] == 6144 and plan(9600, 1, 31)["cap"] == 6080      # 4 901 + 980 + 256 = 6 137 -> 6 144; 4 801 + 960 + 256 = 6 017 -> 6 080
    # the lengths the dedupe cases are built from: 1 000 -> 1 001 + 200 + 256 = 1 457 -> 1 472, ...
    for longest, cap in ((1000, 1472), (2600, 3392), (3100, 4032), (3900, 4992), (4800, 6080)):
        assert plan(longest, 1, 31)["cap"] == cap == capacity(longest, 0)
    # regions that grow: 6 Mbp in 2^10 regions are 5 859 + 1 words -> 5 860 + 1 172 + 256 = 7 288 -> 7 296
    p = plan(6_000_000, 1, 31)
    assert p["logB"] == 10 and p["cap"] == 7296 and p["flat"] == 1
    # ... and the first length beyond the per-region sort: mean 4 907 -> 4 907 + 981 + 256 = 6 144; mean 4 908 -> 6 145 -> 6 208
    assert plan(4907 * 1024 - 1, 1, 31)["flat"] == 0 and plan(4907 * 1024, 1, 31)["flat"] == 1
    assert plan(4907 * 1024, 1, 31)["cap"] == 6208


def test_the_helper_finds_each_capacitys_last_length():
    for cap in (640, 1472, 2048, 3584, 4096, 5120, 6144):
        longest = longest_with_capacity(cap)
        assert capacity(longest, 0) <= cap < capacity(longest + 1, 0)
    # worked: 2 048 -> mean + mean // 5 <= 1 792: mean 1 494 (1 494 + 298), not 1 495 (1 495 + 299 = 1 794) -> 1 493 bases
    assert [longest_with_capacity(c) for c in SHAPES[:4]] == [1493, 2773, 3199, 4053]
    assert longest_with_capacity(6144) == 4906


# ---- dedupe shapes ------------------------------------------------------------------------------------------------------------------------
def test_shape_boundaries():
    # (last length of a shape, its capacity) -> the shape; one base more -> the next capacity (64 more) and the next shape
    #  2 048: mean 1 494 -> 1 494 + 298 + 256 = 2 048           | mean 1 495 -> 2 050 -> 2 112
    #  3 584: mean 2 774 -> 2 774 + 554 + 256 = 3 584           | mean 2 775 -> 3 586 -> 3 648
    #  4 096: mean 3 200 -> 3 200 + 640 + 256 = 4 096           | mean 3 201 -> 4 097 -> 4 160
    #  5 120: mean 4 054 -> 4 054 + 810 + 256 = 5 120           | mean 4 055 -> 5 122 -> 5 184
    for longest, cap, shape, nxt in ((1493, 2048, 2048, 3584), (2773, 3584, 3584, 4096), (3199, 4096, 4096, 5120), (4053, 5120, 5120, 6144)):
        p, q = plan(longest, 1, 31), plan(longest + 1, 1, 31)
        assert (p["logB"], p["cap"], p["shape"]) == (0, cap, shape), p
        assert (q["logB"], q["cap"], q["shape"]) == (0, cap + 64, nxt), q
    assert plan(4900, 1, 31)["shape"] == 6144
    # the launch holds the capacity rounded up to 256 and 512 words at least
    assert plan(10, 1, 31)["cap"] == 320 and plan(10, 1, 31)["sort_cap"] == 512 and plan(10, 1, 31)["shape"] == 2048
    assert plan(1000, 1, 31)["sort_cap"] == 1536 and plan(4800, 1, 31)["sort_cap"] == 6144
    # 128-bit keys: one kernel form; the launch capacity is the rounded capacity, 4 096 at most
    assert plan(1000, 1, 41)["sort_cap"] == 1536 and plan(3100, 1, 41)["sort_cap"] == 4096 and plan(3100, 1, 41)["flat"] == 0


def test_the_typical_region_and_its_shape():
    # 2.4 Mbp: need = ceil(log2(490)) = 9; mean = 4 687 + 1; capacity 4 688 + 937 + 256 = 5 881 -> 5 888: 6 x 1 024
    # typical = 4 688 + 3.3 sqrt(4 688) + 1 = 4 688 + 225.95 + 1 -> 4 914: 5 x 1 024 -> the two-shape launch
    p = plan(2_400_000, 1, 31)
    assert (p["logB"], p["cap"], p["shape"], p["typical"], p["shape_typ"]) == (9, 5888, 6144, 4914, 5120)
    # 4 900 bases in one region: typical = 4 901 + 231.02 + 1 -> 5 133, beyond 5 x 1 024: one shape
    p = plan(4900, 1, 31)
    assert (p["typical"], p["shape"], p["shape_typ"]) == (5133, 6144, 6144)
    # 12 000 bases in 2^2 regions: mean 3 001 -> capacity 3 001 + 600 + 256 = 3 857 -> 3 904: 8 x 512; typical 3 001 + 180.78 + 1 -> 3 182: 7 x 512
    p = plan(12_000, 1, 31)
    assert (p["logB"], p["cap"], p["shape"], p["typical"], p["shape_typ"]) == (2, 3904, 4096, 3182, 3584)


# ---- extraction ---------------------------------------------------------------------------------------------------------------------------
def test_tiles():
    assert plan(786_432, 1, 31)["tile"] == TILE64 and plan(786_432, 1, 41)["tile"] == TILE128
    assert plan(200_000_000, 1, 31)["tile"] == TILE64 and plan(400_000_000, 1, 31)["tile"] == TILE128      # 2^11 | 2^12 regions
    for longest, tiles in ((1, 1), (12288, 1), (12289, 2), (63 * 12288, 63), (63 * 12288 + 1, 64), (64 * 12288, 64)):
        assert plan(longest, 1, 31)["tiles_max"] == tiles
    for longest, tiles in ((8192, 1), (8193, 2), (63 * 8192, 63), (64 * 8192, 64), (64 * 8192 + 1, 65)):
        assert plan(longest, 1, 63)["tiles_max"] == tiles


@pytest.mark.parametrize("k,tile", [(31, TILE64), (41, TILE128)])
def test_parts_table(k, tile):
    # 63 tiles: nobody is dealt
    for n in range(1, 9):
        p = plan(63 * tile, n, k)
        assert (p["tiles_max"], p["parts"], p["tiles_part"]) == (63, 0, 0), (n, p)
    # 64 tiles: 8 // n ranges a sample, none where that is one (n = 5, 6, 7) and none from eight samples on
    for n, parts, tiles_part in ((1, 8, 8), (2, 4, 16), (3, 2, 32), (4, 2, 32)):
        p = plan(64 * tile, n, k)
        assert (p["tiles_max"], p["parts"], p["tiles_part"]) == (64, parts, tiles_part), (n, p)
    for n in (5, 6, 7, 8, 9, 100):
        assert plan(64 * tile, n, k)["parts"] == 0, n
    # tiles_part rounds up: 67 tiles in 8 | 4 | 2 ranges are 9 | 17 | 34 (the last range is short: 4, 16 and 33 tiles), 65 in 8 are 9 (the last: 2)
    for tiles, n, tiles_part in ((67, 1, 9), (67, 2, 17), (67, 3, 34), (67, 4, 34), (65, 1, 9), (72, 1, 9), (73, 1, 10)):
        assert plan(tiles * tile, n, k)["tiles_part"] == tiles_part, (tiles, n)


def test_extract_hi_threshold():
    # bits + 4 - 32 - logB >= 0 <=> 2 (k - 1) >= 28 + logB.  Odd k on either side, per logB:
    #   logB 0: 28 -> k 13 (24) | 15 (28)        logB 9: 37 -> 19 (36) | 21 (40)       logB 10: 38 -> 19 | 21
    #   logB 11: 39 -> 19 | 21                   logB 12: 40 -> 19 (36) | 21 (40)      logB 13: 41 -> 21 (40) | 23 (44)
    for longest, logB, lo_k, hi_k in ((1000, 0, 13, 15), (2_400_000, 9, 19, 21), (5_000_000, 10, 19, 21), (200_000_000, 11, 19, 21),
                                      (400_000_000, 12, 19, 21), (700_000_000, 13, 21, 23)):
        a, b = plan(longest, 1, lo_k), plan(longest, 1, hi_k)
        assert a["logB"] == b["logB"] == logB
        assert (a["extract_hi"], b["extract_hi"]) == (0, 1), (logB, lo_k, hi_k)
    assert plan(1000, 1, 41)["extract_hi"] == 0                          # (128-bit keys: one form)


def test_dedupe_hi_threshold():
    # the micro-bucket field: rem_bits >= 28 + lc, lc = ceil(log2(launch capacity)).  At logB = 0, rem_bits = 2 (k - 1):
    #   launch capacity 1 536 (1 000 bases) or 2 048: lc 11 -> 39: k 19 (36) | 21 (40)
    #   2 304 .. 4 096: lc 12 -> 40: k 19 | 21 (40, just)
    #   4 352 .. 6 144: lc 13 -> 41: k 21 (40) | 23 (44)
    # the sub-range field: rem_bits >= 28 + sb = 32, implied by the first for every capacity (lc >= 9 > sb)
    for longest, sort_cap, lo_k, hi_k in ((1000, 1536, 19, 21), (1493, 2048, 19, 21), (1494, 2304, 19, 21), (3199, 4096, 19, 21),
                                          (3200, 4352, 21, 23), (4800, 6144, 21, 23)):
        a, b = plan(longest, 1, lo_k), plan(longest, 1, hi_k)
        assert a["sort_cap"] == b["sort_cap"] == sort_cap
        assert (a["dedupe_hi"], b["dedupe_hi"]) == (0, 1), (longest, lo_k, hi_k)
    # with 2^9 regions the region's own bits go off: 2.4 Mbp, launch capacity 5 888 (lc 13): rem_bits >= 41 <=> 2 (k - 1) >= 50: k 25 (48) | 27 (52)
    assert plan(2_400_000, 1, 25)["dedupe_hi"] == 0 and plan(2_400_000, 1, 27)["dedupe_hi"] == 1
    # ... and the typical shape's launch holds 5 120 words: lc 13 as well
    assert plan(2_400_000, 1, 25)["dedupe_hi_typ"] == 0 and plan(2_400_000, 1, 27)["dedupe_hi_typ"] == 1
    # 12 000 bases (above): capacity launch 4 096 (3 904 rounded: lc 12), typical launch 3 584 (lc 12): rem_bits = bits - 2 >= 40: k 21 (38) | 23 (42)
    p, q = plan(12_000, 1, 21), plan(12_000, 1, 23)
    assert (p["dedupe_hi"], p["dedupe_hi_typ"], q["dedupe_hi"], q["dedupe_hi_typ"]) == (0, 0, 1, 1)
    assert plan(1000, 1, 41)["dedupe_hi"] == 0                           # (128-bit keys: one form)


def test_the_hook_refuses_bad_arguments():
    lib = E.load_library()
    lib.skx_debug_build_plan.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.skx_debug_build_plan.restype = ctypes.c_int
    out = np.zeros(len(FIELDS), dtype=np.int64)
    assert lib.skx_debug_build_plan(1000, 1, 31, None) == E.EINVAL
    assert lib.skx_debug_build_plan(1000, 0, 31, out.ctypes.data) == E.EINVAL
    assert lib.skx_debug_build_plan(1000, 1, 30, out.ctypes.data) == E.EINVAL          # k must be odd (ska_dict.rs:342-344)
