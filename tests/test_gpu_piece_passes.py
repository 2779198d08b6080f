"""The three passes `ska align` makes over the merge's pieces, at the edges of how they now divide their work:
  * pieces_stats_kernel gives the waves of a workgroup that have no 16-byte columns a slice of the samples instead (P = 4, 2 or 1 slices for
    <= 64, 65-128 or more columns) and sums the slices' counters through LDS; a bounded pass takes its block's cut itself (pieces_cut_block);
  * pieces_rows_kernel (kept rows, and every row: .skf save, export, the device matrix) loads a wave's piece lengths 64 at a time and has the
    next sample's piece on its way while it writes the current one's cells.
Every filter case is checked as tests/test_gpu_rank_cut.py's three_ways does: engine == oracle == engine with stats_eager=1 on keys, cells,
counts, `removed` and the alignment text, bit-exact."""
import ctypes
import math

import numpy as np
import pytest

import ora
from test_gpu_parity import as_map, build_both
from test_gpu_rank_cut import ambiguous_set, late_core_set, related_set, three_ways

pytestmark = pytest.mark.gpu

NONE, NO_CONST = 0, 1


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def fresh(E, samples, k=15):
    return E.DictSet.build([E.record_stream(r) for r in samples], k, True).merge([f"s{i}" for i in range(len(samples))])


def count_for(S):
    return max(2, math.ceil(0.9 * S))


# ---- every split of the samples over the waves ----------------------------------------------------------------------------------------
def clean_start_set(seed, length, n, snps, clean):
    """a related set whose first `clean` samples are the ancestor itself: the private rows of the others (which decide how many row blocks
    there are) all get ranks behind the core, so a block's cut sits at its share of the core"""
    samples = related_set(seed, length, n, snps)
    rng = np.random.default_rng(seed)
    anc = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=length)].tobytes()      # (related_set's ancestor: the same first draw)
    return [[anc] for _ in range(clean)] + samples[clean:]


# 40 related samples at k = 15, min_count 36: the columns a block keeps below its cut are about (rows below the cut / row blocks / 32); the
# three sets put them at <= 64 (four slices), 65-128 (two) and > 128 (one), 8 columns and more away from 64 and 128.  Measured once
# and pinned (the figure is printed): 10 kbp with sixteen clean samples ahead of 24 with 60 SNPs each; 40 kbp with 25 SNPs; 38 kbp with 2.
@pytest.mark.parametrize("length,snps,clean,lo,hi", [(10_000, 60, 16, 8, 56), (40_000, 25, 0, 72, 120), (38_000, 2, 0, 136, 188)])
def test_every_split(E, monkeypatch, length, snps, clean, lo, hi):
    samples = clean_start_set(500 + length // 1000 + snps, length, 40, snps, clean)
    blocks = fresh(E, samples).pieces_info()[1]
    assert blocks > 0
    cut, removed, U, kept = three_ways(E, monkeypatch, samples, 15, 36)
    cols = (U - cut[0]) / blocks / 32
    print(f"length {length} snps {snps} clean {clean}: rows {U}, kept {kept}, row blocks {blocks}, cut {cut}, columns read per block {cols:.1f}")
    assert cut[0] > 0 and 0 < kept < U
    assert lo <= cols <= hi, cols


# ---- slices with nothing or little to do, and the fold cadences -----------------------------------------------------------------------
@pytest.mark.parametrize("S,length,snps", [(1, 6000, 20), (2, 6000, 20), (3, 6000, 20), (5, 6000, 20), (63, 6000, 20), (64, 6000, 20), (65, 6000, 20),
                                           (130, 6000, 5), (260, 6000, 5), (800, 3000, 2)])
def test_slices_and_folds(E, monkeypatch, S, length, snps):
    """S < 64: slices 1-3 have no sample; 65 and 130: the last slices have one group or none; 260: every slice a group, the first a second one
    of four samples; 800 at four slices: a slice passes its nibble folds (12 samples) and its byte fold (192)"""
    samples = related_set(900 + S, length, S, snps)
    cut, removed, U, kept = three_ways(E, monkeypatch, samples, 15, count_for(S))
    if S >= 40:
        assert cut[0] > 0 and 0 < kept < U


# ---- the unbounded pass through the split ---------------------------------------------------------------------------------------------
def test_unfiltered_export_counts_every_rank(E):
    samples = ambiguous_set(61)
    ga, oa = build_both(E, samples, 15, True)
    print("pieces (bytes, row blocks, ranks per block):", ga.pieces_info())
    assert as_map(*ga.export()) == as_map(*oa.export())


@pytest.mark.parametrize("min_count", [0, 1])
def test_full_pass_of_a_filter_below_two(E, monkeypatch, min_count):
    cut, _, _, _ = three_ways(E, monkeypatch, ambiguous_set(62), 15, min_count)
    assert cut == (0, 0)


@pytest.mark.parametrize("mask", [False, True])
def test_ambiguous_as_missing_code_sets_behind_the_combine(E, monkeypatch, mask):
    """the code sets of rows with an ambiguous cell come from the all-wave walk that follows the slices' sum"""
    cut, removed, U, kept = three_ways(E, monkeypatch, ambiguous_set(63), 15, 36, amb=True, ft=NONE, mask=mask)
    assert cut == (0, 0) and 0 < kept < U


# ---- 128-bit keys: 3 072 ranks a block, 96 columns ------------------------------------------------------------------------------------
def test_k41_filtered_and_unfiltered(E, monkeypatch):
    samples = related_set(141, 12_000, 40, 25)
    ga, oa = build_both(E, samples, 41, True)
    print("pieces (bytes, row blocks, ranks per block):", ga.pieces_info())
    assert as_map(*ga.export()) == as_map(*oa.export())
    cut, removed, U, kept = three_ways(E, monkeypatch, samples, 41, 36)
    assert cut[0] > 0 and 0 < kept < U


# ---- kept rows: the ends of the pipeline ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 8, 9, 17, 40])
@pytest.mark.parametrize("mask", [False, True])
def test_kept_rows_few_samples_a_wave(E, monkeypatch, S, mask):
    """eight waves a workgroup: S = 1, 2, 8, 9, 17 leave a wave 0, 1, 2 or 3 samples; at 40 the samples of a workgroup halve"""
    samples = related_set(300 + S, 6000, S, 20)
    cut, removed, U, kept = three_ways(E, monkeypatch, samples, 15, max(1, math.ceil(0.9 * S)), ft=NONE, mask=mask)
    assert kept > 0


@pytest.mark.parametrize("mask", [False, True])
def test_kept_rows_short_and_empty_pieces(E, monkeypatch, mask):
    """sixteen unrelated samples first: in the blocks' kept ranks their pieces are shorter than the largest kept rank, some of length 0"""
    cut, removed, U, kept = three_ways(E, monkeypatch, late_core_set(11), 15, 24, ft=NONE, mask=mask)
    assert kept >= 7000 and kept < U and cut[0] > 0


@pytest.mark.parametrize("mask", [False, True])
def test_kept_rows_with_ambiguous_cells(E, monkeypatch, mask):
    cut, removed, U, kept = three_ways(E, monkeypatch, ambiguous_set(64), 15, 36, ft=NONE, mask=mask)
    assert cut[0] > 0 and 0 < kept < U


def test_kept_rows_end_in_a_partial_dword(E, monkeypatch):
    """a kept-row count that is no multiple of four: blocks whose first output column is unaligned, and a 1-3 byte tail"""
    cut, removed, U, kept = three_ways(E, monkeypatch, related_set(537, 12_000, 40, 25), 15, 36)
    print(f"rows {U}, kept {kept}, cut {cut}")
    assert kept % 4 != 0 and cut[0] > 0


# ---- every row (pieces_rows_kernel<false>): .skf save, the device matrix, export ---------------------------------------------------------
def test_all_rows_save_load_matrix_export(E, tmp_path):
    samples = related_set(71, 12_000, 40, 25)
    ga, oa = build_both(E, samples, 15, True)
    want = as_map(*oa.export())
    p = str(tmp_path / "all.skf")
    ga.save(p)                                                     # (streams the rows a window of row blocks at a time)
    assert as_map(*ora.Array.load(p).export()) == want
    assert as_map(*E.Array.load(p).export()) == want
    gb = fresh(E, samples)
    assert gb.pieces_info()[0] > 0
    gb.device_matrix()                                             # (every row at once; the pieces are dropped)
    assert gb.pieces_info()[0] == 0
    assert as_map(*gb.export()) == want
    assert as_map(*fresh(E, samples).export()) == want


# ---- the cut alone ----------------------------------------------------------------------------------------------------------------------
def pieces_cut(E, ctx, plen, cap, min_count):
    """skx_debug_pieces_cut (a test hook of the library, not in include/skx.h): per row of plen its min_count-th largest value, 0 past the samples"""
    lib = E.load_library()
    lib.skx_debug_pieces_cut.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.skx_debug_pieces_cut.restype = ctypes.c_int
    plen = np.ascontiguousarray(plen, np.uint16)
    out = np.zeros(plen.shape[0], np.uint32)
    assert lib.skx_debug_pieces_cut(ctx.h, plen.ctypes.data, plen.shape[1], plen.shape[0], cap, min_count, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("S", [1, 7, 256, 257, 1000])
@pytest.mark.parametrize("cap", [128, 6016])
def test_cut_hook_against_numpy(E, S, cap):
    ctx = E.default_context()
    rng = np.random.default_rng(1000 * S + cap)
    plen = rng.integers(0, cap + 1, size=(19, S)).astype(np.uint16)
    plen[1] = rng.integers(0, cap + 1)                               # all lengths equal
    plen[2] = cap                                                    # all equal to cap
    plen[3] = 0
    plen[4] = np.sort(plen[4])                                       # growing with the sample, as a merge leaves them
    plen[5] = np.minimum(plen[5], 3)                                 # ties in the lowest bins
    plen[6] = np.maximum(plen[6], cap - 2)                           # ties in the highest
    desc = np.sort(plen.astype(np.uint32), axis=1)[:, ::-1]
    for mc in (1, 2, S, S + 1):
        want = desc[:, mc - 1] if mc <= S else np.zeros(len(plen), np.uint32)
        assert np.array_equal(pieces_cut(E, ctx, plen, cap, mc), want), (S, cap, mc)
