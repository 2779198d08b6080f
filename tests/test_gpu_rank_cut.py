"""`ska align` over an array still held as the merge's pieces: the filter's statistics pass reads only the first-seen ranks that min_count
samples reach (pieces_cut_kernel + the bounded pieces_stats_kernel), the statistics themselves are counted when first asked for, and the
kept rows copy a sample's piece only up to the largest kept rank.  Every case is checked three ways: against the CPU oracle, against the
same run with SKX_KNOBS=stats_eager=1 (statistics in the merge, no bound, whole pieces), and on the alignment text.  Bit-exact throughout.

Why the bound is safe (and what the cases below try to break): a sample's piece of row block j holds exactly plen[j][s] ranks, so rank r has a
cell in at most #{s : plen[j][s] > r} samples; r_cut[j] = the min_count-th largest plen is the first r where that falls below min_count."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import del_knob, set_knob

import ora
from test_gpu_parity import as_map, build_both

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
NONE, NO_CONST, NO_AMBIG, NO_AMBIG_OR_CONST = 0, 1, 2, 3


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def rand_seq(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


def mutate(rng, seq, snps):
    s = np.frombuffer(seq, dtype=np.uint8).copy()
    pos = rng.integers(0, len(s), size=snps)
    s[pos] = ACGT[rng.integers(0, 4, size=snps)]
    return s.tobytes()


def related_set(seed, length, n, snps):
    """n samples from one ancestor, each with its own substitutions: the core rows get their ranks from the first samples, every later
    sample adds private rows behind them"""
    rng = np.random.default_rng(seed)
    anc = rand_seq(rng, length)
    return [[mutate(rng, anc, snps)] for _ in range(n)]


def late_core_set(seed):
    """16 small unrelated samples (one each for the sixteen waves of a row block, and none of the rows they bring is common), then 24 that
    share a core exactly and carry a private record each: the common rows arrive late, behind ranks that no filter keeps"""
    rng = np.random.default_rng(seed)
    core = rand_seq(rng, 8000)
    return [[rand_seq(rng, 1500)] for _ in range(16)] + [[core, rand_seq(rng, 300)] for _ in range(24)]


def boundary_set(seed):
    rng = np.random.default_rng(seed)
    base, contig = rand_seq(rng, 9000), rand_seq(rng, 1200)
    return [[base] for _ in range(10)] + [[base, contig] for _ in range(10)]


def columns(text):
    return sorted(zip(*text.decode().splitlines()[1::2]))


def three_ways(E, monkeypatch, samples, k, min_count, amb=False, ft=NO_CONST, mask=False, gaps=False, rc=True):
    """filter at min_count: engine == oracle == engine with stats_eager, keys / cells / counts / removed / alignment -> (cut, removed, rows before, rows after)"""
    ctx = E.default_context()
    ga, oa = build_both(E, samples, k, rc)
    assert ctx.merge_path().startswith("append"), ctx.merge_path()
    U = ga.nrows
    rg = ga.filter(min_count, amb, ft, mask, gaps, True)
    cut = ctx.filter_cut()
    ro = oa.filter(min_count, amb, ft, mask, gaps, True)
    print(f"k={k} S={len(samples)} min_count={min_count} amb={amb} ft={ft} mask={mask} gaps={gaps}: rows {U} -> {ga.nrows} (oracle {oa.nrows}), "
          f"removed {rg} (oracle {ro}), cut ranks/blocks {cut}")
    got = as_map(*ga.export())
    assert rg == ro and ga.nrows == oa.nrows
    assert got == as_map(*oa.export())
    text = ga.fasta()
    assert columns(text) == columns(oa.fasta())
    set_knob(monkeypatch, "stats_eager", 1)
    try:
        names = [f"s{i}" for i in range(len(samples))]
        gb = E.DictSet.build([E.record_stream(r) for r in samples], k, rc).merge(names)
        rb = gb.filter(min_count, amb, ft, mask, gaps, True)
        assert ctx.filter_cut() == (0, 0)
        assert rb == rg and as_map(*gb.export()) == got and gb.fasta() == text
    finally:
        del_knob(monkeypatch, "stats_eager")
    return cut, rg, U, ga.nrows


# ---- the bound at work ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,length", [(15, 12_000), (15, 20_000), (41, 12_000)])
def test_related_set_the_cut_is_active(E, monkeypatch, k, length):
    samples = related_set(100 + k + length, length, 40, 25)
    cut, removed, U, kept = three_ways(E, monkeypatch, samples, k, 36)          # ceil(0.9 * 40)
    assert cut[0] > 0 and cut[1] > 0
    assert 0 < kept < U


def test_related_set_through_align_at_the_default_frequency(E):
    samples = related_set(115, 12_000, 40, 25)
    ga, oa = build_both(E, samples, 15, True)
    g, o = ga.align(min_freq=0.9), oa.align(min_freq=0.9)
    assert E.default_context().filter_cut()[0] > 0
    assert columns(g) == columns(o) and len(columns(g)) > 0


def test_common_rows_that_arrive_late(E, monkeypatch):
    samples = late_core_set(7)
    cut, removed, U, kept = three_ways(E, monkeypatch, samples, 15, 24, ft=NONE)     # the core rows reach 24 exactly
    assert kept >= 7000 and kept < U and cut[0] > 0
    cut, removed, U, kept = three_ways(E, monkeypatch, samples, 15, 25, ft=NONE)     # one more: they all go
    assert kept == 0 and removed == U


def test_boundary_of_the_bound(E, monkeypatch):
    samples = boundary_set(3)
    _, _, U, kept10 = three_ways(E, monkeypatch, samples, 15, 10, ft=NONE)           # the contig's rows: in ten samples
    assert kept10 == U
    cut, _, _, kept11 = three_ways(E, monkeypatch, samples, 15, 11, ft=NONE)
    # (how many ranks the bound leaves unread here is not asserted: the sixteen waves of a row block take the twenty samples side by side, so
    # the contig's rows get their ranks in the order the waves arrive -- the bound holds for whatever lengths result, which is what is checked)
    assert 0 < kept11 < kept10 and kept10 - kept11 >= 1100


# ---- degenerate cuts ------------------------------------------------------------------------------------------------------------------
def test_identical_samples_nothing_is_skipped(E, monkeypatch):
    rng = np.random.default_rng(5)
    seq = rand_seq(rng, 7000)
    cut, removed, U, kept = three_ways(E, monkeypatch, [[seq] for _ in range(6)], 15, 6, ft=NONE)
    assert cut == (0, 0) and removed == 0 and kept == U


def test_unrelated_samples_everything_goes(E, monkeypatch):
    rng = np.random.default_rng(6)
    samples = [[rand_seq(rng, 5000)] for _ in range(12)]
    cut, removed, U, kept = three_ways(E, monkeypatch, samples, 15, 11)               # ceil(0.9 * 12)
    assert kept == 0 and removed == U


@pytest.mark.parametrize("S,min_count", [(1, 1), (2, 2), (17, 16), (17, 17)])
def test_few_samples(E, monkeypatch, S, min_count):
    samples = related_set(40 + S, 6000, S, 20)
    cut, _, _, _ = three_ways(E, monkeypatch, samples, 15, min_count)
    if min_count < 2:
        assert cut == (0, 0)


@pytest.mark.parametrize("min_count", [0, 1])
def test_counts_below_two_take_the_full_pass(E, monkeypatch, min_count):
    samples = related_set(77, 6000, 12, 20)
    cut, _, _, _ = three_ways(E, monkeypatch, samples, 15, min_count)
    assert cut == (0, 0)


def test_min_count_beyond_the_samples(E, monkeypatch):
    samples = related_set(78, 6000, 12, 20)
    cut, removed, U, kept = three_ways(E, monkeypatch, samples, 15, 13, ft=NONE)
    assert kept == 0 and removed == U and cut[0] > 0


# ---- every combination the filter takes -----------------------------------------------------------------------------------------------
def ambiguous_set(seed, n=40):
    """a related set with a sample that folds two bases into one cell (the same flanks around different middles) and a palindromic
    split k-mer (its two strands name one row: W / S)"""
    rng = np.random.default_rng(seed)
    samples = related_set(seed, 6000, n, 20)
    flank_l, flank_r = rand_seq(rng, 7), rand_seq(rng, 7)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    # (a record of exactly k bases yields no split k-mer: two bases of padding on either side)
    samples[3] += [b"GA" + flank_l + b"A" + flank_r + b"TC", b"CT" + flank_l + b"G" + flank_r + b"AG"]      # A and G between the same flanks: R (Y on the other strand)
    samples[9].append(b"GA" + flank_l + b"A" + flank_l.translate(comp)[::-1] + b"TC")                        # flanks that are each other's reverse complement: W
    for s in samples[5:]:
        s.append(b"GA" + flank_l + b"A" + flank_r + b"TC")
    return samples


@pytest.mark.parametrize("ft", [NONE, NO_CONST, NO_AMBIG, NO_AMBIG_OR_CONST])
@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("mask", [False, True])
def test_every_filter_combination(E, monkeypatch, ft, gaps, mask):
    cut, _, U, kept = three_ways(E, monkeypatch, ambiguous_set(21), 15, 36, ft=ft, mask=mask, gaps=gaps)
    assert cut[0] > 0 and 0 < kept < U


@pytest.mark.parametrize("ft", [NONE, NO_CONST, NO_AMBIG, NO_AMBIG_OR_CONST])
@pytest.mark.parametrize("mask", [False, True])
def test_ambiguous_as_missing_takes_the_full_pass(E, monkeypatch, ft, mask):
    """the silent rows (no unambiguous cell at all) are told by the unambiguous count of EVERY row, and `removed` leaves them out"""
    cut, removed, U, kept = three_ways(E, monkeypatch, ambiguous_set(21), 15, 36, amb=True, ft=ft, mask=mask)
    assert cut == (0, 0)


def _stats_direct_child():
    """runs in a process of its own (the knob is read once per process): per-rank stores fill no zeros, so the pass is not bounded there"""
    import skx_engine as eng
    eng.load_library()
    ctx = eng.default_context()
    samples = related_set(115, 12_000, 40, 25)
    ga, oa = build_both(eng, samples, 15, True)
    rg, ro = ga.filter(36, False, NO_CONST, False, False, True), oa.filter(36, False, NO_CONST, False, False, True)
    assert ctx.filter_cut() == (0, 0), ctx.filter_cut()
    assert rg == ro and as_map(*ga.export()) == as_map(*oa.export())
    assert columns(ga.fasta()) == columns(oa.fasta())
    gu, ou = build_both(eng, samples[:9], 15, True)
    assert as_map(*gu.export()) == as_map(*ou.export())
    print("stats_direct ok")


def test_stats_direct_knob_is_not_bounded():
    env = dict(os.environ, SKX_KNOBS="stats_direct=1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "stats_direct"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "stats_direct ok" in r.stdout, r.stdout + r.stderr


# ---- statistics on demand -------------------------------------------------------------------------------------------------------------
def _read_u32(ptr, n):
    hip = ctypes.CDLL("libamdhip64.so.7")                       # the runtime the engine itself is linked against (already mapped)
    out = np.zeros(n, np.uint32)
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(int(ptr)), ctypes.c_size_t(out.nbytes), 2) == 0     # hipMemcpyDeviceToHost
    return out


def _oracle_stats(var):
    """(present, unambiguous, code set) per row from the oracle's cells, as the engine encodes them (bit c of the set: IUPAC code c occurs)"""
    code = np.zeros(256, np.uint32)
    for ch, c in zip(b"-ACMTWYHGRSVKDBN", range(16)):
        code[ch] = c
    c = code[var]
    present = (c != 0).sum(axis=1)
    unambig = np.isin(c, [1, 2, 4, 8]).sum(axis=1)
    mask = np.zeros(len(var), np.uint32)
    for v in range(1, 16):
        mask |= np.where((c == v).any(axis=1), np.uint32(1 << v), np.uint32(0))
    return present, unambig, mask


@pytest.fixture(scope="module")
def demand(E):
    samples = ambiguous_set(33, 20)
    oa = ora.Array.from_dicts([_odict(r, 15) for r in samples], [f"s{i}" for i in range(len(samples))])
    return samples, oa, oa.export()


def _odict(recs, k):
    d = ora.Dict.new(k, True)
    for r in recs:
        d.add_record(r)
    return d


def _fresh(E, samples, k=15):
    return E.DictSet.build([E.record_stream(r) for r in samples], k, True).merge([f"s{i}" for i in range(len(samples))])


def test_on_demand_export_with_and_without_cells(E, demand):
    samples, oa, (ok, ov, oc) = demand
    ga = _fresh(E, samples)
    assert ga.pieces_info()[0] > 0                               # still held as the merge left it, nothing counted yet
    keys, counts = ga.export_keys()
    assert np.array_equal(keys, ok) and np.array_equal(counts, oc)
    assert as_map(*_fresh(E, samples).export()) == as_map(ok, ov, oc)


def test_on_demand_export_after_the_matrix_dropped_the_pieces(E, demand):
    samples, oa, (ok, ov, oc) = demand
    ga = _fresh(E, samples)
    ga.device_matrix()
    assert ga.pieces_info()[0] == 0
    assert as_map(*ga.export()) == as_map(ok, ov, oc)
    gb = _fresh(E, samples)
    gb.device_matrix()
    keys, counts = gb.export_keys()
    assert np.array_equal(keys, ok) and np.array_equal(counts, oc)


def test_on_demand_skf_save_and_reload(E, demand, tmp_path):
    samples, oa, (ok, ov, oc) = demand
    for how in ("save", "save_skf"):
        ga = _fresh(E, samples)
        p = str(tmp_path / how)
        if how == "save":
            ga.save(p + ".skf")
        else:
            ga.save_skf(p)
        assert as_map(*ora.Array.load(p + ".skf").export()) == as_map(ok, ov, oc)
        assert as_map(*E.Array.load(p + ".skf").export()) == as_map(ok, ov, oc)


def test_on_demand_device_stats(E, demand):
    samples, oa, (ok, ov, oc) = demand
    ga = _fresh(E, samples)
    U = ga.nrows
    pres, unamb, mask, vc = [_read_u32(p, U) for p in ga.device_stats()]
    assert ga.pieces_info()[0] > 0                               # (statistics only: the array stays over its pieces)
    want = sorted(zip(*[x.tolist() for x in _oracle_stats(ov)]))
    assert sorted(zip(pres.tolist(), unamb.tolist(), mask.tolist())) == want
    assert np.array_equal(vc, pres)
    assert (unamb < pres).any()                                  # the folded cell and the palindrome are there


def test_on_demand_distance_filtered(E, demand):
    samples, _, _ = demand
    names = [f"s{i}" for i in range(len(samples))]
    for min_freq, filt in ((0.9, True), (0.5, False)):          # (the table's two filters act on the array itself: a fresh pair each)
        ga, oa = _fresh(E, samples), ora.Array.from_dicts([_odict(r, 15) for r in samples], names)
        assert ga.distance_tsv(min_freq=min_freq, filt_ambig=filt) == oa.distance_tsv(min_freq=min_freq, filt_ambig=filt)
    # the entry point itself, straight after the merge, against the oracle's two filters (generic_modes.rs:136-189: rows below the count go
    # first, then the constant ones, which are counted) and its pair counts over what is left
    for min_freq, filt in ((0.9, True), (0.0, False)):
        pairs, constant, rows = _fresh(E, samples).distance_filtered(min_freq, filt)
        oa = ora.Array.from_dicts([_odict(r, 15) for r in samples], names)
        thr = int(np.ceil(len(samples) * min_freq)) if len(samples) * min_freq >= 1.0 else 0
        oa.filter(thr, False, NONE, False, False, False)
        oc = oa.filter(0, False, NO_CONST, False, False, False)
        od = oa.distance(oc, filt)
        assert constant == oc and rows == oa.nrows and rows > 0
        assert np.array_equal(pairs["match_count"], od["match_count"]) and np.array_equal(pairs["mismatch_count"], od["mismatch_count"])
        assert np.allclose(pairs["distance"], od["distance"], rtol=0, atol=1e-6)
        assert np.allclose(pairs["mismatch_prop"], od["mismatch_prop"], rtol=0, atol=1e-9)


def test_on_demand_sample_kmers(E, demand):
    samples, oa, (ok, ov, oc) = demand
    ga = _fresh(E, samples)
    assert list(ga.sample_kmers()) == [int(x) for x in (ov != ord("-")).sum(axis=0)]


def test_filter_after_the_statistics_were_asked_for(E, demand):
    """counted in full first (device_stats), filtered second: the full pass's numbers serve, nothing is bounded"""
    samples, oa0, _ = demand
    ga, oa = build_both(E, samples, 15, True)
    ga.device_stats()
    assert ga.filter(18, False, NO_CONST, False, False, True) == oa.filter(18, False, NO_CONST, False, False, True)
    assert E.default_context().filter_cut() == (0, 0)
    assert as_map(*ga.export()) == as_map(*oa.export())


# ---- the cut kernel alone -------------------------------------------------------------------------------------------------------------
def _pieces_cut(E, ctx, plen, cap, min_count):
    """skx_debug_pieces_cut (a test hook of the library, not in include/skx.h): per row of plen its min_count-th largest value, 0 past the samples"""
    lib = E.load_library()
    lib.skx_debug_pieces_cut.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.skx_debug_pieces_cut.restype = ctypes.c_int
    plen = np.ascontiguousarray(plen, np.uint16)
    out = np.zeros(plen.shape[0], np.uint32)
    assert lib.skx_debug_pieces_cut(ctx.h, plen.ctypes.data, plen.shape[1], plen.shape[0], cap, min_count, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("S", [1, 63, 64, 65, 1000])
def test_cut_kernel_against_a_sort(E, S):
    ctx = E.default_context()
    rng = np.random.default_rng(S)
    for cap in (128, 6016):
        plen = rng.integers(0, cap + 1, size=(37, S)).astype(np.uint16)
        plen[1] = 0                                              # no rank at all
        plen[2] = cap                                            # all ties, at the top
        plen[3] = rng.integers(0, 3, size=S)                     # ties and zeros
        plen[4, : S // 2] = 0
        plen[5] = np.sort(plen[5])                               # growing with the sample, as a merge leaves them
        for mc in sorted({1, 2, S // 2, S - 1, S, S + 1, 60_000} - {0}):
            want = np.sort(plen.astype(np.uint32), axis=1)[:, ::-1][:, mc - 1] if mc <= S else np.zeros(len(plen), np.uint32)
            assert np.array_equal(_pieces_cut(E, ctx, plen, cap, mc), want), (S, cap, mc)


if __name__ == "__main__" and sys.argv[1:] == ["stats_direct"]:
    _stats_direct_child()
