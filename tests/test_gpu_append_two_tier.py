"""The two tiers of the 64-bit append pass (append_kernel<false, HI, TT> in skx_append.hip): rows met first live in the LDS table, rows first
met after that table was closed live in the workgroup's table in global memory, and cells of ranks beyond a wave's row buffer go through the
wave's list and are OR-ed into the finished piece.

Production reaches this form only where a thousand related samples let the split go one step coarser (two_tier_plan in skx_merge.cpp).  The
tests reach it with SKX_KNOBS=append_lds_ranks=N: every attempt runs with two tiers at whatever split it has, the waves meet after every
sample, and the LDS tier closes at the first meeting that finds N rows (N = 1: closed before the first row -- the only way to close it for
fewer than 32 samples, where no meeting has all sixteen waves).  SKX_KNOBS=append_coarse=1 on top gives blocks with more ranks than a row
buffer covers (5 760), which is what the lists are for.

Every case, bit for bit: keys, cells, counts, sample_kmers and a filtered alignment (min_freq 0.9, no-const) against the CPU oracle, the
sorted path (SKX_KNOBS=sorted_dicts=1) and the one-tier pass (SKX_KNOBS=append_two_tier=0); the shape -- split, readers per region, what
closed and what went to tier 2 -- is asserted from the pass's own SKX_DEBUG lines.  No tolerances."""
import re

import numpy as np
import pytest
from conftest import set_knob, del_knob

import ora
from test_gpu_parity import oracle_dict
from test_gpu_append_shapes import (ACGT, L, append_lines, check_parity, columns, engine_merge, genome, related, rows_of, same_rows, unrel)

pytestmark = pytest.mark.gpu

TT_LINE = re.compile(r"\[skx\] append two tiers: (\w+) split, lds_ranks=(\d+) close_at=(\d+) meet_every=(\d+) closed_blocks=(\d+) of (\d+) "
                     r"lds_rows=(\d+) last_close_meeting=(\d+) tier2_rows=(\d+) list_flushes=(\d+)")
TT_KEYS = ("split", "lds_ranks", "close_at", "meet_every", "closed_blocks", "blocks", "lds_rows", "last_close_meeting", "tier2_rows", "list_flushes")


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def tt_lines(err):
    return [{k: (v if k == "split" else int(v)) for k, v in zip(TT_KEYS, m)} for m in TT_LINE.findall(err)]


def clades(rng, length, n, private, late_shared, cut=2):
    """n related samples; the second half carries late_shared SNPs of its own clade (first seen after the first sixteen samples) besides `private` ones each"""
    anc = genome(rng, length)
    late = anc.copy()
    pos = rng.choice(length, size=late_shared, replace=False)
    late[pos] = ACGT[(np.searchsorted(ACGT, late[pos]) + 1 + rng.integers(0, 3, size=late_shared)) % 4]
    out = []
    for i in range(n):
        s = (anc if i < n // 2 else late).copy()
        p = rng.integers(0, length, size=private)
        s[p] = ACGT[rng.integers(0, 4, size=private)]
        b = s.tobytes()
        step = (length + cut - 1) // cut
        out.append([b[j:j + step] for j in range(0, length, step)])
    return out


def odd_samples(rng, k):
    """a sample that is one repeat, the all-zero key (poly-A), self-palindromic windows, one flank pair around four different middle bases"""
    unit = genome(rng, k + 9).tobytes()
    var = bytearray(unit * 50)
    for p in range(k // 2, len(var), len(unit)):
        var[p] = b"ACGT"[(p // len(unit)) % 4]
    return [[b"A" * 700, unit * 8], [b"AT" * 300], [b"ACGT" * 150, b"A" * 100], [bytes(var)]]


def run_case(E, capfd, monkeypatch, samples, k, lds_ranks, coarse=0):
    """the merge with two tiers (its debug lines returned) against the oracle, the sorted path and the one-tier pass"""
    monkeypatch.setenv("SKX_DEBUG", "1")
    names = [f"s{i}" for i in range(len(samples))]
    set_knob(monkeypatch, "append_two_tier", 0)
    capfd.readouterr()
    g0 = engine_merge(E, samples, k, True, names)
    err0 = capfd.readouterr().err
    base = (rows_of(g0), list(g0.sample_kmers()), columns(engine_merge(E, samples, k, True, names).align(filter_type=E.FILTER_NO_CONST, min_freq=0.9)))
    assert E.default_context().merge_path() == "append64" and not tt_lines(err0)
    del_knob(monkeypatch, "append_two_tier")
    set_knob(monkeypatch, "append_lds_ranks", lds_ranks)
    if coarse:
        set_knob(monkeypatch, "append_coarse", coarse)
    capfd.readouterr()
    ga = engine_merge(E, samples, k, True, names)
    err = capfd.readouterr().err
    assert E.default_context().merge_path() == "append64"
    lines, tts = append_lines(err), tt_lines(err)
    with capfd.disabled():
        print(f"\n    k={k} S={len(samples)} append_lds_ranks={lds_ranks} append_coarse={coarse}: {lines} {tts}", flush=True)
    want = check_parity(E, samples, k, True, ga, monkeypatch)             # the oracle, the sorted path, kept rows and all rows of fresh merges
    assert same_rows(base[0], want) and base[1] == list(ga.sample_kmers())
    assert base[2] == columns(engine_merge(E, samples, k, True, names).align(filter_type=E.FILTER_NO_CONST, min_freq=0.9))
    del_knob(monkeypatch, "append_lds_ranks")
    if coarse:
        del_knob(monkeypatch, "append_coarse")
    assert len(tts) == len(lines) and len(append_lines(err0)) == 1
    return append_lines(err0)[0], lines, tts


def test_tier2_holds_singletons_of_related_samples(E, capfd, monkeypatch):
    """40 related samples: the first sixteen fill the LDS tier, the first meeting closes it, the private SNPs of the other 24 are tier 2's.  Two
    readers a region without the XCD map (logB = 1)."""
    rng = np.random.default_rng(101)
    base, lines, tts = run_case(E, capfd, monkeypatch, related(rng, 9600, 40, 3), 21, 512)
    assert [(x[0], x[1], x[5]) for x in lines] == [(2, 2, "ok")] and lines[0][:4] == base[:4]
    t = tts[0]
    assert (t["split"], t["close_at"], t["meet_every"]) == ("same", 512, 1)
    assert t["closed_blocks"] == t["blocks"] == 4 and t["last_close_meeting"] == 1 and t["tier2_rows"] > 0 and t["lds_rows"] >= 4 * 512


def test_tier2_rows_shared_by_the_late_clade(E, capfd, monkeypatch):
    """rows first seen after the closing that twenty later samples share: the late half's clade SNPs.  Two readers a region that meet through
    the region's counter as well (logB = 3: the XCD map)."""
    rng = np.random.default_rng(202)
    base, lines, tts = run_case(E, capfd, monkeypatch, clades(rng, L, 48, 16, 30), 21, 256)
    assert [(x[0], x[1], x[5]) for x in lines] == [(4, 2, "ok")] and lines[0][:4] == base[:4]
    t = tts[0]
    assert t["closed_blocks"] == t["blocks"] == 16 and t["last_close_meeting"] == 1 and t["tier2_rows"] > 30 * 20


@pytest.mark.parametrize("lds_ranks", [1, 256])
def test_repeats_palindromes_and_the_zero_key_in_tier2(E, lds_ranks, capfd, monkeypatch):
    """after 32 related samples: a repeated split k-mer (its base sets fold), self-palindromic windows, the all-zero key (an entry that is
    nothing but its rank) -- all of them rows of tier 2, whether the LDS tier closed at the first meeting or never opened"""
    rng = np.random.default_rng(303)
    samples = related(rng, 20_000, 32, 5) + odd_samples(rng, 21) + odd_samples(rng, 21)[:2]
    base, lines, tts = run_case(E, capfd, monkeypatch, samples, 21, lds_ranks)
    assert [(x[0], x[1], x[5]) for x in lines] == [(3, 1, "ok")] and lines[0][:4] == base[:4]
    t = tts[0]
    assert t["closed_blocks"] == t["blocks"] == 8 and t["tier2_rows"] > 0
    assert (t["lds_rows"] == 0) == (lds_ranks == 1)


def test_list_flushes_inside_a_sample(E, capfd, monkeypatch):
    """blocks of ~8 100 rows (one step coarser than the split that fits the LDS ranks): a related family fills and closes the LDS tier, then six
    unrelated samples bring ~1 150 rows each to tier 2, at once, with ranks far beyond the row buffer's 5 760 -- more cells a sample than a
    wave's list holds"""
    rng = np.random.default_rng(404)
    base, lines, tts = run_case(E, capfd, monkeypatch, related(rng, L, 32, 2) + unrel(rng, L, 6), 21, 512, coarse=1)
    assert base[0] == 6 and [(x[0], x[1], x[5]) for x in lines] == [(5, 4, "ok")]
    assert 5760 < lines[0][2] <= 12032 and lines[0][3] == 8192
    t = tts[0]
    assert t["lds_ranks"] == 5760 and t["closed_blocks"] == t["blocks"] == 32 and t["list_flushes"] > 32 and t["tier2_rows"] > 32 * 6000


def test_tier2_overflow_takes_the_finer_split(E, capfd, monkeypatch):
    """~9 250 rows a block and the LDS tier closed from the start: more than tier 2 emits (8 256) -- the blocks fail, the pass comes back one
    split finer and the result is the same"""
    rng = np.random.default_rng(505)
    base, lines, tts = run_case(E, capfd, monkeypatch, unrel(rng, L, 8), 21, 1, coarse=1)
    assert base[0] == 6 and [(x[0], x[5]) for x in lines] == [(5, "overflow"), (6, "ok")]
    assert tts[1]["closed_blocks"] == tts[1]["blocks"] == 64 and tts[1]["lds_rows"] == 0


@pytest.mark.parametrize("S", [1, 5, 17])
def test_sample_counts_around_the_waves(E, S, capfd, monkeypatch):
    """one sample, five (eleven waves without a sample), seventeen (a wave with two, no meeting): every row in tier 2"""
    rng = np.random.default_rng(600 + S)
    base, lines, tts = run_case(E, capfd, monkeypatch, related(rng, 20_000, S, 5), 21, 1)
    assert [(x[0], x[1], x[5]) for x in lines] == [(3, 1, "ok")] and lines[0][:4] == base[:4]
    assert tts[0]["closed_blocks"] == 8 and tts[0]["lds_rows"] == 0 and tts[0]["tier2_rows"] >= 19_000


@pytest.mark.parametrize("length,logQ,rem", [(60_000, 4, 32), (120_000, 5, 31)])
def test_both_kernel_forms_at_the_seam(E, length, logQ, rem, capfd, monkeypatch):
    """k = 19: rem = 32 is the last split of the HI form, rem = 31 the first of the other"""
    rng = np.random.default_rng(700 + rem)
    base, lines, tts = run_case(E, capfd, monkeypatch, related(rng, length, 5, 20), 19, 1)
    assert [(x[0], x[1], x[5]) for x in lines] == [(logQ, 1, "ok")] and 2 * (19 - 1) - lines[0][0] == rem
    assert tts[0]["closed_blocks"] == tts[0]["blocks"] == 1 << logQ and tts[0]["tier2_rows"] > length


def test_two_readers_a_region_every_row_in_tier2(E, capfd, monkeypatch):
    """A = 2 with the XCD map and the start counters, two unrelated samples"""
    rng = np.random.default_rng(808)
    base, lines, tts = run_case(E, capfd, monkeypatch, unrel(rng, L, 2), 21, 1)
    assert [(x[0], x[1], x[5]) for x in lines] == [(4, 2, "ok")]
    assert tts[0]["closed_blocks"] == 16 and tts[0]["tier2_rows"] > 2 * L - 100
