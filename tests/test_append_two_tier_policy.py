"""two_tier_plan (csrc/skx_merge.cpp) through skx_debug_two_tier_plan, a test hook of the library: host arithmetic only, no device.
The plan takes the append pass one split coarser (two readers a region, late rows in the second tier) only for many related samples whose
blocks fill the LDS ranks; the numbers below are the ones DESIGN section 5 quotes."""
import ctypes
import math

import numpy as np
import pytest

import skx_engine as E

LDS_RANKS, MAX_CAP = 5760, 6016


@pytest.fixture(scope="module")
def plan():
    lib = E.load_library()
    lib.skx_debug_two_tier_plan.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.skx_debug_two_tier_plan.restype = ctypes.c_int

    def f(u_est, relvar, raw_max, S, logQ_fine, min_logQ):
        out = np.zeros(3, dtype=np.uint32)
        assert lib.skx_debug_two_tier_plan(u_est, relvar, raw_max, S, logQ_fine, min_logQ, out.ctypes.data) == 0
        return bool(out[0]), int(out[1]), int(out[2])
    return f


def need(mean):
    return mean + 6.0 * math.sqrt(mean + 1.0) + 32.0


def test_the_flagship_takes_the_coarser_split(plan):
    """1 000 x 5 Mbp: 22.6 M rows, 5 M windows a sample, the finer split 2^12.  The waves meet every 15 samples each; the tier closes at its
    ranks less what 240 samples may bring (six sigma, + 32)"""
    u, raw, S = 22_608_164.0, 4_999_970, 1000
    on, close, resync = plan(u, 0.0, raw, S, 12, 10)
    assert on and resync == 15
    between = 16 * resync * (u - raw) / 2048 / (S - 1)
    assert close == int(LDS_RANKS - need(between)) and 3300 < close < 3500


def test_what_keeps_the_split(plan):
    u, raw = 22_608_164.0, 4_999_970
    assert plan(u, 0.0, raw, 1000, 12, 10)[0]
    assert not plan(u, 0.0, raw, 1000, 10, 10)[0]                        # no coarser split: logQ >= logB
    assert not plan(13_921_094.0, 0.0, raw, 500, 12, 10)[0]              # (d) 500 genomes: the finer split's blocks are 0.56 full (measured: the coarser split loses)
    assert not plan(9_470_987.0, 0.0, raw, 250, 11, 10)[0]               # (b) 250 genomes: 4 883 windows a block are more than half the LDS tier
    assert not plan(32 * 37_000.0, 0.0, 37_000, 32, 8, 3)[0]             # (b) unrelated samples: every sample brings a sample's rows
    assert not plan(39 * 4_879.0, 0.0, 4_879, 39, 6, 0)[0]
    assert not plan(u, 0.0, raw, 20, 12, 10)[0]                          # no meeting at which every wave has a sample
    assert not plan(2.2 * u, 0.0, raw, 1000, 12, 10)[0]                  # (a) more rows than a block's ranks
    assert not plan(u, 0.0, raw, 1, 12, 10)[0]


def test_the_tier_closes_before_it_can_fill(plan):
    """whatever is taken: what a block has by the first meeting fits the tier, and lds_close leaves room for the rows of one more interval"""
    rng = np.random.default_rng(7)
    taken = 0
    for _ in range(2000):
        S = int(rng.integers(2, 3000))
        raw = int(rng.integers(10_000, 8_000_000))
        u = raw * (1.0 + rng.random() * 0.02 * S)
        fine = int(rng.integers(1, 16))
        on, close, resync = plan(u, 0.0, raw, S, fine, 0)
        assert 1 <= resync <= 16
        if not on:
            continue
        taken += 1
        nsub = 2.0 ** (fine - 1)
        first, per = raw / nsub, (u - raw) / nsub / (S - 1)
        assert resync <= (S - 16) // 16 and first <= 0.5 * LDS_RANKS and per <= 0.02 * first
        assert need(first + 16 * resync * per) <= LDS_RANKS and need(u / nsub) <= 12032 and u / (2 * nsub) >= 0.8 * MAX_CAP
        assert 1 <= close <= LDS_RANKS and close + need(16 * resync * per) <= LDS_RANKS + 1
    assert taken > 5
