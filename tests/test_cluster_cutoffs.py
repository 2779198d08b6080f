"""skh_cluster_cutoffs (host only, through ctypes): the printed-value rules of skh_distance_clusters as the two numbers a device compares.
kmax: '%.2f' of a key's distance, parsed back, is <= T exactly when key <= kmax.  pmax: '%.5f' of a proportion, parsed back, is <= T exactly
when p <= pmax as float64.  The proportions include m / 200000, the exact decimal ties of the fifth place."""
import numpy as np
import pytest

import skx_engine as E

SNPS = (0, 0.004, 0.005, 0.01, 10, 10.004, 10.005, 1e300)
MISM = (0, 0.000005, 0.00001, 0.5, 0.123455, 1.0)


def _key_distance(key, filt_ambig):
    return float(key) if filt_ambig else float(key) / 36.0


@pytest.mark.parametrize("filt_ambig", [1, 0], ids=["filter-ambiguous", "allow-ambiguous"])
@pytest.mark.parametrize("T", SNPS)
def test_kmax_is_the_printed_distance_rule(T, filt_ambig):
    kmax, _ = E.cluster_cutoffs(T, 1.0, filt_ambig)
    for key in range(4001):
        assert (float("%.2f" % _key_distance(key, filt_ambig)) <= T) == (key <= kmax), (T, filt_ambig, key, kmax)
    if T == 1e300:
        # nothing exceeds it: saturated at the bound no key reaches, inside 64 bits
        assert kmax == 1 << 62
    else:
        assert kmax < 4000                                                      # the range above holds the boundary


@pytest.mark.parametrize("T", MISM)
def test_pmax_is_the_printed_proportion_rule(T):
    _, pmax = E.cluster_cutoffs(10.0, T, 1)
    assert 0.0 <= pmax <= 1.0
    ps = {m / n for n in range(1, 401) for m in range(n + 1)} | {m / 200000 for m in range(401)}
    ps |= {float(np.nextafter(p, 2.0)) for p in list(ps) if p < 1.0} | {float(np.nextafter(p, -1.0)) for p in list(ps) if p > 0.0}
    for p in ps:
        assert (float("%.5f" % p) <= T) == (p <= pmax), (T, p, pmax)
    # the largest: the next double up fails (or there is none in [0, 1])
    assert pmax == 1.0 or float("%.5f" % float(np.nextafter(pmax, 2.0))) > T


def test_the_two_rules_do_not_depend_on_each_other():
    assert {E.cluster_cutoffs(10.0, t, 1)[0] for t in MISM} == {10}
    assert {E.cluster_cutoffs(t, 0.5, 0)[1] for t in SNPS} == {E.cluster_cutoffs(0.0, 0.5, 1)[1]}


@pytest.mark.parametrize("snps, mism", [(float("nan"), 1.0), (1.0, float("nan")), (-1.0, 1.0), (1.0, -0.5)])
def test_refusals(snps, mism):
    with pytest.raises(E.EngineError) as e:
        E.cluster_cutoffs(snps, mism, 1)
    assert e.value.code == E.EINVAL
