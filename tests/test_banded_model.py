"""tests/banded_model.py against skh_distance_clusters (host only, no device): the model's labels, through its own CSV writer and through
skh_clusters_csv, give the bytes of skh_distance_clusters' CSV on random tables that include exact duplicates and values on the thresholds."""
import numpy as np
import pytest

import skx_engine as E
from banded_model import clusters, clusters_csv, printed


def _table(S, seed, fractional):
    """a random pair table: groups of samples at distance 0 (duplicates), close pairs, far pairs; distances in 1/36 steps when fractional"""
    rng = np.random.default_rng(seed)
    group = rng.integers(0, max(S // 3, 1), S)
    D, M = np.zeros((S, S)), np.zeros((S, S))
    for i in range(S):
        for j in range(i + 1, S):
            if group[i] == group[j]:
                key = 0 if rng.random() < 0.5 else int(rng.integers(0, 40))
            else:
                key = int(rng.integers(0, 3000)) if rng.random() < 0.1 else int(rng.integers(300, 3000))
            D[i][j] = key / 36.0 if fractional else float(key)
            n = int(rng.integers(1, 400))
            M[i][j] = int(rng.integers(0, n + 1)) / n
    t = np.zeros(S * (S - 1) // 2, E.DIST_DT)
    iu = np.triu_indices(S, 1)
    t["distance"], t["mismatch_prop"] = D[iu], M[iu]
    return t, D.tolist(), M.tolist()


@pytest.mark.parametrize("fractional", [False, True], ids=["integer", "over-36"])
@pytest.mark.parametrize("S", [1, 2, 7, 40])
def test_model_against_the_host_clusters(S, fractional):
    names = [f"s{i}" if i % 5 else f'na,me "{i}"' for i in range(S)]
    t, D, M = _table(S, 100 * S + fractional, fractional)
    own = sorted(set(t["distance"].tolist()))[: 6] if S > 1 else []
    snps = [0.0, 10.0, 1e9] + [printed(v, 2) for v in own] + [printed(v, 2) + 0.005 for v in own] + [max(printed(v, 2) - 0.005, 0.0) for v in own]
    mism = [0.0, 0.25, 1.0] + ([printed(float(t["mismatch_prop"][0]), 5)] if S > 1 else [])
    seen = set()
    for cs in snps:
        for cm in mism:
            labels, edges, n_clusters = clusters(D, M, cs, cm)
            csv, dot = E.distance_clusters(names, t, cs, cm)
            assert clusters_csv(names, labels) == csv, (cs, cm)
            assert E.clusters_csv(names, labels) == csv, (cs, cm)
            assert dot.count(" -- ") == edges
            assert n_clusters == len(set(labels)) == len({ln.rsplit(",", 1)[1] for ln in csv.splitlines()[1:]})
            seen.add(n_clusters)
    if S >= 7:
        assert len(seen) > 2 and 1 in seen and S in seen                       # the thresholds bite: from all alone to one cluster


def test_clusters_csv_refuses_labels_that_are_not_roots():
    names = ["a", "b", "c"]
    for bad in ([0, 2, 2], [0, 0, 1], [1, 1, 2]):
        with pytest.raises(E.EngineError) as e:
            E.clusters_csv(names, bad)
        assert e.value.code == E.EINVAL
