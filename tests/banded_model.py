"""The single-linkage clusters of `ska distance --clusters` in plain Python, over the float64 values of the full table: what the device union
(skx_array_distance_banded) is compared against.  A pair is an edge when its values AS THE TABLE PRINTS THEM ("%.2f", "%.5f", parsed back)
satisfy distance <= cluster_snps and mismatch_prop <= cluster_mismatches; a cluster's label is its lowest sample.  Nothing here is shared
with the engine."""


def printed(value, decimals):
    return float("%.*f" % (decimals, value))


def clusters(D, M, cluster_snps=10.0, cluster_mismatches=1.0):
    """D, M: S x S (only i < j is read) -> (labels: labels[i] = the lowest sample of i's cluster, number of edges, number of clusters)"""
    S = len(D)
    up = list(range(S))

    def find(x):
        while up[x] != x:
            x = up[x]
        return x

    edges = 0
    for i in range(S):
        for j in range(i + 1, S):
            if printed(D[i][j], 2) <= cluster_snps and printed(M[i][j], 5) <= cluster_mismatches:
                edges += 1
                a, b = find(i), find(j)
                if a != b:
                    up[max(a, b)] = min(a, b)
    labels = [find(i) for i in range(S)]
    return labels, edges, sum(1 for i in range(S) if labels[i] == i)


def clusters_csv(names, labels):
    """clusters.csv of the labels: clusters numbered from 1 by size descending (ties: lowest sample), rows by cluster, then by sample; RFC 4180 quoting"""
    S = len(names)
    members = {}
    for i in range(S):
        members.setdefault(labels[i], []).append(i)
    order = sorted(members, key=lambda r: (-len(members[r]), r))
    out = ["id,Cluster__autocolour\n"]
    for k, r in enumerate(order):
        for i in members[r]:
            n = names[i]
            if any(c in n for c in ',"\n\r'):
                n = '"' + n.replace('"', '""') + '"'
            out.append(f"{n},{k + 1}\n")
    return "".join(out)
