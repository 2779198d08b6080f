"""Checks shared by the `ska lo` GPU tests: the device graph of skx_array_lo_graph against tests/lo_model.py, the properties any correct
graph of the same rows has whatever the model says, and the synthetic outbreaks the CLI is run on."""
import collections
import os
import random
import subprocess

import lo_model as M
import skx_engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")


def ska(*args, cwd=None, timeout=300):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=timeout, cwd=cwd)


def rows_of(arr):
    """(split k-mers as Python ints, rows of middle bases as bytes) of a device or oracle Array, in its row order"""
    keys, var, _ = arr.export()
    return [int(lo) | (int(hi) << 64) for lo, hi in zip(keys["lo"], keys["hi"])], [bytes(r) for r in var]


def check_graph(arr, rows=None):
    """device graph of `arr` == the model's graph of `rows` (default: the array's own rows), and check_properties"""
    keys, var = rows if rows is not None else rows_of(arr)
    nodes, edges, entries, exits, colours = M.graph_of(keys, var, arr.k)
    g = E.default_context().lo_graph(arr)
    adj = g.adjacency()
    assert sorted(adj) == nodes
    assert adj == edges
    assert E._to_ints(g.entries, g.wpn) == entries
    assert E._to_ints(g.exits, g.wpn) == exits
    ks = sorted(colours)
    absent = [(max(ks) + 1) if ks else 1]
    got, found = g.gather(ks + absent)
    assert found == [True] * len(ks) + [False]
    assert got[:len(ks)] == [colours[x] for x in ks]
    assert g.info["n_nodes"] == len(nodes) and g.info["n_entries"] == len(entries)
    check_properties(g, keys, var, arr.k)
    return g


def full_kmers(keys, var, k):
    """(every full k-mer K and rc(K) of the rows, number of (row, base) pairs some sample has), straight from the rows"""
    half = (k - 1) // 2
    kmers, pairs = set(), 0
    for key, row in zip(keys, var):
        bases = 0
        for cell in set(row):
            for c in M.IUPAC.get(chr(cell), ""):
                bases |= 1 << M.enc_base(c)
        for b in range(4):
            if (bases >> b) & 1:
                K = ((key >> (2 * half)) << (2 * (half + 1))) | (b << (2 * half)) | (key & ((1 << (2 * half)) - 1))
                kmers |= {K, M.rc(K, k)}
                pairs += 1
    return kmers, pairs


def check_properties(g, keys, var, k):
    """what holds of any correct graph of these rows, without the model: ascending nodes, CSR offsets, every edge's reverse-complement
    twin, exits = rc(entries), strand-independent colours, and the table's and colours' sizes"""
    kg = k - 1
    nodes, nb = E._to_ints(g.nodes, g.wpn), E._to_ints(g.neighbours, g.wpn)
    off = [int(x) for x in g.offsets]
    assert all(a < b for a, b in zip(nodes, nodes[1:])), "nodes not strictly ascending"
    assert off[0] == 0 and off[-1] == len(nb) == g.info["n_edges"] and len(off) == len(nodes) + 1
    assert all(a <= b for a, b in zip(off, off[1:])), "offsets decrease"
    edges = collections.Counter((nodes[i], nb[e]) for i in range(len(nodes)) for e in range(off[i], off[i + 1]))
    for (u, v), n in edges.items():
        assert edges[(M.rc(v, kg), M.rc(u, kg))] == n, ("edge without its twin", u, v)
    entries, exits = E._to_ints(g.entries, g.wpn), E._to_ints(g.exits, g.wpn)
    assert exits == sorted(M.rc(x, kg) for x in entries)
    kmers, pairs = full_kmers(keys, var, k)
    assert g.info["n_colours"] == pairs
    assert g.info["n_kmers"] == len(kmers)
    ks = sorted(kmers)
    got, found = g.gather(ks)
    assert all(found)
    col = dict(zip(ks, got))
    assert all(col[K] == col[M.rc(K, k)] for K in ks), "a k-mer and its reverse complement differ in colour"


def outbreak(tmp_path, seed=11, n=32, length=50_000, n_sites=120, drop_every=0, drop_len=1500):
    """ancestor + samples with planted SNPs and 1-10 bp indels, each carried by a random subset of samples; with drop_every, every
    drop_every-th sample (from sample 0) also loses a stretch of drop_len bases at a random place"""
    rnd = random.Random(seed)
    anc = [rnd.choice("ACGT") for _ in range(length)]
    sites = sorted(rnd.sample(range(200, length - 200, 150), n_sites))
    events = []
    for i, p in enumerate(sites):
        carriers = set(rnd.sample(range(n), rnd.randint(2, n // 2)))
        if i % 6 == 5:
            events.append(("indel", p, rnd.randint(1, 10), carriers))
        else:
            events.append(("snp", p, rnd.choice([b for b in "ACGT" if b != anc[p]]), carriers))
    names = []
    for s in range(n):
        seq = list(anc)
        for kind, p, x, carriers in reversed(events):
            if s not in carriers:
                continue
            if kind == "snp":
                seq[p] = x
            else:
                del seq[p:p + x]
        if drop_every and s % drop_every == 0:
            at = rnd.randrange(100, len(seq) - drop_len - 100)
            del seq[at:at + drop_len]
        names.append(f"s{s}")
        with open(tmp_path / f"s{s}.fa", "w") as f:
            f.write(f">s{s}\n{''.join(seq)}\n")
    with open(tmp_path / "ref.fa", "w") as f:
        f.write(">ref\n" + "".join(anc) + "\n")
    return names, events
