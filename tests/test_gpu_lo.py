"""`ska lo` on the device: the coloured de Bruijn graph of skx_array_lo_graph against tests/lo_model.py, and the CLI's four outputs against
the reference's goldens and the model."""
import os
import random
import subprocess

import numpy as np
import pytest

import lo_model as M
import ora
import skx_engine as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
IN = os.path.join(ROOT, "tests", "golden", "input")
OK = os.path.join(ROOT, "tests", "golden", "correct")


def _ska(*args, cwd=None, timeout=300):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=timeout, cwd=cwd)


def _read(p):
    with open(p) as f:
        return f.read()


def _check_graph(arr):
    """device graph of `arr` == the model's graph of the same array's rows"""
    keys, var, _ = arr.export()
    ints = [int(lo) | (int(hi) << 64) for lo, hi in zip(keys["lo"], keys["hi"])]
    nodes, edges, entries, exits, colours = M.graph_of(ints, [bytes(r) for r in var], arr.k)
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
    return g


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["test_skalo.skf", "test_skalo_indel.skf", "merge.skf", "merge_k41.skf"])
def test_device_graph_equals_model_on_fixtures(name):
    arr = E.Array.load(os.path.join(IN, name))
    g = _check_graph(arr)
    assert g.wpn == (1 if arr.k <= 31 else 2)


@pytest.mark.timeout(300)
def test_device_graph_single_strand_multi_edges():
    inputs = [(n, os.path.join(IN, f"{n}.fa"), None) for n in ("test_1", "test_2")]
    arr = E.Array.build(inputs, k=17, rc=False)
    _check_graph(arr)


@pytest.mark.timeout(300)
def test_device_graph_iupac_expansion():
    inputs = [(n, os.path.join(IN, f"{n}.fa"), None) for n in ("ambig_test_1", "ambig_test_2")]
    arr = E.Array.build(inputs, k=9)
    _, var, _ = arr.export()
    assert set(var.ravel().tobytes()) - set(b"ACGT-"), "fixture should hold ambiguity codes"
    _check_graph(arr)


@pytest.mark.timeout(300)
def test_device_graph_130_samples():
    rng = np.random.default_rng(7)
    k, rows, S = 15, 400, 130
    keys = np.zeros(rows, E.KEY_DT)
    keys["lo"] = np.sort(rng.choice(1 << (2 * (k - 1)), rows, replace=False)).astype(np.uint64)
    var = rng.choice(np.frombuffer(b"ACGT-NRY", np.uint8), size=(rows, S), p=[.22, .22, .22, .22, .06, .02, .02, .02])
    arr = E.Array.from_host(k, True, [f"s{i}" for i in range(S)], keys, var)
    g = _check_graph(arr)
    assert g.info["colour_words"] == 3


@pytest.mark.timeout(300)
def test_lo_cli_snp_golden(tmp_path):
    r = _ska("lo", "-r", os.path.join(IN, "test_skalo_reference.fas"), os.path.join(IN, "test_skalo.skf"), "out", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert _read(tmp_path / "out_snps.fas") == _read(os.path.join(OK, "test_skalo_snps.fas"))
    want, _ = M.run_skf(os.path.join(IN, "test_skalo.skf"), reference=os.path.join(IN, "test_skalo_reference.fas"))
    for suffix in ("_pseudo_genomes.fas", "_snps.vcf", "_indels.vcf"):
        assert _read(tmp_path / f"out{suffix}") == want[suffix], suffix


@pytest.mark.timeout(300)
def test_lo_cli_indel_golden(tmp_path):
    r = _ska("lo", os.path.join(IN, "test_skalo_indel.skf"), "out", "-v", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert _read(tmp_path / "out_indels.vcf") == _read(os.path.join(OK, "test_skalo_indels.vcf"))
    assert not (tmp_path / "out_snps.vcf").exists()
    for line in ("50 nodes", "2 entry nodes", "2 variant groups", "1 indels", "0 SNPs"):
        assert line in r.stderr, line


@pytest.mark.timeout(300)
def test_lo_no_entry_node(tmp_path):
    arr = ora.Array.build([("only", os.path.join(IN, "test_1.fa"), None)], k=17)
    arr.save(str(tmp_path / "one.skf"))
    r = _ska("lo", str(tmp_path / "one.skf"), "out", cwd=tmp_path)
    assert r.returncode == 1, r.stderr
    assert "ERROR [ska::skalo::extremities] Error: there is no entry node in this graph, hence no variant." in r.stderr


def _outbreak(tmp_path, seed=11, n=32, length=50_000):
    """ancestor + samples with planted SNPs and 1-10 bp indels, each carried by a random subset of samples"""
    rnd = random.Random(seed)
    anc = [rnd.choice("ACGT") for _ in range(length)]
    sites = sorted(rnd.sample(range(200, length - 200, 150), 120))
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
        names.append(f"s{s}")
        with open(tmp_path / f"s{s}.fa", "w") as f:
            f.write(f">s{s}\n{''.join(seq)}\n")
    with open(tmp_path / "ref.fa", "w") as f:
        f.write(">ref\n" + "".join(anc) + "\n")
    return names, events


@pytest.mark.timeout(900)
@pytest.mark.parametrize("k", [31, 41])
def test_lo_synthetic_outbreak(tmp_path, k):
    names, events = _outbreak(tmp_path)
    files = [str(tmp_path / f"{n}.fa") for n in names]
    r = _ska("build", "-k", str(k), "-o", str(tmp_path / "out"), *files, "--threads", "4", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    skf = str(tmp_path / "out.skf")
    ref = str(tmp_path / "ref.fa")
    want, counts = M.run_skf(skf, reference=ref)
    got = {}
    for threads in ("1", "8"):
        pre = str(tmp_path / f"lo{threads}")
        r = _ska("lo", skf, pre, "-r", ref, "--threads", threads, cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        got[threads] = {s: _read(pre + s) for s in ("_snps.fas", "_pseudo_genomes.fas", "_snps.vcf", "_indels.vcf")}
    assert got["1"] == got["8"]
    for s, text in got["1"].items():
        assert text == want[s], s
    vcf = [l.split("\t") for l in got["1"]["_snps.vcf"].splitlines() if not l.startswith("#")]
    called = {int(f[1]) for f in vcf}
    positions = [p for _, p, _, _ in events]
    for kind, p, alt, _ in events:
        if kind == "snp" and all(q == p or abs(q - p) > k for q in positions):
            assert p + 1 in called, (k, p)
    indel_lines = [l for l in got["1"]["_indels.vcf"].splitlines() if not l.startswith("#")]
    assert len(indel_lines) >= sum(1 for e in events if e[0] == "indel") // 2
