"""`ska lo` on the device: the coloured de Bruijn graph of skx_array_lo_graph against tests/lo_model.py, and the CLI's four outputs against
the reference's goldens and the model."""
import os

import numpy as np
import pytest

import lo_checks as LC
import lo_model as M
import ora
import skx_engine as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN = os.path.join(ROOT, "tests", "golden", "input")
OK = os.path.join(ROOT, "tests", "golden", "correct")


def _read(p):
    with open(p) as f:
        return f.read()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["test_skalo.skf", "test_skalo_indel.skf", "merge.skf", "merge_k41.skf"])
def test_device_graph_equals_model_on_fixtures(name):
    arr = E.Array.load(os.path.join(IN, name))
    g = LC.check_graph(arr)
    assert g.wpn == (1 if arr.k <= 31 else 2)


@pytest.mark.timeout(300)
def test_device_graph_single_strand_multi_edges():
    inputs = [(n, os.path.join(IN, f"{n}.fa"), None) for n in ("test_1", "test_2")]
    arr = E.Array.build(inputs, k=17, rc=False)
    LC.check_graph(arr)


@pytest.mark.timeout(300)
def test_device_graph_iupac_expansion():
    inputs = [(n, os.path.join(IN, f"{n}.fa"), None) for n in ("ambig_test_1", "ambig_test_2")]
    arr = E.Array.build(inputs, k=9)
    _, var, _ = arr.export()
    assert set(var.ravel().tobytes()) - set(b"ACGT-"), "fixture should hold ambiguity codes"
    LC.check_graph(arr)


@pytest.mark.timeout(300)
def test_device_graph_130_samples():
    rng = np.random.default_rng(7)
    k, rows, S = 15, 400, 130
    keys = np.zeros(rows, E.KEY_DT)
    keys["lo"] = np.sort(rng.choice(1 << (2 * (k - 1)), rows, replace=False)).astype(np.uint64)
    var = rng.choice(np.frombuffer(b"ACGT-NRY", np.uint8), size=(rows, S), p=[.22, .22, .22, .22, .06, .02, .02, .02])
    arr = E.Array.from_host(k, True, [f"s{i}" for i in range(S)], keys, var)
    g = LC.check_graph(arr)
    assert g.info["colour_words"] == 3


@pytest.mark.timeout(300)
def test_lo_cli_snp_golden(tmp_path):
    r = LC.ska("lo", "-r", os.path.join(IN, "test_skalo_reference.fas"), os.path.join(IN, "test_skalo.skf"), "out", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert _read(tmp_path / "out_snps.fas") == _read(os.path.join(OK, "test_skalo_snps.fas"))
    want, _ = M.run_skf(os.path.join(IN, "test_skalo.skf"), reference=os.path.join(IN, "test_skalo_reference.fas"))
    for suffix in ("_pseudo_genomes.fas", "_snps.vcf", "_indels.vcf"):
        assert _read(tmp_path / f"out{suffix}") == want[suffix], suffix


@pytest.mark.timeout(300)
def test_lo_cli_indel_golden(tmp_path):
    r = LC.ska("lo", os.path.join(IN, "test_skalo_indel.skf"), "out", "-v", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert _read(tmp_path / "out_indels.vcf") == _read(os.path.join(OK, "test_skalo_indels.vcf"))
    assert not (tmp_path / "out_snps.vcf").exists()
    for line in ("50 nodes", "2 entry nodes", "2 variant groups", "1 indels", "0 SNPs"):
        assert line in r.stderr, line


@pytest.mark.timeout(300)
def test_lo_no_entry_node(tmp_path):
    arr = ora.Array.build([("only", os.path.join(IN, "test_1.fa"), None)], k=17)
    arr.save(str(tmp_path / "one.skf"))
    r = LC.ska("lo", str(tmp_path / "one.skf"), "out", cwd=tmp_path)
    assert r.returncode == 1, r.stderr
    assert "ERROR [ska::skalo::extremities] Error: there is no entry node in this graph, hence no variant." in r.stderr


@pytest.mark.timeout(900)
@pytest.mark.parametrize("k", [31, 41])
def test_lo_synthetic_outbreak(tmp_path, k):
    names, events = LC.outbreak(tmp_path)
    files = [str(tmp_path / f"{n}.fa") for n in names]
    r = LC.ska("build", "-k", str(k), "-o", str(tmp_path / "out"), *files, "--threads", "4", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    skf = str(tmp_path / "out.skf")
    ref = str(tmp_path / "ref.fa")
    want, counts = M.run_skf(skf, reference=ref)
    got = {}
    for threads in ("1", "8"):
        pre = str(tmp_path / f"lo{threads}")
        r = LC.ska("lo", skf, pre, "-r", ref, "--threads", threads, cwd=tmp_path)
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
