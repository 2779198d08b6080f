"""`ska lo` at its edges.  The device graph (csrc/skx_lo.hip) at k = 5 to 63, one to three colour words, row counts around the colour
kernel's 64-row wave and 256-row block and the sort and scan tiles, every middle-base code, the wide path of an array built on the device,
and its refusals -- each against tests/lo_model.py and against properties any correct graph has.  The calling half (host/ska_lo.cpp) with
two and three colour words and every option away from its default, on synthetic outbreaks, against the model's four outputs."""
import os
import subprocess

import numpy as np
import pytest

import lo_checks as LC
import lo_model as M
import ora
import skx_engine as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN = os.path.join(ROOT, "tests", "golden", "input")
U64 = (1 << 64) - 1
# ACGT, every ambiguity code, and '-' (no colour)
BASES = np.frombuffer(b"ACGTMRWSYKVHDBN-", np.uint8)
P_BASES = [0.2] * 4 + [0.1 / 11] * 11 + [0.1]


def _keys(rng, k, R):
    """R distinct split k-mers, ascending.  At k >= 31 one has both arms all G (every bit of the key set); at small k a drawn key brings
    the row of its reverse complement, so full k-mers of different rows and colours collide and the first-writer rule decides"""
    kg = k - 1
    space = 1 << (2 * kg)
    keys = {space - 1} if k >= 31 else set()
    while len(keys) < R:
        x = int.from_bytes(rng.bytes(16), "little") % space
        keys.add(x)
        if k <= 7 and len(keys) < R:
            keys.add(M.rc(x, kg))
    return sorted(keys)


def _variants(rng, R, S):
    var = rng.choice(BASES, size=(R, S), p=P_BASES)
    for r in range(0, R, 7):                 # one sample's N next to A: all four bases present
        var[r, :] = ord("A")
        var[r, (r * 13) % S] = ord("N")
    for r in range(3, R, 11):                # no sample has this row: it adds no colour
        var[r, :] = ord("-")
    return var


def _array(k, keys, var):
    kd = np.zeros(len(keys), E.KEY_DT)
    kd["lo"] = [x & U64 for x in keys]
    kd["hi"] = [x >> 64 for x in keys]
    return E.Array.from_host(k, True, [f"s{i}" for i in range(var.shape[1])], kd, var)


def _check_absent(g, k, present):
    """k-mers outside the table -- below its first, above its last, and one differing from a present k-mer only in its top base --
    come back not found with no colour"""
    assert g.gather([]) == ([], [])
    ks = sorted(present)
    q = ([ks[0] - 1] if ks[0] > 0 else []) + [ks[-1] + 1]
    top = 2 * (k - 1)
    for K in ks:
        flips = [K ^ (x << top) for x in (1, 2, 3) if K ^ (x << top) not in present]
        if flips:
            q.append(flips[0])
            break
    assert len(q) >= 2
    got, found = g.gather(q)
    assert found == [False] * len(q)
    assert got == [0] * len(q)


# (k, samples, rows): every k, every sample count (W = 1, 1, 1, 2, 2, 3) and every row count appear; k = 63 meets S = 129
CASES = [
    (5, 1, 200), (5, 65, 200), (5, 129, 256), (5, 64, 63), (7, 63, 255), (7, 64, 257), (7, 128, 1), (7, 1, 64), (7, 129, 65),
    (31, 1, 1), (31, 63, 63), (31, 64, 65), (31, 65, 256), (31, 128, 257), (31, 129, 3000),
    (33, 1, 257), (33, 64, 1), (33, 65, 64), (33, 128, 255), (33, 63, 3000),
    (63, 129, 1), (63, 129, 257), (63, 65, 63), (63, 1, 256), (63, 64, 3000),
]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("k,S,R", CASES)
def test_device_graph_edges(k, S, R):
    rng = np.random.default_rng(10_000 * k + 100 * S + R)
    keys = _keys(rng, k, R)
    var = _variants(rng, R, S)
    arr = _array(k, keys, var)
    g = LC.check_graph(arr)
    assert g.info["colour_words"] == (S + 63) // 64
    assert g.wpn == (1 if k <= 31 else 2)
    kmers, _ = LC.full_kmers(keys, [bytes(r) for r in var], k)
    _check_absent(g, k, kmers)


def _wide_inputs(d, which):
    """(name, fasta, None) pairs: golden inputs long enough for the k, or a seeded pair whose second sample holds two copies of the
    sequence with different SNPs, so that its rows carry ambiguity codes"""
    if which != "generated":
        return [(n, os.path.join(IN, f"{n}.fa"), None) for n in which]
    rng = np.random.default_rng(17)
    anc = rng.choice(list("ACGT"), 600)
    copies = []
    for start in (40, 75):
        c = anc.copy()
        c[start::70] = ["ACGT"["ACGT".index(b) ^ 1] for b in c[start::70]]
        copies.append("".join(c))
    with open(d / "gen_1.fa", "w") as f:
        f.write(">gen_1\n" + "".join(anc) + "\n")
    with open(d / "gen_2.fa", "w") as f:
        f.write(">gen_2a\n" + copies[0] + "\n>gen_2b\n" + copies[1] + "\n")
    return [(n, str(d / f"{n}.fa"), None) for n in ("gen_1", "gen_2")]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("which,k", [(("test_1", "test_2"), 33), (("test_1", "test_2"), 41), (("test_ref", "test_ref_two_chrom"), 33),
                                     (("test_ref", "test_ref_two_chrom"), 63), ("generated", 33), ("generated", 41), ("generated", 63)])
def test_device_built_wide_array(tmp_path, which, k):
    """k > 31 built on the device: the keys are unmixed on the device (lo_unmix_wide_kernel), not taken from the host.  The graph equals
    the model's graph of the CPU oracle's array of the same inputs, and the graph of the same array saved and loaded back"""
    inputs = _wide_inputs(tmp_path, which)
    arr = E.Array.build(inputs, k=k)
    if which == "generated":
        assert set(arr.export()[1].ravel().tobytes()) - set(b"ACGT-"), "the generated pair should give ambiguity codes"
    g = LC.check_graph(arr, rows=LC.rows_of(ora.Array.build(inputs, k=k)))
    assert g.info["n_nodes"] > 0
    arr.save(str(tmp_path / "a.skf"))
    g2 = E.default_context().lo_graph(E.Array.load(str(tmp_path / "a.skf")))
    assert g2.info == g.info
    for f in ("nodes", "offsets", "neighbours", "entries", "exits"):
        assert np.array_equal(getattr(g2, f), getattr(g, f)), f
    ks = sorted(LC.full_kmers(*LC.rows_of(arr), k)[0])
    assert g2.gather(ks) == g.gather(ks)


def _refusal(arr):
    with pytest.raises(E.EngineError) as ei:
        E.default_context().lo_graph(arr)
    return ei.value


@pytest.mark.timeout(300)
def test_sample_limit():
    """sample indexes are 16-bit (read_graph.rs): 65 535 samples are taken, 65 536 refused"""
    for S in (65535, 65536):
        var = np.full((1, S), ord("C"), np.uint8)
        var[0, S - 1] = ord("G")
        arr = _array(31, [0x123456789], var)
        if S == 65535:
            g = E.default_context().lo_graph(arr)
            assert g.info["colour_words"] == 1024 and g.info["n_colours"] == 2
            kmers, _ = LC.full_kmers([0x123456789], [bytes(var[0])], 31)
            ks = sorted(kmers)
            got, found = g.gather(ks)
            assert all(found)
            same = set(got) == {(1 << (S - 1)) - 1, 1 << (S - 1)}     # (65 535-bit ints: too long for an assertion's repr)
            assert same, "colours of the C and G k-mers"
        else:
            e = _refusal(arr)
            assert e.code == E.EUNSUP and "65536 samples; sample indexes are 16-bit (at most 65535 samples)" in str(e)


@pytest.mark.timeout(300)
def test_sharded_array_refused():
    rng = np.random.default_rng(3)
    arr = _array(31, _keys(rng, 31, 20), _variants(rng, 20, 3))
    arr.set_total_samples(4)
    e = _refusal(arr)
    assert e.code == E.EUNSUP and "needs every sample of the array on one device" in str(e)


@pytest.mark.timeout(300)
def test_filtered_load_refused():
    arr, _, _ = E.Array.load_filtered(os.path.join(IN, "test_skalo.skf"))
    e = _refusal(arr)
    assert e.code == E.EINVAL and "the array's split k-mers do not match its rows" in str(e)


@pytest.mark.timeout(300)
def test_all_gaps_is_an_empty_graph(tmp_path):
    """every middle base '-': no colour, no node; gather answers not found without a table to read; the CLI has no entry node"""
    rng = np.random.default_rng(5)
    keys = _keys(rng, 31, 100)
    arr = _array(31, keys, np.full((100, 5), ord("-"), np.uint8))
    g = E.default_context().lo_graph(arr)
    for f in ("n_colours", "n_nodes", "n_edges", "n_entries", "n_kmers"):
        assert g.info[f] == 0, f
    assert list(g.offsets) == [0]
    kmers, _ = LC.full_kmers(keys, [b"ACGTN"] * len(keys), 31)
    q = sorted(kmers)[:50] + [0, (1 << 62) - 1]
    assert g.gather(q) == ([0] * len(q), [False] * len(q))
    arr.save(str(tmp_path / "gaps.skf"))
    r = LC.ska("lo", str(tmp_path / "gaps.skf"), "out", cwd=tmp_path, timeout=120)
    assert r.returncode == 1, r.stderr
    assert "ERROR [ska::skalo::extremities] Error: there is no entry node in this graph, hence no variant." in r.stderr


# ---- the calling half: `ska lo` on outbreaks of two and three colour words, each option away from its default, against the model

OUTBREAKS = {"A": dict(seed=21, n=70, length=10_000, n_sites=40, k=31),     # W = 2
             "B": dict(seed=23, n=130, length=6_000, n_sites=24, k=41)}     # W = 3
SUFFIXES = ("_snps.fas", "_pseudo_genomes.fas", "_snps.vcf", "_indels.vcf")
# (CLI arguments, model keywords); "no_ref" runs without -r
OPTIONS = {
    "defaults": ((), {}),
    "m0": (("-m", "0"), dict(missing=0.0)),
    "m0.5": (("-m", "0.5"), dict(missing=0.5)),
    "d1": (("-d", "1"), dict(depth=1)),
    "d2": (("-d", "2"), dict(depth=2)),
    "d6": (("-d", "6"), dict(depth=6)),
    "n0": (("-n", "0"), dict(indel_kmers=0)),
    "n5": (("-n", "5"), dict(indel_kmers=5)),
    "no_ref": ((), dict(reference=None)),
}
# a missing count j with f32(j / S) as -m: the model keeps a site there that the next float32 below drops (asserted below)
BOUNDARY_J = {"A": 1, "B": 1}


class Outbreak:
    """an outbreak of OUTBREAKS built once with `ska build`; every seventh sample lacks 1.5 kbp, so sites miss different numbers of
    samples.  The model's results are kept per option set."""

    def __init__(self, d, spec):
        self.dir, self.k = d, spec["k"]
        names, self.events = LC.outbreak(d, spec["seed"], spec["n"], spec["length"], spec["n_sites"], drop_every=7)
        r = LC.ska("build", "-k", str(self.k), "-o", str(d / "out"), *[str(d / f"{n}.fa") for n in names], "--threads", "4", cwd=d)
        assert r.returncode == 0, r.stderr
        self.skf, self.ref, self.S = str(d / "out.skf"), str(d / "ref.fa"), len(names)
        self.inputs = M.array_inputs(ora.Array.load(self.skf))
        self._model = {}

    def model(self, **kw):
        kw.setdefault("reference", self.ref)
        key = tuple(sorted(kw.items()))
        if key not in self._model:
            self._model[key] = M.run(*self.inputs, **kw)
        return self._model[key]

    def start(self, tag, args, ref, threads="4"):
        """`ska lo` in the background (the model runs meanwhile); finish() collects its outputs"""
        pre = str(self.dir / tag)
        cmd = [LC.SKA, "lo", self.skf, pre, "--threads", threads, *args, *(("-r", ref) if ref else ())]
        return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=self.dir), pre


def finish(started, timeout=300):
    proc, pre = started
    try:
        _, err = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        proc.kill()
        proc.communicate()
        raise
    assert proc.returncode == 0, err
    out = {}
    for s in SUFFIXES:
        if os.path.exists(pre + s):
            with open(pre + s) as f:
                out[s] = f.read()
    return out


def assert_same(got, want):
    assert sorted(got) == sorted(want)
    for s in want:
        assert got[s] == want[s], s


@pytest.fixture(scope="module")
def outbreaks(tmp_path_factory):
    return {name: Outbreak(tmp_path_factory.mktemp(f"outbreak_{name}"), spec) for name, spec in OUTBREAKS.items()}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("fix", list(OUTBREAKS))
def test_lo_option_against_model(outbreaks, fix, opt):
    ob = outbreaks[fix]
    args, kw = OPTIONS[opt]
    started = ob.start(opt, args, None if "reference" in kw else ob.ref)
    want, _ = ob.model(**kw)
    assert_same(finish(started), want)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fix", list(OUTBREAKS))
def test_lo_missing_at_its_boundary(outbreaks, fix):
    """-m exactly at an occurring ratio f32(j / S) and at the next float32 below, each given as its shortest repr so that strtof and
    the model's f32(float(s)) agree"""
    ob = outbreaks[fix]
    at = np.float32(BOUNDARY_J[fix] / ob.S)
    want = {}
    for tag, x in (("at", at), ("below", np.nextafter(at, np.float32(0)))):
        s = str(x)
        assert np.float32(s) == x and M.f32(float(s)) == float(x), s
        started = ob.start(f"m_{tag}", ("-m", s), ob.ref)
        want[tag], _ = ob.model(missing=float(s))
        assert_same(finish(started), want[tag])
    assert want["at"] != want["below"], "no site has the boundary's missing count"


@pytest.mark.timeout(600)
@pytest.mark.parametrize("opt", ["defaults", "d6"])
@pytest.mark.parametrize("fix", list(OUTBREAKS))
def test_lo_thread_counts_agree(outbreaks, fix, opt):
    ob = outbreaks[fix]
    args, kw = OPTIONS[opt]
    one, eight = ob.start(f"{opt}_t1", args, ob.ref, threads="1"), ob.start(f"{opt}_t8", args, ob.ref, threads="8")
    want, _ = ob.model(**kw)
    assert_same(finish(one), want)
    assert_same(finish(eight), want)


@pytest.mark.timeout(600)
def test_lo_options_are_not_vacuous(outbreaks):
    """each option changes the model's output on some outbreak, so that the runs above test it"""
    for flag, opts in (("-m", ("m0", "m0.5")), ("-d", ("d1", "d2", "d6")), ("-n", ("n0", "n5")), ("-r", ("no_ref",))):
        assert any(ob.model(**OPTIONS[o][1])[0] != ob.model()[0] for ob in outbreaks.values() for o in opts), flag


def _reference_variant(ob, variant):
    with open(ob.ref) as f:
        anc = f.read().split("\n")[1]
    if variant == "wrapped_lowercase":
        lines = [anc[i:i + 60] for i in range(0, len(anc), 60)]
        return ">ref wrapped\n" + "\n".join(x.lower() if i % 2 else x for i, x in enumerate(lines)) + "\n"
    if variant == "n_run":
        p = next(p for kind, p, _, _ in ob.events if kind == "snp")
        return ">ref\n" + anc[:p - 12] + "N" * 8 + anc[p - 4:] + "\n"
    return ">ref\n" + anc[:len(anc) // 2] + "\n"       # truncated


@pytest.mark.timeout(600)
@pytest.mark.parametrize("variant", ["wrapped_lowercase", "n_run", "truncated"])
def test_lo_reference_variants(outbreaks, variant):
    ob = outbreaks["A"]
    path = ob.dir / f"ref_{variant}.fa"
    with open(path, "w") as f:
        f.write(_reference_variant(ob, variant))
    started = ob.start(f"ref_{variant}", (), str(path))
    want, counts = ob.model(reference=str(path))
    assert_same(finish(started), want)
    if variant == "truncated":
        assert counts["unpositioned"] > 0


@pytest.mark.timeout(300)
def test_lo_reference_of_two_records(outbreaks):
    ob = outbreaks["A"]
    with open(ob.ref) as f:
        text = f.read()
    with open(ob.dir / "ref_two.fa", "w") as f:
        f.write(text + ">second\nACGTACGTACGT\n")
    r = LC.ska("lo", ob.skf, "two", "-r", str(ob.dir / "ref_two.fa"), cwd=ob.dir, timeout=300)
    assert r.returncode != 0
    assert "more than one sequence detected in the reference genome file" in r.stderr
