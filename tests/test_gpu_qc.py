"""skx_array_sample_qc / skh_qc / `ska qc` (`-m gpu`), through skx_engine.py and the executable, against tests/qc_model.py (held against the
oracle, curve_model and a hand-worked example by tests/test_qc_model.py on the CPU).  All counts are integers: the arrays must be equal.  The
shapes come from the kernels as built: 16 rows a lane and four loads in flight in both, skx_engine.QC_TILE_ROWS rows and QC_SAMPLES samples a
workgroup of the second."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import curve_model as CM
import qc_model as Q
import subset_model as M
from test_qc_model import HAND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
FREQS = (0.0, 1e-9, 0.5, 0.9, 1.0)
LETTERS = np.frombuffer(b"-ACMTWYHGRSVKDBN", np.uint8)
AMBIGUOUS = np.frombuffer(b"MRWSYKVHDB", np.uint8)
ROWS_A_LANE = 16


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def _planted(S):
    """the rows of the hand-worked example for S samples (at S = 4 the example itself): an A/C tie and a T/G tie for major, ambiguous cells
    only, one cell, a plain base alone among ambiguous cells, a row with exactly ceil(S / 2) cells, two bases once each, no cell"""
    if S == 4:
        return HAND.copy()
    r = np.full((8, S), ord("-"), np.uint8)
    r[0] = np.frombuffer(b"AC", np.uint8)[np.arange(S) % 2]
    r[1] = np.frombuffer(b"GT", np.uint8)[np.arange(S) % 2]
    r[2] = AMBIGUOUS[np.arange(S) % len(AMBIGUOUS)]
    r[3, S // 2] = ord("G")
    r[4] = ord("N")
    r[4, S - 1] = ord("A")
    half = -(-S // 2)
    r[5, :half] = ord("A")
    r[5, half - 1] = ord("C")
    r[6, 0] = ord("A")
    r[6, S - 1] = ord("C")
    return r


def _synthetic(S, U, seed):
    """a base per row, in a third of the rows a second base in some samples, gaps, a little noise of all 16 letters -- and, from 8 rows on, the
    planted rows at the start and, from 16 on, again (reversed) in the last lane's rows"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    var = np.repeat(acgt[rng.integers(0, 4, size=(U, 1))], S, axis=1)
    second = (rng.random((U, 1)) < 0.33) & (rng.random((U, S)) < 0.4)
    var[second] = np.broadcast_to(acgt[rng.integers(0, 4, size=(U, 1))], (U, S))[second]
    var[rng.random((U, S)) < 0.3] = ord("-")
    var[(rng.random((U, 1)) < 0.1) & (rng.random((U, S)) < 0.8)] = ord("-")        # rows few samples have
    noise = rng.random((U, S)) < 0.02
    var[noise] = LETTERS[rng.integers(0, 16, size=int(noise.sum()))]
    if U >= 8:
        var[:8] = _planted(S)
    if U >= 16:
        var[U - 8:] = _planted(S)[::-1]
    return var


def _from_host(E, var, k=31):
    U, S = var.shape
    keys = np.zeros(U, E.KEY_DT)
    keys["lo"] = np.arange(U, dtype=np.uint64) * 3 + 5
    return E.Array.from_host(k, True, [f"s{i:05d}" for i in range(S)], keys, var)


def _check(arr, var, freqs=FREQS, where=None):
    for f in freqs:
        got, info = arr.sample_qc(f)
        want, winfo = Q.sample_qc(var, f)
        assert got.dtype == Q.SAMPLE_DT and got.shape == want.shape, (where, f)
        for field in Q.COUNTS:
            assert np.array_equal(got[field], want[field]), (where, f, field, np.flatnonzero(got[field] != want[field])[:5].tolist())
        assert [int(info[x]) for x in Q.INFO] == [int(winfo[x]) for x in Q.INFO], (where, f)


# ---- (a) rows: around the 16 rows of a lane and the tile of a workgroup ----
@pytest.mark.parametrize("U", [0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 1234])
def test_rows(E, U):
    assert E.QC_TILE_ROWS == 4096 and ROWS_A_LANE == 16, "the row counts above are placed around these"
    S = 6
    var = _synthetic(S, U, U + 1)
    arr = _from_host(E, var)
    _check(arr, var, where=U)
    if U == 0:
        got, info = arr.sample_qc(0.9)
        assert not any(got[f].any() for f in Q.COUNTS) and [int(info[x]) for x in Q.INFO] == [0, 0, 0, 0, 6]       # threshold still set
    if U >= 16:                                                         # what was planted is there to be counted
        want, winfo = Q.sample_qc(var, 0.5)
        assert want["singletons"][S // 2] >= 2 and want["private_alleles"][0] >= 2 and want["minor_alleles"].sum() > 0 and want["ambiguous"].min() >= 2
        assert int(winfo["rows_present"]) < U and 0 < int(winfo["core_variant_rows"]) < int(winfo["core_rows"])


# ---- (b) samples: around the four loads in flight and the samples of a workgroup ----
@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 2 * 64 + 3])
def test_samples(E, S):
    assert E.QC_SAMPLES == 64, "the sample counts above are placed around this block"
    var = _synthetic(S, 40, 100 + S)
    _check(_from_host(E, var), var, where=S)


def test_hand_worked_example_on_the_device(E):
    got, info = _from_host(E, HAND).sample_qc(0.7)
    assert Q.as_lists(got, info) == Q.as_lists(*Q.sample_qc(HAND, 0.7))
    assert [int(x) for x in got["minor_alleles"]] == [0, 0, 3, 2] and [int(x) for x in got["private_alleles"]] == [1, 0, 2, 0]


def test_three_hundred_samples_and_a_row_that_is_a_throughout(E):
    """an 8-bit counter per row would wrap at 256"""
    S, U = 300, 33
    var = _synthetic(S, U, 300)
    var[10] = ord("A")
    var[11] = ord("A")
    var[11, 299] = ord("G")
    _check(_from_host(E, var), var, freqs=(0.0, 0.9, 1.0), where=S)
    want, info = Q.sample_qc(var, 1.0)
    assert int(info["core_rows"]) >= 2 and want["private_alleles"][299] >= 1


def test_many_samples_many_rows(E):
    S, U = 70, 2 * 4096 + 77
    var = _synthetic(S, U, 65)
    assert set(np.unique(Q.CODE[var])) == set(range(16))
    _check(_from_host(E, var), var, freqs=(0.5, 0.9), where=(S, U))


def test_the_most_samples_taken_and_one_more_refused(E):
    S, U = 65535, 17
    rng = np.random.default_rng(17)
    var = np.frombuffer(b"ACGT-N", np.uint8)[rng.integers(0, 6, size=(U, S))]
    var[3] = ord("A")                                                   # c[A] = 65 535: the 16-bit counter's last value
    var[4] = ord("-")
    var[4, S - 1] = ord("T")
    arr = _from_host(E, var)
    _check(arr, var, freqs=(0.2, 1.0), where=S)
    got, info = arr.sample_qc(1.0)
    assert int(info["core_rows"]) == 1 and (got["core_present"] == 1).all() and int(got["singletons"][S - 1]) == 1
    wide = _from_host(E, np.full((1, 65536), ord("A"), np.uint8))
    with pytest.raises(E.EngineError) as ei:
        wide.sample_qc(0.9)
    assert ei.value.code == E.EUNSUP and "] qc:" in str(ei.value), str(ei.value)


# ---- (c) refusals ----
def test_refusals(E):
    var = _synthetic(6, 40, 6)
    arr = _from_host(E, var)
    for f in (float("nan"), 1.5, -0.1, float("inf")):
        with pytest.raises(E.EngineError) as ei:
            arr.sample_qc(f)
        assert ei.value.code == E.EINVAL and "] qc:" in str(ei.value), str(ei.value)
    lib = E.load_library()
    rec = np.zeros(6, E.QC_SAMPLE_DT)
    info = np.zeros(1, E.QC_INFO_DT)
    for a, r in ((None, rec.ctypes.data), (arr.h, None)):
        assert lib.skx_array_sample_qc(a, 0.9, r, info.ctypes.data) == E.EINVAL and lib.skx_last_error().startswith(b"qc:")
    assert lib.skx_array_sample_qc(arr.h, 0.9, rec.ctypes.data, None) == E.OK                   # info may be NULL
    assert np.array_equal(rec, Q.sample_qc(var, 0.9)[0])
    _check(arr, var, freqs=(0.9,), where="after the refusals")


@pytest.mark.parametrize("where", ["last_row", "last_sample"])
def test_a_cell_outside_the_alphabet(E, where):
    """Array.from_host refuses such a byte itself, so it is written into the device matrix behind the array's back: the first kernel raises its
    flag and the call is refused; the same byte in the row's padding (past the last row) is nobody's cell"""
    S, U = 5, 4096 + 20
    var = _synthetic(S, U, 12)
    arr = _from_host(E, var)
    _check(arr, var, freqs=(0.9,), where="before")
    # the runtime the engine itself is linked against, by the path it is already mapped from (no version number written down here)
    mapped = {l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64.so" in l}
    assert len(mapped) == 1, mapped
    hip = ctypes.CDLL(mapped.pop())
    p, pitch, rows = arr.device_matrix()
    assert rows == U and pitch >= U + 256
    x = np.array([ord("X")], np.uint8)

    def poke(sample, row, byte):
        x[0] = byte
        assert hip.hipMemcpy(ctypes.c_void_p(int(p) + sample * pitch + row), ctypes.c_void_p(x.ctypes.data), ctypes.c_size_t(1), 1) == 0      # hipMemcpyHostToDevice

    sample, row = (2, U - 1) if where == "last_row" else (S - 1, 7)
    poke(sample, U, ord("X"))                                           # the first byte of that sample's padding
    _check(arr, var, freqs=(0.9,), where="padding")
    poke(sample, row, ord("X"))
    with pytest.raises(E.EngineError) as ei:
        arr.sample_qc(0.9)
    assert ei.value.code == E.EINVAL and "] qc:" in str(ei.value)
    poke(sample, row, int(var[row, sample]))
    _check(arr, var, freqs=(0.9,), where="restored")


# ---- (d) consistency with what the engine already answers ----
def test_consistency_with_sample_kmers_curve_and_export(E):
    S, U = 11, 4096 + 301
    var = _synthetic(S, U, 11)
    arr = _from_host(E, var)
    before = arr.export()
    for f in FREQS:
        got, info = arr.sample_qc(f)
        assert np.array_equal(got["kmers"].astype(np.int64), np.asarray(arr.sample_kmers(), np.int64))
        last = arr.curve(np.arange(S, dtype=np.int32), f)[0, -1]
        assert (int(info["rows_present"]), int(info["core_rows"]), int(info["core_variant_rows"])) == (int(last[0]), int(last[1]), int(last[3])), f
        assert int(info["threshold"]) == int(CM.thresholds(S, f)[-1]) and int(info["rows"]) == U
    a, b = arr.sample_qc(0.9), arr.sample_qc(0.9)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    after = arr.export()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))    # the array keeps its content


# ---- (e) provenance: as merged from a dictset (pieces, or lazily held), loaded from .skf at both key widths, after a merge ----
@pytest.mark.parametrize("case", ["k31", "k41"])
def test_provenance(E, case, tmp_path):
    k, names = M.CASES[case]["k"], M.names_of(case)
    streams = [E.record_stream(r) for r in M.records(case)]
    arr = E.DictSet.build(streams, k, True).merge(names)
    first = arr.sample_qc(0.9)                                          # on the array as the merge left it
    _, var, _ = arr.export()
    want = Q.sample_qc(var, 0.9)
    assert Q.as_lists(*first) == Q.as_lists(*want)
    assert Q.as_lists(*first) == Q.as_lists(*Q.sample_qc(M.oracle_export(case), 0.9))          # rows in another order: the same counts
    _check(arr, var, freqs=(0.0, 0.6, 1.0), where=case)
    assert first[0]["private_alleles"].sum() > 0 and first[0]["minor_alleles"].sum() > 0 and first[0]["ambiguous"].sum() > 0
    arr.save_skf(str(tmp_path / case))
    loaded = E.Array.load(str(tmp_path / f"{case}.skf"))
    _check(loaded, loaded.export()[1], freqs=(0.9,), where=(case, "loaded"))
    assert Q.as_lists(*loaded.sample_qc(0.9)) == Q.as_lists(*want)
    half = len(names) // 2
    left = E.DictSet.build(streams[:half], k, True).merge(names[:half])
    right = E.DictSet.build(streams[half:], k, True).merge(names[half:])
    merged = E.Array.merge([left, right])
    _check(merged, merged.export()[1], freqs=(0.9,), where=(case, "merged"))
    assert Q.as_lists(*merged.sample_qc(0.9)) == Q.as_lists(*want)


# ---- (f) the executable ----
def _ska(*args, ok=True, cwd=None):
    r = subprocess.run([SKA, *[str(a) for a in args]], capture_output=True, timeout=120, cwd=cwd)
    assert (r.returncode == 0) == ok, (args, r.stderr.decode()[-2000:])
    return r


def family(n=8, L=3000, seed=4):
    """n samples of one ancestor in pairs, each pair with three point mutations of its own far apart, and one sample of another sequence
    altogether -> ([names], [one record each])"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    anc = acgt[rng.integers(0, 4, size=L)]
    recs = []
    for i in range(n):
        s = anc.copy()
        for j in range(3):
            p = 200 + 100 * (i // 2) + 900 * j
            s[p] = acgt[(int(np.flatnonzero(acgt == s[p])[0]) + 1) % 4]
        recs.append(s.tobytes())
    recs.append(acgt[rng.integers(0, 4, size=L)].tobytes())
    return [f"m{i}" for i in range(n)] + ["foreign"], recs


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("qc")
    names, recs = family()
    files = []
    for name, rec in zip(names, recs):
        p = d / f"{name}.fa"
        p.write_bytes(b">r\n" + rec + b"\n")
        files.append(p)
    _ska("build", "-k", 15, "-o", d / "x", *files)
    return {"dir": d, "skf": d / "x.skf", "names": names}


def test_cli_files_equal_the_model_and_delete_takes_the_flagged_list(E, cli):
    d, names = cli["dir"], cli["names"]
    arr = E.Array.load(str(cli["skf"]))
    assert arr.names == names
    var = arr.export()[1]
    _ska("qc", cli["skf"], "-o", d / "out", "--min-freq", 0.8)
    want = Q.texts_of(var, names, min_freq=0.8, M=5.0)
    assert sorted(p.name for p in d.iterdir() if p.name.startswith("out.")) == sorted("out" + s for s in want)
    for suffix, text in want.items():
        assert (d / ("out" + suffix)).read_bytes() == text.encode(), suffix
    assert want[".qc.flagged.txt"] == "foreign\n"                       # the planted sample and nobody else
    line = [l for l in want[".qc.tsv"].splitlines() if l.startswith("foreign\t")][0]
    assert "singletons" in line.split("\t")[-1] and "core_missing" in line.split("\t")[-1]
    _ska("qc", cli["skf"], "-o", d / "lax", "--mad", 1e9)                # nobody is that far out: the list is written, and empty
    assert (d / "lax.qc.flagged.txt").read_bytes() == b"" and (d / "lax.qc.tsv").read_bytes() == Q.texts_of(var, names, 0.9, 1e9)[".qc.tsv"].encode()
    _ska("delete", "-s", cli["skf"], "-f", d / "out.qc.flagged.txt", "-o", d / "clean")
    assert E.Array.load(str(d / "clean.skf")).names == names[:-1]
    r = _ska("qc", d / "missing.skf", "-o", d / "none", ok=False)
    assert not [p for p in d.iterdir() if p.name.startswith("none.")], r.stderr
