"""skx_array_curve / skh_curve / `ska curve` (`-m gpu`), through skx_engine.py and the executable, against tests/curve_model.py (held against
subset_model, the oracle chain and a hand-worked example by tests/test_curve_model.py on the CPU).  All counts are integers: the arrays must be
equal.  The shapes come from the kernel as built (skx_engine.CURVE_*: 16 rows a thread, CURVE_TILE_ROWS a workgroup, CURVE_LDS_STEPS steps of
counters on chip, CURVE_BATCH_ORDERS orders and 2^22 (order, step) pairs a launch, four loads in flight)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import curve_model as CM
import subset_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
FREQS = (0.0, 1e-9, 0.5, 0.9, 1.0)
LETTERS = np.frombuffer(b"-ACMTWYHGRSVKDBN", np.uint8)
AMBIGUOUS = np.frombuffer(b"MRWSYKVHDB", np.uint8)


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def _synthetic(S, U, seed):
    """a base per row, in a third of the rows a second base in some samples, gaps, a little noise of all 16 letters -- and, from six rows on,
    planted rows: no cell present, only ambiguous cells, only N, a second base in the last sample alone, in the first sample alone, one cell"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    var = np.repeat(acgt[rng.integers(0, 4, size=(U, 1))], S, axis=1)
    second = (rng.random((U, 1)) < 0.33) & (rng.random((U, S)) < 0.4)
    var[second] = np.broadcast_to(acgt[rng.integers(0, 4, size=(U, 1))], (U, S))[second]
    var[rng.random((U, S)) < 0.3] = ord("-")
    var[(rng.random((U, 1)) < 0.1) & (rng.random((U, S)) < 0.8)] = ord("-")        # rows few samples have
    noise = rng.random((U, S)) < 0.02
    var[noise] = LETTERS[rng.integers(0, 16, size=int(noise.sum()))]
    if U >= 6:
        var[0] = ord("-")
        var[1] = AMBIGUOUS[np.arange(S) % len(AMBIGUOUS)]
        var[1, S // 2] = ord("-") if S > 2 else var[1, S // 2]
        var[2] = ord("N")
        var[3] = ord("A")
        var[3, S - 1] = ord("C")
        var[4] = ord("A")
        var[4, 0] = ord("C")
        var[5] = ord("-")
        var[5, S // 2] = ord("G")
    return var


def _from_host(E, var, k=31):
    U, S = var.shape
    keys = np.zeros(U, E.KEY_DT)
    keys["lo"] = np.arange(U, dtype=np.uint64) * 3 + 5
    return E.Array.from_host(k, True, [f"s{i:04d}" for i in range(S)], keys, var)


def _orders(S, seed=3, n=3):
    return np.concatenate([np.arange(S, dtype=np.int32)[None], np.arange(S, dtype=np.int32)[::-1][None], CM.orders(seed, S, n)])


def _check(arr, var, orders, freqs=FREQS, where=None):
    for f in freqs:
        got = arr.curve(orders, f)
        want = CM.curve(var, orders, f)
        assert got.dtype == np.uint64 and got.shape == want.shape, (where, f)
        assert np.array_equal(got, want), (where, f, np.argwhere(got != want)[:5].tolist())


# ---- (a) rows: around the 16 rows of a thread and the tile of a workgroup ----
@pytest.mark.parametrize("U", [0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 1234])
def test_rows(E, U):
    tile = E.CURVE_TILE_ROWS
    assert tile == 4096, "the row counts above are placed around this tile"
    S = 6
    var = _synthetic(S, U, U + 1)
    arr = _from_host(E, var)
    _check(arr, var, _orders(S), where=U)
    if U == 0:
        assert not arr.curve(_orders(S), 0.9).any()
    if U >= 6:                                                          # what was planted is there to be counted
        ident = CM.curve(var, [np.arange(S)], 0.9)[0]
        absent = int((CM.CODE[var] == 0).all(axis=1).sum())
        assert absent >= 1 and ident[-1, 0] == U - absent and ident[-1, 2] > ident[-2, 2] and ident[0, 2] == 0


# ---- (b) samples: around the four loads in flight, a wave's worth, and the LDS counter block ----
@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 7, 8, 9, 64, 65])
def test_samples(E, S):
    var = _synthetic(S, 17, 100 + S)
    arr = _from_host(E, var)
    _check(arr, var, _orders(S), where=S)


def test_one_more_sample_than_the_counter_block(E):
    S = E.CURVE_LDS_STEPS + 1
    var = _synthetic(S, 17, 7)
    arr = _from_host(E, var)
    _check(arr, var, _orders(S, n=1), freqs=(0.5, 0.9), where=S)
    S = 2 * E.CURVE_LDS_STEPS + 3                                       # two full blocks and a ragged third
    var = _synthetic(S, 17, 8)
    _check(_from_host(E, var), var, _orders(S, n=1)[1:], freqs=(0.9,), where=S)


def test_many_samples_many_rows(E):
    S, U = 65, 2 * 4096 + 77
    var = _synthetic(S, U, 65)
    assert set(np.unique(CM.CODE[var])) == set(range(16))
    _check(_from_host(E, var), var, _orders(S, n=2), freqs=(0.5, 0.9), where=(S, U))


# ---- (c) orders ----
def test_orders_twice_one_and_more_than_a_launch(E):
    S = 5
    var = _synthetic(S, 17, 55)
    arr = _from_host(E, var)
    o = CM.orders(9, S, 1)
    twice = arr.curve(np.concatenate([o, o]), 0.9)
    assert np.array_equal(twice[0], twice[1]) and np.array_equal(twice[:1], arr.curve(o, 0.9))          # the same order twice; P = 1
    assert np.array_equal(arr.curve(o[0], 0.9), twice[:1])                                             # (a single order given flat)
    many = CM.orders(10, S, E.CURVE_BATCH_ORDERS + 1)                                                  # one order more than a launch takes
    _check(arr, var, many, freqs=(0.5,), where="batch")
    S = 4200                                                                                           # 2^22 / S = 998 orders a launch
    var = _synthetic(S, 17, 56)
    rng = np.random.default_rng(11)
    many = np.array([rng.permutation(S) for _ in range((1 << 22) // S + 1)], np.int32)
    assert len(many) <= E.CURVE_BATCH_ORDERS
    _check(_from_host(E, var), var, many, freqs=(0.9,), where="pairs")


def test_identical_calls_give_identical_bytes(E):
    S, U = 9, 2 * 4096 + 5
    var = _synthetic(S, U, 99)
    arr = _from_host(E, var)
    o = _orders(S, n=6)
    assert arr.curve(o, 0.9).tobytes() == arr.curve(o, 0.9).tobytes()
    assert np.array_equal(arr.export()[1], var)                                                        # the array keeps its content


# ---- (d) the last step ----
@pytest.mark.parametrize("f", FREQS)
def test_at_the_last_step_every_order_agrees_and_core_is_the_filter(E, f):
    S, U = 11, 4096 + 301
    var = _synthetic(S, U, 11)
    arr = _from_host(E, var)
    got = arr.curve(_orders(S, n=5), f)
    assert (got[:, -1, :] == got[0, -1, :]).all()
    thr = int(CM.thresholds(S, f)[-1])
    copy = _from_host(E, var)
    copy.filter(thr, filter_type=E.FILTER_NONE)
    assert int(got[0, -1, 1]) == copy.nrows == int((((CM.CODE[var] != 0).sum(axis=1)) >= thr).sum())
    assert got[0, -1].tolist() == CM.curve(var, [np.arange(S)], f)[0, -1].tolist()


# ---- (e) provenance: as merged from a dictset, after export / from_host, filtered while loading ----
@pytest.mark.parametrize("case", sorted(M.CASES))
def test_cases_of_subset_model(E, case, tmp_path):
    k, names = M.CASES[case]["k"], M.names_of(case)
    S = len(names)
    arr = E.DictSet.build([E.record_stream(r) for r in M.records(case)], k, True).merge(names)
    orders = _orders(S, n=2)
    first = arr.curve(orders, 0.9)                                      # on the array as the merge left it (pieces, or lazily held)
    keys, var, counts = arr.export()
    assert np.array_equal(first, CM.curve(var, orders, 0.9))
    assert np.array_equal(first, CM.curve(M.oracle_export(case), orders, 0.9))      # rows in another order: the same counts
    _check(arr, var, orders, freqs=(0.0, 0.6, 1.0), where=case)
    again = E.Array.from_host(k, True, names, keys, var, counts)
    assert np.array_equal(again.curve(orders, 0.9), first)
    assert first[:, :, 3].max() > 0 and (first[:, :, 1] < first[:, :, 0]).any()
    # an array without split k-mers: filtered while it was loaded
    arr.save_skf(str(tmp_path / case))
    opts = M.Opts((0.6, False, 1, False, False))
    filtered, _, _ = E.Array.load_filtered(str(tmp_path / f"{case}.skf"), min_freq=0.6, filter_type=E.FILTER_NO_CONST)
    _, kept = M.verdicts(var, range(S), opts)
    assert 0 < len(kept) < len(var) and filtered.nrows == len(kept)
    _check(filtered, kept, orders, freqs=(0.9,), where=(case, "load_filtered"))
    sub, _ = arr.subset_filtered([0, 2, 3, 5], min_freq=0.0, filter_type=E.FILTER_NONE)
    _, kept = M.verdicts(var, [0, 2, 3, 5], M.Opts((0.0, False, 0, False, False)))
    _check(sub, kept, _orders(4, n=1), freqs=(0.9,), where=(case, "subset_filtered"))


# ---- (f) refusals ----
def test_refusals(E):
    S = 6
    var = _synthetic(S, 40, 6)
    arr = _from_host(E, var)
    ok = _orders(S)

    def refused(code, call):
        with pytest.raises(E.EngineError) as ei:
            call()
        assert ei.value.code == code and "] curve:" in str(ei.value), str(ei.value)

    for f in (float("nan"), 1.5, -0.1, float("inf")):
        refused(E.EINVAL, lambda: arr.curve(ok, f))
    for at, value in ((0, 1), (S - 1, S), (2, -1), (3, 1 << 20)):     # a repeat, an index past the end, a negative one, a far one
        bad = ok.copy()
        bad[0, at] = value                                              # (row 0 is the identity)
        refused(E.EINVAL, lambda: arr.curve(bad, 0.9))
    refused(E.EINVAL, lambda: arr.curve(np.zeros((0, S), np.int32), 0.9))      # n_orders == 0
    lib = E.load_library()
    counts = np.zeros((1, S, 4), np.uint64)
    one = np.ascontiguousarray(ok[:1])
    for a, o, c in ((None, one.ctypes.data, counts.ctypes.data), (arr.h, None, counts.ctypes.data), (arr.h, one.ctypes.data, None)):
        assert lib.skx_array_curve(a, o, 1, 0.9, c) == E.EINVAL and lib.skx_last_error().startswith(b"curve:")
    assert np.array_equal(arr.curve(ok, 0.9), CM.curve(var, ok, 0.9))          # and the array still answers
    # more than 65 535 samples
    wide = np.full((1, 65536), ord("A"), np.uint8)
    big = _from_host(E, wide)
    refused(E.EUNSUP, lambda: big.curve(np.arange(65536, dtype=np.int32), 0.9))
    most = _from_host(E, wide[:, :65535])
    got = most.curve(np.arange(65535, dtype=np.int32), 1.0)
    assert (got[0, :, :2] == 1).all() and not got[0, :, 2:].any()


def test_a_cell_outside_the_alphabet(E):
    """Array.from_host refuses such a byte itself, so it is written into the device matrix behind the array's back: the kernel raises its flag
    and the call is refused; the same byte in the row's padding (past the last row) is nobody's cell"""
    S, U = 5, 4096 + 20
    var = _synthetic(S, U, 12)
    bad = var.copy()
    bad[U - 3, 2] = ord("X")
    with pytest.raises(E.EngineError) as ei:
        _from_host(E, bad)
    assert ei.value.code == E.EUNSUP
    arr = _from_host(E, var)
    o = _orders(S)
    want = CM.curve(var, o, 0.9)
    assert np.array_equal(arr.curve(o, 0.9), want)
    hip = ctypes.CDLL("libamdhip64.so.7")                               # the runtime the engine itself is linked against (already mapped)
    p, pitch, rows = arr.device_matrix()
    assert rows == U and pitch >= U + 256
    x = np.array([ord("X")], np.uint8)

    def poke(sample, row, byte):
        x[0] = byte
        assert hip.hipMemcpy(ctypes.c_void_p(int(p) + sample * pitch + row), ctypes.c_void_p(x.ctypes.data), ctypes.c_size_t(1), 1) == 0      # hipMemcpyHostToDevice

    poke(2, U, ord("X"))                                                # the first byte of sample 2's padding
    assert np.array_equal(arr.curve(o, 0.9), want)
    poke(2, U - 3, ord("X"))
    with pytest.raises(E.EngineError) as ei:
        arr.curve(o, 0.9)
    assert ei.value.code == E.EINVAL and "] curve:" in str(ei.value)
    poke(2, U - 3, int(var[U - 3, 2]))
    assert np.array_equal(arr.curve(o, 0.9), want)


# ---- (g) the executable ----
def _ska(*args, ok=True):
    r = subprocess.run([SKA, *[str(a) for a in args]], capture_output=True, timeout=120)
    assert (r.returncode == 0) == ok, (args, r.stderr.decode()[-2000:])
    return r


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("curve")
    files = []
    for name, recs in zip(M.names_of("k9"), M.records("k9")):
        p = d / f"{name}.fa"
        p.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
        files.append(p)
    _ska("build", "-k", 9, "-o", d / "x", *files)
    return {"dir": d, "skf": d / "x.skf", "names": M.names_of("k9"), "var": M.oracle_export("k9")}


def test_cli_seeded_files_equal_the_model(cli):
    d = cli["dir"]
    _ska("curve", cli["skf"], "-o", d / "seeded", "--seed", 7, "--permutations", 5, "--all-permutations")
    want = CM.texts(cli["var"], cli["names"], min_freq=0.9, permutations=5, seed=7, all_permutations=True)
    assert sorted(p.name for p in d.iterdir() if p.name.startswith("seeded.")) == sorted("seeded" + s for s in want)
    for suffix, text in want.items():
        assert (d / ("seeded" + suffix)).read_bytes() == text.encode(), suffix
    assert want[".curve.permutations.tsv"].count("\n") == 1 + 5 * 13
    _ska("curve", cli["skf"], "-o", d / "plain", "--min-freq", 0.5)                 # the defaults: 20 orders of seed 1, the summary alone
    assert [p.name for p in d.iterdir() if p.name.startswith("plain.")] == ["plain.curve.tsv"]
    assert (d / "plain.curve.tsv").read_bytes() == CM.texts(cli["var"], cli["names"], min_freq=0.5)[".curve.tsv"].encode()


def test_cli_order_file(cli):
    d, names = cli["dir"], cli["names"]
    order = [names[i] for i in CM.orders(4, len(names), 1)[0]]
    (d / "order.txt").write_text("".join(n + "\n" for n in order[:5]) + "\n" + "".join(n + "\r\n" for n in order[5:]))
    _ska("curve", cli["skf"], "-o", d / "dated", "--order-file", d / "order.txt", "--min-freq", 0.6)
    want = CM.texts(cli["var"], names, min_freq=0.6, order_names=order)
    for suffix, text in want.items():
        assert (d / ("dated" + suffix)).read_bytes() == text.encode(), suffix
    for lines, word in ((order[:-1] + ["nobody"], "nobody"), (order[:-1] + [order[0]], order[0]), (order[:-1], order[-1]), (order + [order[3]], order[3])):
        (d / "bad.txt").write_text("".join(n + "\n" for n in lines))
        r = _ska("curve", cli["skf"], "-o", d / "bad", "--order-file", d / "bad.txt", ok=False)
        assert r.returncode == 101 and word in r.stderr.decode() and not (d / "bad.curve.tsv").exists(), r.stderr.decode()[-500:]
