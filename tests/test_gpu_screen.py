"""skx_array_screen / skh_screen / `ska screen` (`-m gpu`), through skx_engine.py and the executable, against tests/screen_model.py (held against
the oracle's `ska map` and `weed --reverse`, a hand-worked example and a plain-loop restatement by tests/test_screen_model.py on the CPU).  All
counts are integers: the arrays must be equal.  The shapes come from the kernel as built: a workgroup walks SCREEN_TILE = 1 024 consecutive hit
windows for SCREEN_SAMPLES = 256 samples, a lane a sample, eight loads in flight."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import screen_model as SM
import subset_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
LETTERS = np.frombuffer(b"-ACMTWYHGRSVKDBN", np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)
TILE, BLOCK = 1024, 256


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    assert (eng.SCREEN_TILE, eng.SCREEN_SAMPLES) == (TILE, BLOCK), "the hit counts and sample counts below are placed around these"
    return eng


def _random(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


def _write(path, panel):
    with open(path, "wb") as f:
        for i, s in panel:
            f.write(b">" + i.encode() + b" panel record\n" + s + b"\n")
    return str(path)


def _panel(lens, seed):
    rng = np.random.default_rng(seed)
    return [(f"rec{i:05d}", _random(rng, n)) for i, n in enumerate(lens)]


def _array_for(E, panel, S, k, seed, hits=0.5, rc=True, windows=None):
    """an array whose keys are the split k-mers of some of the panel's windows -- a fraction `hits` of them, or exactly the windows whose flat
    indices `hits` lists -- and whose cells are half the panel's own middle base (on the canonical strand), half any of the 16 letters"""
    rng = np.random.default_rng(seed)
    windows = windows if windows is not None else SM.record_windows(panel, k, rc)
    flat = [(seq, w) for (_, seq), ws in zip(panel, windows) for w in ws]
    if isinstance(hits, float):
        pick = np.flatnonzero(rng.random(len(flat)) < hits)
    else:
        pick = np.asarray(hits, np.int64)
    chosen = {}
    for i in pick:
        seq, (pos, split, is_rc) = flat[i]
        base = seq[pos] & 0xDF
        chosen.setdefault(split, SM._RC[base] if is_rc else base)
    splits = list(chosen)
    order = rng.permutation(len(splits))
    keys = np.zeros(len(splits), E.KEY_DT)
    var = LETTERS[rng.integers(0, 16, size=(len(splits), S))]
    for at, j in enumerate(order):
        keys[at] = (splits[j] & ((1 << 64) - 1), splits[j] >> 64)
        own = rng.random(S) < 0.5
        var[at, own] = chosen[splits[j]]
    return E.Array.from_host(k, rc, [f"s{i:04d}" for i in range(S)], keys, var), keys, var


def _check(E, arr, keys, var, k, rc, panel, path, mutants_differ=()):
    ids, records, cells = arr.screen(_write(path, panel))
    want_rec, want = SM.screen(keys, var, k, rc, panel)
    assert ids == [i for i, _ in panel]
    assert records.dtype == E.SCREEN_RECORD_DT and cells.dtype == E.SCREEN_CELL_DT and cells.shape == want.shape[:2]
    assert records.tolist() == want_rec.tolist()
    got = np.stack([cells["found"], cells["match"], cells["ambig"]], axis=2)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    for mutant in mutants_differ:                                       # the input reaches the edge the mutant stands for
        assert not np.array_equal(SM.screen(keys, var, k, rc, panel, mutant)[1], want), mutant
    return records, got


# ---- (a) the cases of subset_model: 64- and 128-bit look-ups, engine order and exported order, both strands and one
@pytest.mark.parametrize("case", sorted(M.CASES))
def test_cases_of_subset_model(E, case, tmp_path):
    k, names, recs = M.CASES[case]["k"], M.names_of(case), M.records(case)
    rng = np.random.default_rng(len(case))
    panel = [("own_a", recs[0][0][:1500]), ("own_b", recs[min(5, len(recs) - 1)][-1][:1500]), ("foreign", _random(rng, 300))]
    arr = E.DictSet.build([E.record_stream(r) for r in recs], k, True).merge(names)
    keys, var, counts = arr.export()
    records, got = _check(E, arr, keys, var, k, True, panel, tmp_path / "p.fa", mutants_differ=("no_rc_iupac", "gap_cells_found"))      # engine order
    assert records["rows_hit"][0] > 0 and got[0, :, 1].max() > 0 and records["rows_hit"][0] == records["windows"][0]
    again = E.Array.from_host(k, True, names, keys, var, counts)                                                                         # exported order
    ids, rec2, cells2 = again.screen(str(tmp_path / "p.fa"))
    assert rec2.tolist() == records.tolist() and np.array_equal(np.stack([cells2[f] for f in ("found", "match", "ambig")], axis=2), got)


def test_single_strand_array(E, tmp_path):
    case = "k9"
    k, names, recs = 9, M.names_of(case), M.records(case)
    panel = [("own_a", recs[0][0][:1200]), ("own_b", recs[4][1]), ("foreign", _random(np.random.default_rng(3), 200))]
    arr = E.DictSet.build([E.record_stream(r) for r in recs], k, False).merge(names)
    assert not arr.rc
    keys, var, _ = arr.export()
    _check(E, arr, keys, var, k, False, panel, tmp_path / "p.fa")
    assert not any(w[2] for ws in SM.record_windows(panel, k, False) for w in ws)


# ---- (b) samples: around a wave and past a sample block; all 16 codes and gaps; about half the windows hit
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, BLOCK + 1])
def test_samples(E, S, tmp_path):
    panel = _panel([300, 47, 520], seed=S)
    arr, keys, var = _array_for(E, panel, S, 31, seed=S + 1)
    records, got = _check(E, arr, keys, var, 31, True, panel, tmp_path / "p.fa", mutants_differ=("no_rc_iupac", "gap_cells_found") if S > 2 else ())
    hit, windows = int(records["rows_hit"].sum()), int(records["windows"].sum())
    assert 0.3 * windows < hit < 0.7 * windows
    if S >= 63:
        assert set(np.unique(var)) == set(LETTERS.tolist())


# ---- (c) hit windows: at the tile, one either side, three tiles and a ragged fourth
@pytest.mark.parametrize("H", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_hit_counts_around_the_tile(E, H, tmp_path):
    panel = _panel([700, 40, 2 * H + 100 - 740 + 3 * 30], seed=H)     # 2 H + 100 windows in three records
    windows = SM.record_windows(panel, 31, True)
    n = sum(len(ws) for ws in windows)
    assert n == 2 * H + 100 and len({w[1] for ws in windows for w in ws}) == n                   # every split k-mer once: a chosen window a hit
    pick = np.sort(np.random.default_rng(H).permutation(n)[:H])
    arr, keys, var = _array_for(E, panel, 5, 31, seed=H + 1, hits=pick, windows=windows)
    records, _ = _check(E, arr, keys, var, 31, True, panel, tmp_path / "p.fa")
    assert int(records["rows_hit"].sum()) == H


def test_records_against_tile_edges(E, tmp_path):
    """every window of to_the_edge, three_tiles and after hits.  to_the_edge ends exactly on the first tile's edge; three_tiles spans the second,
    third and fourth tile, and shares the fourth with after; records without a window stand first, last and in between, and never_hits has
    windows none of which hits"""
    k = 31
    lens = [0, TILE + k - 1, 2 * TILE + 50 + k - 1, k, 200, 90, 10, 0]
    panel = _panel(lens, seed=77)
    panel = [("none_first", panel[0][1]), ("to_the_edge", panel[1][1]), ("three_tiles", panel[2][1]), ("k_letters", panel[3][1]), ("after", panel[4][1]),
             ("never_hits", panel[5][1]), ("short", panel[6][1]), ("none_last", panel[7][1])]
    windows = SM.record_windows(panel, k, True)
    assert [len(ws) for ws in windows] == [0, TILE, 2 * TILE + 50, 0, 170, 60, 0, 0]
    flat_rec = np.repeat(np.arange(len(panel)), [len(ws) for ws in windows])
    arr, keys, var = _array_for(E, panel, 70, k, seed=78, hits=np.flatnonzero(flat_rec != 5), windows=windows)
    records, got = _check(E, arr, keys, var, k, True, panel, tmp_path / "p.fa")
    assert records["rows_hit"].tolist() == [0, TILE, 2 * TILE + 50, 0, 170, 0, 0, 0] and records["length"].tolist() == lens
    assert not got[[0, 3, 5, 6, 7]].any() and got[1].any() and got[2].any() and got[4].any()


def test_thousands_of_short_records(E, tmp_path):
    """4 000 records of two windows each in one call: hundreds of record changes inside a tile, and every tile's last record shared with the next
    tile whenever an odd number of hits precedes it"""
    k = 9
    panel = _panel([k + 1] * 4000, seed=9)
    windows = SM.record_windows(panel, k, True)
    assert all(len(ws) == 2 for ws in windows)
    arr, keys, var = _array_for(E, panel, 66, k, seed=10, hits=0.6, windows=windows)
    records, got = _check(E, arr, keys, var, k, True, panel, tmp_path / "p.fa", mutants_differ=("distinct_kmers",))
    assert int(records["rows_hit"].sum()) > 4 * TILE and (records["rows_hit"] == 1).sum() > 100       # (k = 9: split k-mers recur, so most windows hit)


# ---- (d) nothing to find
def test_no_window_hits_and_no_rows(E, tmp_path):
    panel = _panel([400, 0, 90], seed=21)
    other = _panel([600], seed=22)
    arr, keys, var = _array_for(E, other, 7, 31, seed=23, hits=1.0)
    records, got = _check(E, arr, keys, var, 31, True, panel, tmp_path / "p.fa")
    assert not got.any() and not records["rows_hit"].any() and records["windows"].tolist() == [370, 0, 60]
    empty = E.Array.from_host(31, True, ["a", "b", "c"], np.zeros(0, E.KEY_DT), np.zeros((0, 3), np.uint8))
    ids, records, cells = empty.screen(str(tmp_path / "p.fa"))
    assert ids == [i for i, _ in panel] and records["windows"].tolist() == [370, 0, 60] and cells.shape == (3, 3)
    assert not any(cells[f].any() for f in ("found", "match", "ambig")) and not records["rows_hit"].any()


# ---- (e) refusals, the flag, and what a call leaves behind
def test_refusals(E, tmp_path):
    panel = _panel([200, 100], seed=31)
    arr, keys, var = _array_for(E, panel, 4, 31, seed=32)

    def refused(code, text, words):
        p = tmp_path / "bad.fa"
        p.write_bytes(text)
        with pytest.raises(E.EngineError) as ei:
            arr.screen(str(p))
        assert ei.value.code == code and all(w in str(ei.value) for w in words), str(ei.value)

    refused(E.EINVAL, b"@r0\nACGTACGTAC\n+\nIIIIIIIIII\n", ["Cannot create reference from FASTQ files"])
    refused(E.EEMPTY, b">a\nACGTACGTACGTACGT\n>b\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\n", ["has no valid sequence", "bad.fa"])
    refused(E.EINVAL, b">one first\n" + panel[0][1] + b"\n>two\n" + panel[1][1] + b"\n>one again\nACGT\n", ["screen:", "one", "more than once"])
    _check(E, arr, keys, var, 31, True, panel, tmp_path / "p.fa")       # and the array still answers
    # more than 2^31 (record, sample) pairs: 65 536 samples x 32 769 records, one of them with windows
    split = SM.record_windows(panel, 31, True)[0][0][1]
    wide = E.Array.from_host(31, True, [f"s{i}" for i in range(65536)], np.array([(split & ((1 << 64) - 1), split >> 64)], E.KEY_DT), np.full((1, 65536), ord("A"), np.uint8))
    with open(tmp_path / "many.fa", "wb") as f:
        f.write(b">first\n" + panel[0][1] + b"\n" + b"".join(b">r%d\nA\n" % i for i in range(32768)))
    with pytest.raises(E.EngineError) as ei:
        wide.screen(str(tmp_path / "many.fa"))
    assert ei.value.code == E.EUNSUP and "screen:" in str(ei.value) and "2^31" in str(ei.value)


def test_a_cell_outside_the_alphabet(E, tmp_path):
    """Array.from_host refuses such a byte itself, so it is written into the device matrix behind the array's back: the kernel raises its flag
    and the call is refused; the same byte in a row no window hits, or in the row's padding, is nobody's cell"""
    S = 5
    panel = _panel([300], seed=41)
    windows = SM.record_windows(panel, 31, True)
    arr, keys, var = _array_for(E, panel, S, 31, seed=42, hits=np.arange(0, 200), windows=windows)
    other = _panel([100], seed=43)                                      # rows that no window of the panel names: their cells are never read
    extra = [w[1] for w in SM.record_windows(other, 31, True)[0]]
    keys2 = np.concatenate([keys, np.array([(x & ((1 << 64) - 1), x >> 64) for x in extra], E.KEY_DT)])
    var[:, 0] = ord("-")                                                # sample 0 tells the two kinds of row apart on the device: '-' in the
    var2 = np.concatenate([var, np.full((len(extra), S), ord("N"), np.uint8)])      # rows the panel hits, 'N' in the others
    arr = E.Array.from_host(31, True, [f"s{i}" for i in range(S)], keys2, var2)
    path = tmp_path / "p.fa"
    _, want = _check(E, arr, keys2, var2, 31, True, panel, path)
    hip = ctypes.CDLL("libamdhip64.so.7")                               # the runtime the engine itself is linked against (already mapped)
    p, pitch, rows = arr.device_matrix()
    U = len(keys2)
    assert rows == U and pitch >= U
    first = np.zeros(U, np.uint8)                                       # sample 0's cells in the device's own row order
    assert hip.hipMemcpy(ctypes.c_void_p(first.ctypes.data), ctypes.c_void_p(int(p)), ctypes.c_size_t(U), 2) == 0      # hipMemcpyDeviceToHost
    assert sorted(first.tolist()) == sorted(var2[:, 0].tolist())
    hit_row, other_row = int(np.flatnonzero(first == ord("-"))[17]), int(np.flatnonzero(first == ord("N"))[-1])
    x = np.array([ord("X")], np.uint8)

    def poke(sample, row, byte):
        """-> the byte that was there"""
        at = ctypes.c_void_p(int(p) + sample * pitch + row)
        assert hip.hipMemcpy(ctypes.c_void_p(x.ctypes.data), at, ctypes.c_size_t(1), 2) == 0      # hipMemcpyDeviceToHost
        old = int(x[0])
        x[0] = byte
        assert hip.hipMemcpy(at, ctypes.c_void_p(x.ctypes.data), ctypes.c_size_t(1), 1) == 0      # hipMemcpyHostToDevice
        return old

    def counts():
        cells = arr.screen(str(path))[2]
        return np.stack([cells[f] for f in ("found", "match", "ambig")], axis=2)

    pad = poke(2, U, ord("X")) if pitch > U else None                   # the first byte of sample 2's padding
    assert poke(3, other_row, ord("X")) == ord("N")                     # a row no window names
    assert np.array_equal(counts(), want)
    was = poke(2, hit_row, ord("X"))                                    # a row the panel hits
    with pytest.raises(E.EngineError) as ei:
        arr.screen(str(path))
    assert ei.value.code == E.EINVAL and "screen:" in str(ei.value)
    poke(2, hit_row, was)
    poke(3, other_row, ord("N"))
    if pad is not None:
        poke(2, U, pad)
    assert np.array_equal(counts(), want)


def test_identical_calls_give_identical_bytes(E, tmp_path):
    panel = _panel([10] * 1500 + [3000], seed=51)
    arr, keys, var = _array_for(E, panel, 65, 9, seed=52, hits=0.5)
    path = _write(tmp_path / "p.fa", panel)
    before = arr.export()
    first, second = arr.screen(path), arr.screen(path)
    assert first[0] == second[0] and first[1].tobytes() == second[1].tobytes() and first[2].tobytes() == second[2].tobytes()
    assert first[2]["found"].any() and len(first[0]) == 1501
    after = arr.export()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))                                                 # the array keeps its content
    assert sorted(map(bytes, after[1])) == sorted(map(bytes, var))


def test_host_texts_equal_the_model(E, tmp_path):
    panel = _panel([120, 0, 64, 35], seed=61)
    arr, keys, var = _array_for(E, panel, 9, 31, seed=62, hits=0.8)
    names = [f"s{i:04d}" for i in range(9)]
    ids, records, cells = arr.screen(_write(tmp_path / "p.fa", panel))
    for c, i in ((0.9, 0.0), (0.5, 0.5), (0.0, 1.0)):
        want = SM.texts(keys, var, names, 31, True, panel, c, i, matrix=True)
        got = {".screen.tsv": E.screen_text(E.SCREEN_PAIRS, ids, records, cells, names, c, i),
               ".screen.summary.tsv": E.screen_text(E.SCREEN_SUMMARY, ids, records, cells, names, c, i),
               ".screen.matrix.tsv": E.screen_text(E.SCREEN_MATRIX, ids, records, cells, names, c, i)}
        assert got == want, (c, i)
    assert 1 < want[".screen.tsv"].count("\n") < 1 + 3 * 9                # some pairs pass at identity 1, not all


# ---- (f) the executable
def _ska(*args, code=0):
    r = subprocess.run([SKA, *[str(a) for a in args]], capture_output=True, timeout=120)
    assert r.returncode == code, (args, r.returncode, r.stderr.decode()[-2000:])
    return r


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("screen")
    files = []
    recs = M.records("k9")
    for name, rs in zip(M.names_of("k9"), recs):
        p = d / f"{name}.fa"
        p.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(rs)))
        files.append(p)
    _ska("build", "-k", 9, "-o", d / "x", *files)
    rng = np.random.default_rng(8)
    cut = recs[2][0]
    panel = [("gene_a", recs[0][0][100:700]), ("gene_b", recs[6][1]), ("with_n", cut[2000:2300] + b"NN" + cut[2500:2600].lower()), ("nine", cut[:9]),
             ("elsewhere", _random(rng, 250)), ("late", recs[9][0][-500:])]
    keys, var, _ = M._oracle_array("k9").export()
    return {"dir": d, "skf": d / "x.skf", "names": M.names_of("k9"), "keys": keys, "var": var, "panel": panel, "fa": _write(d / "panel.fa", panel)}


@pytest.mark.parametrize("cover", [0, 0.5, 0.9, 1])
def test_cli_files_equal_the_model(cli, cover):
    d = cli["dir"]
    for identity in (0, 0.5, 0.9, 1):
        matrix = identity in (0, 0.9)
        out = d / f"c{int(cover * 100)}_i{int(identity * 100)}"
        _ska("screen", cli["skf"], cli["fa"], "-o", out, "--min-cover", cover, "--min-identity", identity, *(["--matrix"] if matrix else []))
        want = SM.texts(cli["keys"], cli["var"], cli["names"], 9, True, cli["panel"], cover, identity, matrix=matrix)
        assert sorted(p.name for p in d.iterdir() if p.name.startswith(out.name + ".")) == sorted(out.name + s for s in want)
        for suffix, text in want.items():
            assert (d / (out.name + suffix)).read_bytes() == text.encode(), (cover, identity, suffix)
    lines = SM.texts(cli["keys"], cli["var"], cli["names"], 9, True, cli["panel"], cover, 0)[".screen.tsv"].count("\n") - 1
    assert 0 < lines < len(cli["panel"]) * len(cli["names"])


def test_python_mirror_of_the_command(E, cli):
    d = cli["dir"]
    E.default_context().screen(cli["skf"], cli["fa"], d / "mirror", min_cover=0.5, min_identity=0.9, matrix=True)
    want = SM.texts(cli["keys"], cli["var"], cli["names"], 9, True, cli["panel"], 0.5, 0.9, matrix=True)
    assert sorted(p.name for p in d.iterdir() if p.name.startswith("mirror.")) == sorted("mirror" + s for s in want)
    for suffix, text in want.items():
        assert (d / ("mirror" + suffix)).read_bytes() == text.encode(), suffix


def test_cli_defaults_and_refusals(cli):
    d = cli["dir"]
    _ska("screen", cli["skf"], cli["fa"], "-o", d / "plain")
    want = SM.texts(cli["keys"], cli["var"], cli["names"], 9, True, cli["panel"])
    assert sorted(p.name for p in d.iterdir() if p.name.startswith("plain.")) == ["plain.screen.summary.tsv", "plain.screen.tsv"]
    for suffix, text in want.items():
        assert (d / ("plain" + suffix)).read_bytes() == text.encode(), suffix
    (d / "twice.fa").write_bytes(b">gene_a x\nACGTTGCATGCAAGT\n>gene_b\nACGTTGCATGCATGT\n>gene_a y\nACGTTGCATGCATGA\n")
    r = _ska("screen", cli["skf"], d / "twice.fa", "-o", d / "twice", code=1)
    assert b"record id gene_a occurs more than once" in r.stderr and not (d / "twice.screen.tsv").exists()
    (d / "reads.fq").write_bytes(b"@r0\nACGTTGCATGCAAGT\n+\nIIIIIIIIIIIIIII\n")
    r = _ska("screen", cli["skf"], d / "reads.fq", "-o", d / "reads", code=1)
    assert b"Cannot create reference from FASTQ files" in r.stderr and not (d / "reads.screen.tsv").exists()
