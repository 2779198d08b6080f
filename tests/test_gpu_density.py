"""skx_array_snp_density / skh_density / `ska density` (`-m gpu`), through skx_engine.py and the executable, against tests/density_model.py (held
against the oracle's `ska map`, a sliding-window restatement and a hand-worked example by tests/test_density_model.py on the CPU).  Everything is
an integer: the arrays must be equal, the files byte for byte.  The shapes come from the kernels as built: a unit of density_kernel is
DENSITY_TILE_ROWS = 4 096 rows x DENSITY_SAMPLES = 64 samples, a lane 16 rows; the passes over the sorted SNP list run in blocks of
DENSITY_SCAN_BLOCK = 4 096 records."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import density_model as DM
import map_model as MM
import subset_model as M
import test_density_model as TM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
LETTERS = np.frombuffer(b"-ACMTWYHGRSVKDBN", np.uint8)
AMBIGUOUS = np.frombuffer(b"MWYHRSVKDBN", np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)
TILE, BLOCK, SCAN = 4096, 64, 4096
FIELDS = ("info", "samples", "regions", "bins", "chrom_lens", "snps", "snp_ref")


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    assert (eng.DENSITY_TILE_ROWS, eng.DENSITY_SAMPLES, eng.DENSITY_SCAN_BLOCK) == (TILE, BLOCK, SCAN), "the rows, samples and SNP counts below are placed around these"
    return eng


def _random(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


def _write(path, ref):
    with open(path, "wb") as f:
        for i, s in ref:
            f.write(b">" + i.encode() + b" a chromosome\n" + s + b"\n")
    return str(path)


def _other(rng, base):
    return ACGT[(np.searchsorted(ACGT, base) + rng.integers(1, 4, size=base.shape)) % 4]


class World:
    """a reference and an array made for it.  The sites are the reference's windows whose split k-mer occurs once, the first n_sites of them (all
    by default); the array's rows are those split k-mers, the split k-mers of the repeated windows (rows that are nobody's site) and `foreign`
    rows no window names, in a random order.  cells [n_sites, S] holds, in reference order and as the reference's strand reads them, what every
    sample has at every site: the reference's own base to begin with"""

    def __init__(self, E, ref, S, k, seed, rc=True, n_sites=None, foreign=0):
        self.E, self.ref, self.S, self.k, self.rc, self.rng = E, ref, S, k, rc, np.random.default_rng(seed)
        wins = [MM.chrom_windows(s, k, rc) for _, s in ref]
        count = {}
        for ws in wins:
            for _, split, _ in ws:
                count[split] = count.get(split, 0) + 1
        flat = [(c, w) for c, ws in enumerate(wins) for w in ws]
        self.sites = [(c, w) for c, w in flat if count[w[1]] == 1][:n_sites]
        self.repeats = sorted({w[1] for c, w in flat if count[w[1]] > 1})
        self.foreign = [int(x) for x in self.rng.integers(1, 1 << 60, size=foreign)]
        self.base = np.array([ref[c][1][w[0]] & 0xDF for c, w in self.sites], np.uint8)
        self.cells = np.repeat(self.base[:, None], S, axis=1) if len(self.sites) else np.zeros((0, S), np.uint8)
        self.names = [f"s{i:04d}" for i in range(S)]
        others = self.repeats + self.foreign
        splits = [w[1] for _, w in self.sites] + others
        self.others = LETTERS[self.rng.integers(0, 16, size=(len(others), S))]
        self.order = self.rng.permutation(len(splits))
        self.keys = np.zeros(len(splits), E.KEY_DT)
        for at, j in enumerate(self.order):
            self.keys[at] = (splits[j] & ((1 << 64) - 1), splits[j] >> 64)
        self.row_of_site = np.argsort(self.order)[:len(self.sites)]

    def sprinkle(self, snp=0.0, gap=0.0, ambig=0.0):
        r = self.rng.random(self.cells.shape)
        other = _other(self.rng, self.cells)
        self.cells = np.where(r < snp, other, self.cells)
        self.cells[(r >= snp) & (r < snp + gap)] = ord("-")
        m = (r >= snp + gap) & (r < snp + gap + ambig)
        self.cells[m] = AMBIGUOUS[self.rng.integers(0, len(AMBIGUOUS), size=int(m.sum()))]
        return self

    def snp(self, site, sample):
        self.cells[site, sample] = _other(self.rng, self.base[site:site + 1])[0]

    def build(self):
        """the array of the cells as they stand (the rows keep their order from one call to the next); var: what it was given"""
        strand = np.array([w[2] for _, w in self.sites], bool)
        stored = np.where(strand[:, None], DM._RC[self.cells], self.cells) if len(self.sites) else self.cells
        self.var = np.ascontiguousarray(np.concatenate([stored, self.others])[self.order])
        self.arr = self.E.Array.from_host(self.k, self.rc, self.names, self.keys, self.var)
        return self

    def site_of_row(self, row):
        return int(np.flatnonzero(self.row_of_site == row)[0])


def _same(got, want, where=None):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (where, f, got[f][:8], want[f][:8])
    assert got["chrom_ids"] == want["chrom_ids"], where


def _check(w, path, W, T, where=None):
    got = w.arr.snp_density(_write(path, w.ref), W, T, snps=True)
    want = DM.density(w.keys, w.var, w.k, w.rc, w.ref, W, T)
    assert got["samples"].dtype == w.E.DENSITY_SAMPLE_DT and got["regions"].dtype == w.E.DENSITY_REGION_DT and got["bins"].dtype == w.E.DENSITY_BIN_DT
    _same(got, want, where)
    plain = w.arr.snp_density(str(path), W, T)                             # without the list: the same counts, no list
    assert plain["snps"] is None and all(np.array_equal(plain[f], want[f]) for f in ("info", "samples", "regions", "bins"))
    return got


# ---- (a) rows: none, one, around the tile; a SNP in the first and the last row of a tile and of the array
@pytest.mark.parametrize("U", [0, 1, TILE - 1, TILE, TILE + 1])
def test_rows(E, U, tmp_path):
    S, k = 3, 31
    ref = [("chr1", _random(np.random.default_rng(U), U + 90))]
    w = World(E, ref, S, k, seed=U + 1, n_sites=U).sprinkle(snp=0.25, gap=0.1, ambig=0.05)
    assert len(w.sites) == U and not w.repeats
    rows = sorted({r for r in (0, U - 1, TILE - 1, TILE) if 0 <= r < U})
    for r in rows:
        for s in (0, S - 1):
            w.snp(w.site_of_row(r), s)
    w.build()
    assert len(w.var) == U
    got = _check(w, tmp_path / "r.fa", 12, 3, where=U)
    assert int(got["info"]["sites"]) == U and int(got["info"]["windows"]) == 60 + U
    if U:
        snp_x = {(int(v) >> 34 & 0xFFFFFFF, int(v) >> 2 & 0xFFFFFFFF) for v in got["snps"]}
        for r in rows:
            c, (pos, _, _) = w.sites[w.site_of_row(r)]
            assert (0, pos) in snp_x and (S - 1, pos) in snp_x, r
    if U >= TILE - 1:
        assert len(got["regions"]) > 10 and 0 < int(got["samples"]["dense_snps"].sum()) < int(got["samples"]["snps"].sum())


# ---- (b) samples: one, around a wave and a sample block; a SNP in the first and the last sample of a block; every letter
@pytest.mark.parametrize("S", sorted({1, 63, 64, 65, BLOCK + 1, 2 * BLOCK + 1}))
def test_samples(E, S, tmp_path):
    rng = np.random.default_rng(S)
    seg = _random(rng, 60)
    ref = [("one", _random(rng, 300) + seg + b"N" + _random(rng, 80).lower()), ("none", b"ACGT"), ("two", _random(rng, 150) + seg + _random(rng, 41))]
    w = World(E, ref, S, 31, seed=S + 1, foreign=37).sprinkle(snp=0.2, gap=0.15, ambig=0.15)
    assert 30 <= len(w.repeats) <= 32 and {x[2] for _, x in w.sites} == {False, True}      # (the letters around the shared stretch may agree too)
    for s in sorted({0, S - 1, min(BLOCK - 1, S - 1), min(BLOCK, S - 1)}):
        for site in (0, 1, 2, len(w.sites) - 1):
            w.snp(site, s)
    w.build()
    got = _check(w, tmp_path / "r.fa", 15, 3, where=S)
    assert got["chrom_ids"] == ["one", "none", "two"] and got["chrom_lens"].tolist() == [441, 4, 251] and int(got["info"]["repeat_windows"]) == 2 * len(w.repeats)
    assert (got["samples"]["snps"] >= 4).all() and (got["samples"]["regions"] >= 1).all()
    assert np.array_equal(got["samples"]["missing"] + got["samples"]["ambiguous"] + got["samples"]["callable"], got["samples"]["sites"])
    if S >= 63:
        assert set(np.unique(w.var)) == set(LETTERS.tolist())
    for mutant in ("repeats_kept", "no_rc_iupac", "ambig_as_snp", "ref_case_sensitive"):      # the input reaches the edges the mutants stand for
        assert not np.array_equal(DM.density(w.keys, w.var, 31, True, ref, 15, 3, mutant)["samples"], got["samples"]), mutant


# ---- (c) units with and without SNPs side by side; no SNP at all; no site
def test_units_with_and_without_snps(E, tmp_path):
    S, U = 2 * BLOCK + 5, 2 * TILE + 100
    ref = [("chr1", _random(np.random.default_rng(3), U + 30))]
    w = World(E, ref, S, 31, seed=4)
    tile_of_site = w.row_of_site // TILE
    rng = np.random.default_rng(5)
    for tile, block in ((0, 2), (1, 0), (2, 1)):                        # three of the nine units hold SNPs
        sites = np.flatnonzero(tile_of_site == tile)
        for site in rng.choice(sites, size=40 if tile < 2 else 9, replace=False):
            for s in rng.choice(np.arange(block * BLOCK, min(S, (block + 1) * BLOCK)), size=3, replace=False):
                w.snp(int(site), int(s))
    w.build()
    got = _check(w, tmp_path / "r.fa", 400, 2)
    assert int(got["info"]["n_snps"]) == 3 * (40 + 40 + 9) and int(got["info"]["n_regions"]) > 0
    assert (got["samples"]["snps"][:BLOCK].sum(), got["samples"]["snps"][BLOCK:2 * BLOCK].sum(), got["samples"]["snps"][2 * BLOCK:].sum()) == (120, 27, 120)


def test_no_snp_and_no_site(E, tmp_path):
    ref = [("chr1", _random(np.random.default_rng(6), 500)), ("chr2", _random(np.random.default_rng(7), 90))]
    w = World(E, ref, 5, 31, seed=8).sprinkle(gap=0.2, ambig=0.2).build()
    got = _check(w, tmp_path / "r.fa", 50, 2)
    assert int(got["info"]["n_snps"]) == 0 and len(got["regions"]) == 0 and not got["bins"]["snps"].any() and got["samples"]["ambiguous"].all()
    assert int(got["info"]["sites"]) == 530 and got["snps"].shape == (0,)
    elsewhere = World(E, ref, 5, 31, seed=9, n_sites=0, foreign=300).build()         # rows, none of them a window's
    got = _check(elsewhere, tmp_path / "r.fa", 50, 2)
    assert int(got["info"]["sites"]) == 0 and int(got["info"]["windows"]) == 530 and not any(got["samples"][f].any() for f in DM.SAMPLE_DT.names)
    assert len(got["bins"]) == 10 + 2


# ---- (d) the sorted list around the scan block: a qualifying run that straddles a block, one that ends at the last record
@pytest.mark.parametrize("n", [SCAN - 1, SCAN, SCAN + 1, 2 * SCAN + 1])
def test_snp_list_sizes(E, n, tmp_path):
    S, U = 5, 2600
    ref = [("chr1", _random(np.random.default_rng(n), 1500)), ("chr2", _random(np.random.default_rng(n + 1), U + 60 - 1500))]
    w = World(E, ref, S, 31, seed=n + 2)
    assert len(w.sites) == U
    rng = np.random.default_rng(n + 3)
    fixed = [(100, 0), (400, 0), (700, 0),                              # sample 0: three SNPs far apart, none of them dense
             (U - 3, S - 1), (U - 2, S - 1), (U - 1, S - 1)]            # the list's last three records: the last sample's last three sites
    free = [(i, s) for i in range(U) for s in range(1, S) if (i, s) not in fixed]
    for j in rng.permutation(len(free))[:n - len(fixed)]:
        w.snp(*free[j])
    for i, s in fixed:
        w.snp(i, s)
    w.build()
    got = _check(w, tmp_path / "r.fa", 9, 3, where=n)
    assert int(got["info"]["n_snps"]) == n
    dense = (got["snps"] >> np.uint64(62)).astype(bool)
    sample = (got["snps"] >> np.uint64(34)) & np.uint64(0xFFFFFFF)
    assert dense[-1] and dense[-3:].all() and 0.2 * n < dense.sum() < n
    if n > SCAN:
        at = [b for b in range(SCAN, n, SCAN) if dense[b - 1] and dense[b] and sample[b - 1] == sample[b]]
        assert at, "no run of dense SNPs straddles a scan block: choose another seed"


# ---- (e) the window's edges, a run across a chromosome boundary and across two samples' adjacent records: the hand-worked example
@pytest.mark.parametrize("WT", [(12, 3), (13, 3), (12, 2), (11, 2), (12, 7), (1, 2), (1 << 31, 65535), (1 << 31, 2)])
def test_hand_worked_example_on_the_device(E, WT, tmp_path):
    W, T = WT
    keys, var = TM._hand_array()
    arr = E.Array.from_host(9, True, TM.HAND_NAMES, keys, var)
    got = arr.snp_density(_write(tmp_path / "r.fa", TM.HAND_REF), W, T, snps=True)
    _same(got, DM.density(keys, var, 9, True, TM.HAND_REF, W, T), WT)
    if WT == (12, 3):
        assert [tuple(int(x) for x in g) for g in got["regions"]] == TM.HAND_REGIONS and [tuple(int(x) for x in q) for q in got["samples"]] == TM.HAND_SAMPLES
        assert [tuple(int(x) for x in b) for b in got["bins"]] == TM.HAND_BINS
        for mutant in DM.MUTANTS:
            assert not np.array_equal(DM.density(keys, var, 9, True, TM.HAND_REF, W, T, mutant)["samples"], got["samples"]), mutant
    if WT == (12, 7):
        assert len(got["regions"]) == 0 and int(got["info"]["n_snps"]) == 15
    if WT == (1 << 31, 2):                                              # every SNP with a neighbour on its chromosome is dense; s2's lone SNP on c2 is not
        assert got["samples"]["dense_snps"].tolist() == [6, 5, 2] and [tuple(int(x) for x in g)[:2] for g in got["regions"]] == [(0, 0), (1, 0), (2, 0)]


# ---- (f) both key widths, engine order and exported order, the provenances of test_gpu_qc.py, one strand
@pytest.mark.parametrize("case", ["k31", "k41"])
def test_provenance_and_orders(E, case, tmp_path):
    k, names, recs = M.CASES[case]["k"], M.names_of(case), M.records(case)
    ref = [("genome", recs[1][0]), ("island", recs[1][1])]              # the second record repeats a stretch of the clade's founder
    path = _write(tmp_path / "r.fa", ref)
    streams = [E.record_stream(r) for r in recs]
    arr = E.DictSet.build(streams, k, True).merge(names)                # engine order, held as the merge left it
    first = arr.snp_density(path, 300, 3, snps=True)
    keys, var, counts = arr.export()
    want = DM.density(keys, var, k, True, ref, 300, 3)
    _same(first, want, (case, "merged from a dictset"))
    assert int(want["info"]["repeat_windows"]) > 100 and int(want["info"]["n_regions"]) > 0 and want["samples"]["snps"].sum() >= want["samples"]["dense_snps"].sum() > 0
    again = E.Array.from_host(k, True, names, keys, var, counts)        # exported order
    _same(again.snp_density(path, 300, 3, snps=True), want, (case, "from the host"))
    arr.save_skf(str(tmp_path / case))
    loaded = E.Array.load(str(tmp_path / f"{case}.skf"))
    lk, lv, _ = loaded.export()
    _same(loaded.snp_density(path, 300, 3, snps=True), DM.density(lk, lv, k, True, ref, 300, 3), (case, "loaded"))
    half = len(names) // 2
    merged = E.Array.merge([E.DictSet.build(streams[:half], k, True).merge(names[:half]), E.DictSet.build(streams[half:], k, True).merge(names[half:])])
    mk, mv, _ = merged.export()
    _same(merged.snp_density(path, 300, 3, snps=True), DM.density(mk, mv, k, True, ref, 300, 3), (case, "merged"))
    assert np.array_equal(merged.snp_density(path, 300, 3)["samples"], want["samples"])      # rows in another order: the same counts


def test_single_strand_array(E, tmp_path):
    k, names, recs = 9, M.names_of("k9"), M.records("k9")
    ref = [("a", recs[0][0][:1200]), ("b", recs[4][1])]
    arr = E.DictSet.build([E.record_stream(r) for r in recs], k, False).merge(names)
    assert not arr.rc
    keys, var, _ = arr.export()
    got = arr.snp_density(_write(tmp_path / "r.fa", ref), 100, 2, snps=True)
    _same(got, DM.density(keys, var, k, False, ref, 100, 2), "single strand")
    assert int(got["info"]["sites"]) > 0 and not any(x[3] for x in DM.sites(keys, k, False, ref)[2])


# ---- (g) refusals, the flag, and what a call leaves behind
def test_refusals(E, tmp_path):
    ref = [("chr1", _random(np.random.default_rng(31), 400))]
    w = World(E, ref, 4, 31, seed=32).sprinkle(snp=0.2).build()
    path = _write(tmp_path / "r.fa", ref)

    def refused(code, words, *args, file=None):
        with pytest.raises(E.EngineError) as ei:
            w.arr.snp_density(file or path, *args)
        assert ei.value.code == code and all(x in str(ei.value) for x in words), str(ei.value)

    for W, T in ((0, 5), ((1 << 31) + 1, 5)):
        refused(E.EINVAL, ["] density:", "window"], W, T)
    for W, T in ((1000, 1), (1000, 0), (1000, 65536)):
        refused(E.EINVAL, ["] density:", "min_snps"], W, T)

    def file(name, text):
        (tmp_path / name).write_bytes(text)
        return str(tmp_path / name)

    refused(E.EINVAL, ["Cannot create reference from FASTQ files"], 1000, 5, file=file("reads.fq", b"@r0\nACGTACGTAC\n+\nIIIIIIIIII\n"))
    refused(E.EEMPTY, ["has no valid sequence", "empty.fa"], 1000, 5, file=file("empty.fa", b">a\nACGTACGTACGTACGT\n>b\n" + b"N" * 50 + b"\n"))
    refused(E.EINVAL, ["] density:", "one", "more than once"], 1000, 5, file=file("twice.fa", b">one first\n" + ref[0][1] + b"\n>two\nACGT\n>one again\nACGT\n"))
    lib = E.load_library()
    r = E.DensityResult()
    for a, p, out in ((None, path.encode(), ctypes.byref(r)), (w.arr.h, None, ctypes.byref(r)), (w.arr.h, path.encode(), None)):
        assert lib.skx_array_snp_density(a, p, 1000, 5, 0, out) == E.EINVAL and lib.skx_last_error().startswith(b"density:")
    assert not any((r.samples, r.regions, r.bins, r.chrom_ids, r.chrom_lens, r.snps, r.snp_ref))      # on an error nothing is returned
    _check(w, tmp_path / "r.fa", 30, 2, where="after the refusals")                                  # and the array still answers
    before = w.arr.export()
    a, b = w.arr.snp_density(path, 30, 2, snps=True), w.arr.snp_density(path, 30, 2, snps=True)
    assert all(a[f].tobytes() == b[f].tobytes() for f in FIELDS)
    assert all(np.array_equal(x, y) for x, y in zip(before, w.arr.export()))                         # the array keeps its content
    w.arr.set_total_samples(9)                                          # a rank's share of a collection spread over several devices
    refused(E.EUNSUP, ["] density:", "every sample"], 1000, 5)


def test_a_cell_outside_the_alphabet_and_the_zero_byte(E, tmp_path):
    """Array.from_host takes neither byte, so they are written into the device matrix behind the array's back (the route of test_gpu_curve.py):
    the 0 byte in a site's cell counts as '-'; a byte outside the alphabet there raises the kernel's flag and the call is refused; the same
    byte in a row that is no site, or in the row's padding, is nobody's cell"""
    S = 5
    ref = [("chr1", _random(np.random.default_rng(41), 300))]
    w = World(E, ref, S, 31, seed=42, foreign=40).sprinkle(snp=0.2).build()
    path = tmp_path / "r.fa"
    want = _check(w, path, 20, 2)
    mapped = {l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64.so" in l}
    assert len(mapped) == 1, mapped
    hip = ctypes.CDLL(mapped.pop())
    p, pitch, rows = w.arr.device_matrix()
    U = len(w.var)
    assert rows == U and pitch >= U + 256
    x = np.array([0], np.uint8)

    def poke(sample, row, byte):
        x[0] = byte
        assert hip.hipMemcpy(ctypes.c_void_p(int(p) + sample * pitch + row), ctypes.c_void_p(x.ctypes.data), ctypes.c_size_t(1), 1) == 0      # hipMemcpyHostToDevice

    site_row = int(w.row_of_site[17])
    other_row = int(np.setdiff1d(np.arange(U), w.row_of_site)[-1])
    poke(2, U, ord("X"))                                                # the first byte of sample 2's padding
    poke(3, other_row, ord("X"))                                        # a row no window names
    _same(w.arr.snp_density(str(path), 20, 2, snps=True), want, "padding and a row that is no site")
    poke(2, site_row, 0)
    var0 = w.var.copy()
    var0[site_row, 2] = 0
    _same(w.arr.snp_density(str(path), 20, 2, snps=True), DM.density(w.keys, var0, 31, True, ref, 20, 2), "the 0 byte")
    poke(2, site_row, ord("X"))
    with pytest.raises(E.EngineError) as ei:
        w.arr.snp_density(str(path), 20, 2)
    assert ei.value.code == E.EINVAL and "] density:" in str(ei.value) and "outside" in str(ei.value)
    poke(2, site_row, int(w.var[site_row, 2]))
    poke(3, other_row, int(w.var[other_row, 3]))
    _same(w.arr.snp_density(str(path), 20, 2, snps=True), want, "restored")


# ---- (h) the host's texts on the engine's result, the executable and its Python mirror
def _ska(*args, code=0):
    r = subprocess.run([SKA, *[str(a) for a in args]], capture_output=True, timeout=120)
    assert r.returncode == code, (args, r.returncode, r.stderr.decode()[-2000:])
    return r


@pytest.fixture(scope="module")
def cli(E, tmp_path_factory):
    d = tmp_path_factory.mktemp("density")
    recs = M.records("k9")
    files = []
    for name, rs in zip(M.names_of("k9"), recs):
        p = d / f"{name}.fa"
        p.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(rs)))
        files.append(p)
    _ska("build", "-k", 15, "-o", d / "x", *files)
    cut = recs[2][0]
    ref = [("chrom_a", recs[1][0][:3000]), ("with_n", cut[3000:3400] + b"NN" + cut[3500:3700].lower()), ("nine", cut[:9]), ("island", recs[1][1])]
    keys, var, _ = E.Array.load(str(d / "x.skf")).export()
    return {"dir": d, "skf": d / "x.skf", "names": M.names_of("k9"), "keys": keys, "var": var, "ref": ref, "fa": _write(d / "ref.fa", ref)}


@pytest.mark.parametrize("WT", [(1000, 5), (200, 3), (50, 2)])
def test_cli_files_equal_the_model(cli, WT):
    d, (W, T) = cli["dir"], WT
    out = d / f"w{W}_t{T}"
    snps = W != 1000
    extra = [] if W == 1000 else ["--window", W, "--min-snps", T, "--snps", "--masked-aln", d / f"{out.name}.masked.aln"]
    _ska("density", cli["fa"], cli["skf"], "-o", out, *extra)
    want = DM.texts(cli["keys"], cli["var"], cli["names"], 15, True, cli["ref"], W, T, snps=snps)
    assert sorted(p.name for p in d.iterdir() if p.name.startswith(out.name + ".density")) == sorted(out.name + s for s in want)
    for suffix, text in want.items():
        assert (d / (out.name + suffix)).read_bytes() == text.encode(), (WT, suffix)
    if snps:
        res = DM.density(cli["keys"], cli["var"], 15, True, cli["ref"], W, T)
        masked = DM.masked_alignment(cli["keys"], cli["var"], cli["names"], 15, True, cli["ref"], res)
        assert (d / f"{out.name}.masked.aln").read_bytes() == masked
        assert len(res["regions"]) > 0 and masked != MM.MapModel(cli["keys"], cli["var"], cli["names"], 15, True, cli["ref"]).write_aln(repeat_mask=True)


def test_python_mirror_and_host_texts(E, cli):
    d = cli["dir"]
    E.default_context().density(cli["fa"], cli["skf"], d / "mirror", window=200, min_snps=3, snps=True, masked_aln=d / "mirror.aln")
    want = DM.texts(cli["keys"], cli["var"], cli["names"], 15, True, cli["ref"], 200, 3, snps=True)
    for suffix, text in want.items():
        assert (d / ("mirror" + suffix)).read_bytes() == text.encode(), suffix
    res = DM.density(cli["keys"], cli["var"], 15, True, cli["ref"], 200, 3)
    assert (d / "mirror.aln").read_bytes() == DM.masked_alignment(cli["keys"], cli["var"], cli["names"], 15, True, cli["ref"], res)
    got = E.Array.load(str(cli["skf"])).snp_density(cli["fa"], 200, 3, snps=True)
    assert E.density_text(E.DENSITY_REGIONS, got, cli["names"], 200) == want[".density.regions.tsv"]
    assert E.density_text(E.DENSITY_SNPS, got, cli["names"], 200) == want[".density.snps.tsv"]


def test_cli_refusals(cli):
    d = cli["dir"]
    (d / "twice.fa").write_bytes(b">a x\nACGTTGCATGCAAGTAC\n>b\nACGTTGCATGCATGTAA\n>a y\nACGTTGCATGCATGAAA\n")
    r = _ska("density", d / "twice.fa", cli["skf"], "-o", d / "twice", code=1)
    assert b"chromosome id a occurs more than once" in r.stderr and not (d / "twice.density.regions.tsv").exists()
    (d / "reads.fq").write_bytes(b"@r0\nACGTTGCATGCAAGT\n+\nIIIIIIIIIIIIIII\n")
    r = _ska("density", d / "reads.fq", cli["skf"], "-o", d / "reads", code=1)
    assert b"Cannot create reference from FASTQ files" in r.stderr and not (d / "reads.density.summary.tsv").exists()
