"""skx_array_mask_regions / skh_mask / `ska mask` (`-m gpu`), through skx_engine.py and the executable, against tests/mask_model.py (held against
the oracle's `ska map`, `ska weed` and delete_samples, a hand-worked example and a restatement in plain loops by tests/test_mask_model.py on the
CPU).  Everything is an integer: export() of the masked array must equal the model's keys, variants and counts exactly, and the saved file,
read back, must hold the same rows.  The worlds are test_gpu_density.py's; the item counts are placed around the kernel's chunk as built:
a workgroup of mask_items_kernel takes MASK_CHUNK = 1 024 consecutive (interval, site) items."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import density_model as DM
import mask_model as KM
import ora
import subset_model as M
import test_density_model as TM
import test_mask_model as TK
from test_gpu_density import World, _random, _write

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
ALL = KM.ALL
CHUNK = 1024


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    assert eng.MASK_CHUNK == CHUNK, "the item counts below are placed around it"
    return eng


def _by_key(keys, var, counts):
    order = np.lexsort((keys["lo"], keys["hi"]))
    return keys[order], var[order], np.asarray(counts, np.uint64)[order]


def _holds(E, arr, want, tmp_path, where):
    """the array equals the model's result, as it stands and after a save and a load"""
    gk, gv, gc = arr.export()
    assert np.array_equal(gk, want["keys"]), where
    assert np.array_equal(gv, want["var"]), where
    assert np.array_equal(gc, want["counts"]), where
    assert arr.nrows == len(want["keys"]) == arr.nkmers
    arr.save_skf(str(tmp_path / "masked"))
    back = E.Array.load(str(tmp_path / "masked.skf"))
    assert back.names == arr.names and (back.k, back.rc) == (arr.k, arr.rc)
    for x, y in zip(_by_key(*back.export()), _by_key(gk, gv, gc)):
        assert np.array_equal(x, y), where


def _mask(E, arr, k, rc, ref, path, iv, tmp_path, where=None):
    """mask arr in place and hold everything it returns and leaves against the model on what the array exported before"""
    keys, var, counts = arr.export()
    want = KM.mask(keys, var, counts, k, rc, ref, iv)
    sm, info = arr.mask_regions(path, iv)
    assert sm.dtype == E.MASK_SAMPLE_DT and np.array_equal(sm, want["samples"]), (where, sm, want["samples"])
    assert {f: int(info[f]) for f in KM.INFO_DT.names} == {f: int(want["info"][f]) for f in KM.INFO_DT.names}, where
    _holds(E, arr, want, tmp_path, where)
    return want


def _site_pos(w, i):
    c, (pos, _, _) = w.sites[i]
    return c, pos


# ---- (a) samples, key widths, strands: two chromosomes with an interval on each, sites at a chromosome's first and last window, an interval
# without a site, overlapping input, many samples over the same rows, rows that are no site, a BED interval and a region over the same row
@pytest.mark.parametrize("S,k,rc", [(1, 31, True), (64, 31, False), (65, 31, True), (1, 41, False), (64, 41, True), (65, 41, True)])
def test_samples_widths_and_strands(E, S, k, rc, tmp_path):
    rng = np.random.default_rng(S * 100 + k)
    seg = _random(rng, 70)
    ref = [("one", _random(rng, 400) + seg + b"N" * 60 + _random(rng, 90).lower()), ("none", b"ACGT"), ("two", _random(rng, 200) + seg + _random(rng, 50))]
    w = World(E, ref, S, k, seed=S + k, rc=rc, foreign=29).sprinkle(snp=0.2, gap=0.2, ambig=0.1).build()
    assert w.repeats and len(w.sites) > 500 and (not rc or {x[2] for _, x in w.sites} == {False, True})
    path = _write(tmp_path / "r.fa", ref)
    first_one = min(p for c, (p, _, _) in w.sites if c == 0)
    last_one = max(p for c, (p, _, _) in w.sites if c == 0)
    first_two = min(p for c, (p, _, _) in w.sites if c == 2)
    last_two = max(p for c, (p, _, _) in w.sites if c == 2)
    iv = []
    for s in sorted({0, S // 2, S - 1}):
        iv += [(s, 0, 0, first_one + 3), (s, 0, first_one + 2, first_one + 9), (s, 0, first_one + 10, first_one + 12), (s, 0, 0, first_one + 3),      # overlapping, touching, twice
               (s, 0, last_one - 2, len(ref[0][1]) - 1), (s, 2, first_two, first_two), (s, 2, last_two - 5, last_two),
               (s, 0, 480, 520)]                                        # inside the run of N: no site
    for s in range(S):                                                  # every sample over the same rows: some of them are left without a cell
        iv.append((s, 2, 100, 130))
    iv += [(0, 0, 395, 440), (ALL, 2, 215, 225)]                        # over the stretch both chromosomes share: repeated windows, nobody's site
    iv += [(ALL, 0, 200, 240), (S - 1, 0, 230, 260), (ALL, 2, len(ref[2][1]) - 8, len(ref[2][1]) - 1), (ALL, 1, 0, 3)]      # a row in a BED interval and in a region
    keys0, var0, counts0 = w.arr.export()
    want = _mask(E, w.arr, k, rc, ref, path, iv, tmp_path, (S, k, rc))
    info = want["info"]
    assert int(info["rows_all_samples"]) >= 41 and int(info["rows_emptied"]) >= 10 and int(info["rows_out"]) < int(info["rows_in"])
    assert (want["samples"]["sites_in_regions"] >= want["samples"]["cells_masked"]).all() and want["samples"]["cells_masked"].sum() > 0
    # (with one sample a row that loses its cell is removed: its count is never seen)
    for mutant in ("repeats_masked", "empty_rows_kept") + (("counts_not_lowered", "double_decrement") if S > 1 else ()) + (("row_of_forward_strand",) if rc else ()):
        other = KM.mask(keys0, var0, counts0, k, rc, ref, iv, mutant)                       # the input reaches the edges the mutants stand for
        assert not (np.array_equal(other["keys"], want["keys"]) and np.array_equal(other["var"], want["var"]) and np.array_equal(other["counts"], want["counts"])), mutant
    again, info2 = w.arr.mask_regions(path, iv)                         # a second time: nothing is left to mask
    assert not again["cells_masked"].any() and int(info2["rows_all_samples"]) == 0 and int(info2["rows_emptied"]) == 0
    _holds(E, w.arr, want, tmp_path, "twice")


# ---- (b) the items around the kernel's chunk: chunk - 1, chunk, chunk + 1 over two samples' intervals; one interval longer than two chunks; ALL
# intervals of chunk + 1 sites
@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_item_counts_around_the_chunk(E, n, tmp_path):
    S, U = 3, 2 * CHUNK + 200
    ref = [("chr1", _random(np.random.default_rng(n), 1300)), ("chr2", _random(np.random.default_rng(n + 1), U + 60 - 1300))]
    w = World(E, ref, S, 31, seed=n + 2).sprinkle(snp=0.1, gap=0.3).build()
    assert len(w.sites) == U and not w.repeats
    on_one = [i for i, (c, _) in enumerate(w.sites) if c == 0]
    on_two = [i for i, (c, _) in enumerate(w.sites) if c == 1]
    path = _write(tmp_path / "r.fa", ref)
    if n > 2 * CHUNK:                                                   # one interval longer than a chunk: every site of chr1; the rest on chr2
        assert CHUNK < len(on_one) < n
        iv = [(1, 0, 0, len(ref[0][1]) - 1), (1, 1, 0, _site_pos(w, on_two[n - len(on_one) - 1])[1])]
    else:                                                               # two samples' intervals, the second one's items end the chunk
        iv = [(0, 0, 0, _site_pos(w, on_one[n - 11])[1]), (2, 1, _site_pos(w, on_two[5])[1], _site_pos(w, on_two[14])[1])]
    want = _mask(E, w.arr, 31, True, ref, path, iv, tmp_path, n)
    assert int(want["samples"]["sites_in_regions"].sum()) == n and 0 < int(want["samples"]["cells_masked"].sum()) < n
    if n == CHUNK + 1:                                                  # the ALL launch at the same size, on the array as it was
        w.build()
        want = _mask(E, w.arr, 31, True, ref, path, [(ALL, 0, 0, _site_pos(w, on_one[CHUNK])[1])], tmp_path, "all")
        assert int(want["info"]["rows_all_samples"]) == CHUNK + 1 and w.arr.nrows == U - CHUNK - 1


# ---- (c) a mask that empties every row, one that removes every row, no interval, no site, no rows
def test_every_row_and_no_row(E, tmp_path):
    ref = [("chr1", _random(np.random.default_rng(3), 300)), ("chr2", _random(np.random.default_rng(4), 120))]
    path = _write(tmp_path / "r.fa", ref)
    whole = lambda s: [(s, c, 0, len(seq) - 1) for c, (_, seq) in enumerate(ref)]
    w = World(E, ref, 2, 31, seed=5).sprinkle(gap=0.3).build()
    U = len(w.var)
    want = _mask(E, w.arr, 31, True, ref, path, whole(0) + whole(1), tmp_path, "emptied")
    present_rows = int(((w.var != KM.GAP).any(1)).sum())
    assert int(want["info"]["rows_emptied"]) == present_rows and w.arr.nrows == U - present_rows
    w = World(E, ref, 3, 31, seed=6).sprinkle(snp=0.2).build()
    want = _mask(E, w.arr, 31, True, ref, path, whole(ALL), tmp_path, "all rows")
    assert int(want["info"]["rows_out"]) == 0 and w.arr.nrows == 0
    sm, info = w.arr.mask_regions(path, whole(ALL) + whole(1))          # the array without rows is taken again
    assert int(info["sites"]) == 0 and int(info["rows_in"]) == 0 and not sm["sites_in_regions"].any()
    w = World(E, ref, 3, 31, seed=7).sprinkle(snp=0.2).build()
    before = w.arr.export()
    sm, info = w.arr.mask_regions(path, [])                             # n == 0
    assert int(info["sites"]) == len(w.sites) and int(info["rows_out"]) == int(info["rows_in"]) == len(w.var) and int(info["n_intervals_merged"]) == 0
    assert all(np.array_equal(x, y) for x, y in zip(before, w.arr.export()))
    assert w.arr.mask_regions(path, [(1, 0, 5, 9)], want_samples=False)[0] is None          # samples == NULL; no site before position 15
    assert all(np.array_equal(x, y) for x, y in zip(before, w.arr.export()))
    elsewhere = World(E, ref, 3, 31, seed=8, n_sites=0, foreign=200).build()                # rows, none of them a window's
    want = _mask(E, elsewhere.arr, 31, True, ref, path, whole(ALL) + whole(0), tmp_path, "no site")
    assert int(want["info"]["sites"]) == 0 and int(want["info"]["rows_out"]) == 200


# ---- (d) the hand-worked example of tests/test_mask_model.py on the device
def test_hand_worked_example_on_the_device(E, tmp_path):
    keys, var = TM._hand_array()
    arr = E.Array.from_host(9, True, TM.HAND_NAMES, keys, var)
    path = _write(tmp_path / "r.fa", TM.HAND_REF)
    want = _mask(E, arr, 9, True, TM.HAND_REF, path, TK.HAND_INTERVALS, tmp_path, "hand")
    assert [tuple(int(x) for x in q) for q in want["samples"]] == TK.HAND_SAMPLES and {f: int(want["info"][f]) for f in KM.INFO_DT.names} == TK.HAND_INFO


# ---- (e) the array as built (held as the merge left it), as loaded and after skx_array_delete_samples; both key widths; a stored count that
# is not the number of present cells
@pytest.mark.parametrize("case", ["k31", "k41"])
def test_provenance(E, case, tmp_path):
    k, names, recs = M.CASES[case]["k"], M.names_of(case), M.records(case)
    ref = [("genome", recs[1][0]), ("island", recs[1][1])]
    path = _write(tmp_path / "r.fa", ref)
    streams = [E.record_stream(r) for r in recs]
    S = len(names)
    n0 = len(ref[0][1])
    iv = [(s, 0, 100 + 37 * s, 600 + 41 * s) for s in range(S)] + [(0, 0, n0 - 400, n0 - 1), (S - 1, 1, 0, len(ref[1][1]) - 1), (ALL, 0, 1000, 1100), (ALL, 1, 10, 30)]
    built = E.DictSet.build(streams, k, True).merge(names)
    want = _mask(E, built, k, True, ref, path, iv, tmp_path, (case, "as built"))
    assert want["samples"]["cells_masked"].sum() > 0 and int(want["info"]["rows_all_samples"]) > 0
    E.DictSet.build(streams, k, True).merge(names).save_skf(str(tmp_path / "whole"))
    loaded = E.Array.load(str(tmp_path / "whole.skf"))
    _mask(E, loaded, k, True, ref, path, iv, tmp_path, (case, "as loaded"))
    cut = E.Array.load(str(tmp_path / "whole.skf"))
    cut.delete_samples([names[1], names[3]])
    iv_cut = [q for q in iv if q[0] == ALL or q[0] < S - 2]
    _mask(E, cut, k, True, ref, path, iv_cut, tmp_path, (case, "after delete_samples"))
    keys, var, counts = E.Array.load(str(tmp_path / "whole.skf")).export()
    counts = counts.copy()
    counts[::5] = 1                                                     # as update_counts(true) may leave them: fewer than the present cells
    odd = E.Array.from_host(k, True, names, keys, var, counts)
    want = _mask(E, odd, k, True, ref, path, iv, tmp_path, (case, "stored counts"))
    assert (want["counts"] == 0).any()


# ---- (f) every refusal leaves the array as it was
def test_refusals_leave_the_array_unchanged(E, tmp_path):
    ref = [("chr1", _random(np.random.default_rng(31), 400)), ("chr2", _random(np.random.default_rng(32), 100))]
    w = World(E, ref, 4, 31, seed=33).sprinkle(snp=0.2).build()
    path = _write(tmp_path / "r.fa", ref)
    before = w.arr.export()
    good = [(0, 0, 20, 60)]

    def refused(code, words, iv, file=None):
        with pytest.raises(E.EngineError) as ei:
            w.arr.mask_regions(file or path, iv)
        assert ei.value.code == code and all(x in str(ei.value) for x in words), str(ei.value)
        assert all(np.array_equal(x, y) for x, y in zip(before, w.arr.export())), words

    refused(E.EINVAL, ["] mask:", "starts at 30"], good + [(1, 0, 30, 29)])
    refused(E.EINVAL, ["] mask:", "past chromosome chr1"], good + [(1, 0, 30, 400)])
    refused(E.EINVAL, ["] mask:", "past chromosome chr2"], good + [(ALL, 1, 0, 100)])
    refused(E.EINVAL, ["] mask:", "names sample 4"], good + [(4, 0, 1, 2)])
    refused(E.EINVAL, ["] mask:", "names chromosome 2"], good + [(1, 2, 1, 2)])

    def file(name, text):
        (tmp_path / name).write_bytes(text)
        return str(tmp_path / name)

    refused(E.EINVAL, ["] mask:", "one", "more than once"], good, file=file("twice.fa", b">one first\n" + ref[0][1] + b"\n>two\nACGT\n>one again\nACGT\n"))
    refused(E.EINVAL, ["Cannot create reference from FASTQ files"], good, file=file("reads.fq", b"@r0\nACGTACGTAC\n+\nIIIIIIIIII\n"))
    refused(E.EEMPTY, ["has no valid sequence"], [], file=file("empty.fa", b">a\nACGTACGTACGTACGT\n>b\n" + b"N" * 50 + b"\n"))
    lib = E.load_library()
    iv = np.array(good, E.MASK_INTERVAL_DT)
    info = np.zeros(1, E.MASK_INFO_DT)
    p_iv, p_info = iv.ctypes.data_as(ctypes.c_void_p), info.ctypes.data_as(ctypes.c_void_p)
    for a, p, q, n, i in ((None, path.encode(), p_iv, 1, p_info), (w.arr.h, None, p_iv, 1, p_info), (w.arr.h, path.encode(), None, 1, p_info), (w.arr.h, path.encode(), p_iv, 1, None)):
        assert lib.skx_array_mask_regions(a, p, q, n, None, i) == E.EINVAL and lib.skx_last_error().startswith(b"mask:")
    assert all(np.array_equal(x, y) for x, y in zip(before, w.arr.export()))
    w.arr.set_total_samples(9)                                          # a rank's share of a collection spread over several devices
    refused(E.EUNSUP, ["] mask:", "every sample"], good)
    w.arr.set_total_samples(4)
    want = _mask(E, w.arr, 31, True, ref, path, good, tmp_path, "after the refusals")      # and the array is still taken
    assert int(want["samples"]["cells_masked"][0]) > 0
    g = World(E, ref, 4, 31, seed=34).sprinkle(snp=0.3).build().arr
    if g.apply_filters(0.0, filter_type=E.FILTER_NO_CONST) > 0 and g.nkmers != g.nrows:     # filtered for output only: keys and rows out of step
        with pytest.raises(E.EngineError, match="out of step"):
            g.mask_regions(path, good)


# ---- (g) through the executable
def _ska(*args, code=0):
    r = subprocess.run([SKA, *[str(a) for a in args]], capture_output=True, timeout=120)
    assert r.returncode == code, (args, r.returncode, r.stderr.decode()[-2000:])
    return r


@pytest.fixture(scope="module")
def cli(E, tmp_path_factory):
    d = tmp_path_factory.mktemp("mask")
    recs = M.records("k9")
    files = []
    for name, rs in zip(M.names_of("k9"), recs):
        p = d / f"{name}.fa"
        p.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(rs)))
        files.append(p)
    _ska("build", "-k", 15, "-o", d / "x", *files)
    cut = recs[2][0]
    ref = [("chrom_a", recs[1][0][:3000]), ("with_n", cut[3000:3400] + b"NN" + cut[3500:3700].lower()), ("nine", cut[:9]), ("island", recs[1][1])]
    keys, var, counts = E.Array.load(str(d / "x.skf")).export()
    return {"dir": d, "skf": d / "x.skf", "names": M.names_of("k9"), "keys": keys, "var": var, "counts": counts, "ref": ref, "fa": _write(d / "ref.fa", ref)}


def _file_holds(E, path, want, names):
    back = E.Array.load(str(path))
    assert back.names == list(names)
    for x, y in zip(_by_key(*back.export()), _by_key(want["keys"], want["var"], want["counts"])):
        assert np.array_equal(x, y), path


W_T = (200, 3)


def test_cli_dense_equals_density_then_regions(E, cli):
    d, (W, T) = cli["dir"], W_T
    _ska("mask", cli["fa"], cli["skf"], "-o", d / "dense.skf", "--dense", "--window", W, "--min-snps", T, "--summary", d / "dense")
    _ska("density", cli["fa"], cli["skf"], "-o", d / "den", "--window", W, "--min-snps", T)
    _ska("mask", cli["fa"], cli["skf"], "-o", d / "two_steps", "--regions", d / "den.density.regions.tsv", "--summary", d / "two_steps")
    assert (d / "dense.skf").read_bytes() == (d / "two_steps.skf").read_bytes()
    assert (d / "dense.mask.summary.tsv").read_bytes() == (d / "two_steps.mask.summary.tsv").read_bytes()
    res = DM.density(cli["keys"], cli["var"], 15, True, cli["ref"], W, T)
    iv = [(int(g["sample"]), int(g["chrom"]), int(g["start"]), int(g["end"])) for g in res["regions"]]
    assert len(iv) > 0
    want = KM.mask(cli["keys"], cli["var"], cli["counts"], 15, True, cli["ref"], iv)
    assert want["samples"]["cells_masked"].sum() > 0
    _file_holds(E, d / "dense.skf", want, cli["names"])
    assert (d / "dense.mask.summary.tsv").read_bytes() == KM.summary_text(want, cli["names"], iv).encode()
    # `ska density` of the masked file at the same W and T: no SNP inside a masked interval
    _ska("density", cli["fa"], d / "dense.skf", "-o", d / "after", "--window", W, "--min-snps", T, "--snps")
    ids = [i for i, _ in cli["ref"]]
    merged = KM.merge_intervals(iv)
    lines = (d / "after.density.snps.tsv").read_text().splitlines()[1:]
    assert lines
    for line in lines:
        name, chrom, pos = line.split("\t")[:3]
        s, c, x = cli["names"].index(name), ids.index(chrom), int(pos) - 1
        assert not any(q == s and c2 == c and a <= x <= b for q, c2, a, b in merged), line
    # the oracle's `ska distance` and `ska align` on the model's array
    o = ora.Array.load(str(d / "dense.skf"))                           # (the model's rows, held above, as the oracle's own reader takes the file)
    ok_, ov, oc = o.export()
    for x, y in zip(_by_key(ok_, ov, oc), _by_key(want["keys"], want["var"], want["counts"])):
        assert np.array_equal(x, y)
    assert _ska("distance", d / "dense.skf").stdout == o.distance_tsv()
    assert _ska("align", d / "dense.skf").stdout == o.align()
    assert _ska("align", cli["skf"]).stdout != o.align()


def test_cli_bed_and_regions_together(E, cli):
    d = cli["dir"]
    (d / "phage.bed").write_bytes(b"#track\nchrom_a\t500\t900\tphage\r\nisland\t0\t40\n\nchrom_a\t880\t1000\n")
    (d / "own.tsv").write_bytes(b"sample\tchromosome\tstart\tend\n" + f"{cli['names'][0]}\tchrom_a\t850\t1200\n{cli['names'][2]}\twith_n\t1\t602\tfrom another tool\n".encode())
    _ska("mask", cli["fa"], cli["skf"], "-o", d / "both", "--regions", d / "own.tsv", "--bed", d / "phage.bed", "--summary", d / "both")
    iv = [(0, 0, 849, 1199), (2, 1, 0, 601), (ALL, 0, 500, 899), (ALL, 3, 0, 39), (ALL, 0, 880, 999)]
    want = KM.mask(cli["keys"], cli["var"], cli["counts"], 15, True, cli["ref"], iv)
    assert int(want["info"]["rows_all_samples"]) > 300 and want["samples"]["cells_masked"][0] > 0 and want["samples"]["cells_masked"][2] > 0
    _file_holds(E, d / "both.skf", want, cli["names"])
    assert (d / "both.mask.summary.tsv").read_bytes() == KM.summary_text(want, cli["names"], iv).encode()
    E.default_context().mask(cli["fa"], cli["skf"], d / "mirror", regions=d / "own.tsv", bed=d / "phage.bed", summary=d / "mirror")      # the Python mirror
    assert (d / "mirror.skf").read_bytes() == (d / "both.skf").read_bytes() and (d / "mirror.mask.summary.tsv").read_bytes() == (d / "both.mask.summary.tsv").read_bytes()
    sm, info = E.Array.load(str(cli["skf"])).mask_regions(cli["fa"], iv)
    assert E.mask_text(sm, info, iv, cli["names"]) == KM.summary_text(want, cli["names"], iv)


def test_cli_refusals(cli):
    d = cli["dir"]
    size = cli["skf"].stat().st_size
    r = _ska("mask", cli["fa"], cli["skf"], "-o", cli["skf"], "--dense", code=1)
    assert b"never overwritten" in r.stderr and cli["skf"].stat().st_size == size
    r = _ska("mask", cli["fa"], cli["skf"], "-o", d / "x", "--dense", code=1)                # ".skf" is appended: the input again
    assert b"never overwritten" in r.stderr and cli["skf"].stat().st_size == size
    (d / "bad.tsv").write_bytes(b"sample\tchromosome\tstart\tend\n\nnobody\tchrom_a\t1\t2\n")
    r = _ska("mask", cli["fa"], cli["skf"], "-o", d / "bad", "--regions", d / "bad.tsv", code=1)
    assert b"mask: regions line 3: unknown sample nobody" in r.stderr and not (d / "bad.skf").exists()
    (d / "bad.bed").write_bytes(b"chrom_a\t0\t10\nnine\t0\t10\n")
    r = _ska("mask", cli["fa"], cli["skf"], "-o", d / "bad", "--bed", d / "bad.bed", code=1)
    assert b"mask: bed line 2: end past chromosome nine" in r.stderr and not (d / "bad.skf").exists()
    r = _ska("mask", cli["fa"], cli["skf"], "-o", d / "bad", "--bed", d / "missing.bed", code=1)
    assert b"cannot open" in r.stderr and not (d / "bad.skf").exists()
