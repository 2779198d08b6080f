"""skx_array_group_markers / skh_markers / `ska markers` (`-m gpu`), through skx_engine.py and the executable, against tests/markers_model.py
(held against a worked example, a second restatement and the oracle by tests/test_markers_model.py on the CPU).  Records and their split
k-mers must be the model's exactly: the model works on the array's export (rows ascending by split k-mer), the device on the array's own row
order, so a record is identified by its split k-mer; the device's own order -- ascending (group, row), every pair once -- is checked besides,
and where the array was made from rows given in ascending order (Array.from_host) the row indices must be the model's too."""
import os
import subprocess

import numpy as np
import pytest

import markers_model as MM
import subset_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PART = [[4, 5, 6, 7], [9, 11, 8, 10], [0, 3, 1, 2], [12]]
PART_TINY = [[0, 3], [1, 2, 4], [5]]
PQ = [(1.0, 0.0), (0.75, 0.0), (0.5, 0.1), (0.0, 0.0)]
FIELDS = ("group", "n_in", "n_out", "kind", "bases_in", "bases_out")


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def _key_order(keys, group):
    return np.lexsort((keys["lo"], keys["hi"], group))


def _check(arr, export, seg, n_groups, reported=None, P=1.0, Q=0.0, kinds=3, rows_too=False, where=None):
    """one call against the model -> the model's per-group counts"""
    ekeys, var = export[0], export[1]
    rec, keys, info = arr.group_markers(seg, n_groups, reported, P, Q, kinds)
    want, counts = MM.markers(var, seg, n_groups, reported, P, Q, kinds)
    where = (where, P, Q, kinds, len(rec), len(want))
    assert len(rec) == len(want) == len(keys), where
    assert [(int(i["presence"]), int(i["allele"])) for i in info] == counts, where
    # the device's order: ascending (group, row), every (group, row) once, rows of the array
    word = (rec["group"].astype(np.int64) << 32) | rec["row"].astype(np.int64)
    assert (np.diff(word) > 0).all() and (rec["row"] < max(len(var), 1)).all() and (rec["reserved"] == 0).all(), where
    o = _key_order(keys, rec["group"])
    for f in FIELDS:
        assert np.array_equal(rec[f][o], want[f]), (where, f)
    assert np.array_equal(keys[o], ekeys[want["row"].astype(np.int64)]), where
    if rows_too:
        assert np.array_equal(rec["row"], want["row"]) and np.array_equal(o, np.arange(len(o))), where
    return counts


# ---- (a) the four cases of subset_model: 13 192 / 8 637 / 14 109 / 154 rows (more than two 4 096-column blocks, no multiple of 16) ----
@pytest.fixture(scope="module", params=["k31", "k9", "k41", "tiny"])
def source(request, E):
    case = request.param
    k, names = M.CASES[case]["k"], M.names_of(case)
    arr = E.DictSet.build([E.record_stream(r) for r in M.records(case)], k, True).merge(names)
    first = arr.group_markers(MM.partition(len(names), PART_TINY if case == "tiny" else PART), 3 if case == "tiny" else 4)      # on the array as the merge left it
    export = arr.export()
    return {"case": case, "arr": arr, "export": export, "S": len(names), "part": PART_TINY if case == "tiny" else PART, "first": first}


def _variant(src, name):
    """-> (segment_of, n_groups, reported)"""
    S, part = src["S"], [list(g) for g in src["part"]]
    if name == "all-listed":
        pass
    elif name == "one-unlisted":                                         # the last sample (12; 5 in the tiny case) is listed by no group
        part = [[s for s in g if s != S - 1] for g in part]
        part = [g for g in part if g]
    elif name == "shuffled":                                             # the file's lines shuffled: the groups in another order, their members too
        rng = np.random.default_rng(5)
        part = [[int(s) for s in rng.permutation(part[g])] for g in rng.permutation(len(part))]
    elif name == "everybody":                                            # one group holding all samples: the other side is empty
        part = [list(range(S))]
    reported = [len(g) >= 2 for g in part] if name == "min-size-2" else None
    return MM.partition(S, part), len(part), reported


@pytest.mark.parametrize("variant", ["all-listed", "one-unlisted", "min-size-2", "shuffled", "everybody"])
def test_cases_equal_the_model(source, variant):
    seg, G, reported = _variant(source, variant)
    total = 0
    for P, Q in PQ:
        counts = _check(source["arr"], source["export"], seg, G, reported, P, Q, where=(source["case"], variant))
        total += sum(p + a for p, a in counts)
    assert total > 0
    if variant == "min-size-2":
        assert reported.count(False) == 1
    if variant == "all-listed":
        rec, keys, info = source["first"]                               # the call on the array as it came equals the one after the export
        again = source["arr"].group_markers(seg, G)
        assert all(np.array_equal(x, y) for x, y in zip(source["first"], again))
        if source["case"] in ("k31", "k9"):                             # the anchors tests/test_markers_model.py holds against the oracle
            want = {"k31": [(531, 12), (569, 18), (613, 15), (685, 19)], "k9": [(145, 19), (95, 7), (124, 14), (83, 11)]}[source["case"]]
            assert [(int(i["presence"]), int(i["allele"])) for i in info] == want
    after = source["arr"].export()
    assert all(np.array_equal(x, y) for x, y in zip(after, source["export"]))      # the array keeps its content


# ---- (b) Array.from_host matrices: 70 samples, 8 245 rows, all 16 codes plus gaps ----
LETTERS = np.frombuffer(MM.IUPAC.encode(), np.uint8)


def _synthetic(S, U, seed, groups):
    """a background letter per row (or none), one group with a letter of its own, in a third of the rows a second such group, gaps and a little
    noise -- and planted rows, so that what the tests must see is there whatever the draw"""
    rng = np.random.default_rng(seed)
    lo = np.unique(rng.integers(1 << 33, 1 << 59, size=U + 64, dtype=np.uint64))[:U]
    assert len(lo) == U
    seg, G = MM.partition(S, groups), len(groups)
    var = np.repeat(LETTERS[rng.integers(0, 16, size=(U, 1))], S, axis=1)
    for share in (1.0, 0.33):
        special, letter = rng.integers(0, G + 1, size=U), LETTERS[rng.integers(0, 16, size=U)]
        hit = (seg[None, :] == special[:, None]) & (rng.random((U, 1)) < share)
        var[hit] = np.broadcast_to(letter[:, None], (U, S))[hit]
    var[rng.random((U, S)) < 0.3] = ord("-")
    noise = rng.random((U, S)) < 0.01
    var[noise] = LETTERS[rng.integers(0, 16, size=int(noise.sum()))]
    last = groups[-1]                                                   # a group with index >= 64 when there are that many
    planted = [("-", "R"),                                              # presence marker with an ambiguous set
               ("C", "W"),                                              # allele marker with an ambiguous set
               ("-", "G"), ("A", "T")]
    for r, (others, mine) in enumerate(planted[:U]):
        var[r] = ord(others)
        var[r, last] = ord(mine)
    if U > len(planted) and G > 1:                                      # a marker of two groups
        var[len(planted)] = ord("-")
        var[len(planted), groups[0]] = ord("A")
        var[len(planted), last] = ord("C")
    return lo, var, seg


def _from_host(E, S, lo, var):
    keys = np.zeros(len(lo), E.KEY_DT)
    keys["lo"] = lo                                                     # ascending: the array's row order is the export's
    arr = E.Array.from_host(31, True, [f"s{i:02d}" for i in range(S)], keys, var)
    return arr, arr.export()


SYNTH = {
    "singletons": [[s] for s in range(70)],
    "pairs": [[2 * g, 2 * g + 1] for g in range(35)],
    # 5 of the 70 samples listed by no group: 65 remain, 32 pairs and a group of one
    "pairs-5-unlisted": (lambda rest: [rest[2 * g:2 * g + 2] for g in range(33)])([s for s in range(70) if s not in (3, 17, 40, 41, 69)]),
}


@pytest.mark.parametrize("layout", sorted(SYNTH))
def test_from_host_matrices(E, layout):
    groups = SYNTH[layout]
    S, U, G = 70, 8245, len(groups)
    lo, var, seg = _synthetic(S, U, 70 + G, groups)
    assert set(np.unique(MM.CODE[var])) == set(range(16))
    want, _ = MM.markers(var, seg, G)
    pop = np.array([bin(x).count("1") for x in range(16)])[want["bases_in"]]
    for kind in (MM.PRESENCE, MM.ALLELE):
        assert ((want["kind"] == kind) & (pop >= 2)).any(), kind
    if layout == "singletons":
        assert (want["group"] >= 64).any()
    assert len(np.unique(want["row"])) < len(want)                      # some row is a marker of several groups
    arr, export = _from_host(E, S, lo, var)
    assert np.array_equal(export[1], var)
    for P, Q in PQ:
        _check(arr, export, seg, G, None, P, Q, rows_too=True, where=layout)
    reported = [g % 3 != 1 for g in range(G)]
    _check(arr, export, seg, G, reported, 0.5, 0.05, rows_too=True, where=(layout, "reported"))


# ---- (c) edges ----
@pytest.mark.parametrize("U", [0, 1, 15, 16, 17])
def test_few_rows(E, U):
    groups = [[0, 1], [2], [4, 3]]                                      # sample 5 unlisted
    lo, var, seg = _synthetic(6, U, U, groups)
    arr, export = _from_host(E, 6, lo, var)
    for P, Q in PQ:
        for kinds in (1, 2, 3):
            _check(arr, export, seg, 3, None, P, Q, kinds, rows_too=True, where=U)


def test_one_sample(E):
    lo, var, seg = _synthetic(1, 4097, 1, [[0]])
    arr, export = _from_host(E, 1, lo, var)
    for P, Q in PQ:
        counts = _check(arr, export, seg, 1, None, P, Q, rows_too=True)
        assert counts == [(int((MM.CODE[var[:, 0]] != 0).sum()), 0)]
    rec, _, _ = arr.group_markers([1], 1, reported=[0])                 # the one sample unlisted, the group not reported: nothing
    assert len(rec) == 0


def test_kinds_one_at_a_time(source):
    seg, G, _ = _variant(source, "all-listed")
    both = _check(source["arr"], source["export"], seg, G, None, 0.5, 0.1, 3)
    assert _check(source["arr"], source["export"], seg, G, None, 0.5, 0.1, 1) == [(p, 0) for p, _ in both]
    assert _check(source["arr"], source["export"], seg, G, None, 0.5, 0.1, 2) == [(0, a) for _, a in both]


def test_refusals(source, E):
    arr, S = source["arr"], source["S"]
    seg, G, _ = _variant(source, "all-listed")
    bad = [dict(min_in=1.5), dict(min_in=-0.1), dict(min_in=float("nan")), dict(max_out=1.01), dict(max_out=-1e-9), dict(max_out=float("nan")), dict(kinds=0), dict(kinds=4)]
    for kw in bad:
        with pytest.raises(E.EngineError) as ei:
            arr.group_markers(seg, G, **kw)
        assert ei.value.code == E.EINVAL and "] markers:" in str(ei.value), (kw, str(ei.value))
    for s, g, rep in ((np.where(np.arange(S) == 0, G + 1, seg), G, None), (np.where(np.arange(S) == 0, -1, seg), G, None), (seg, G + 1, None)):
        with pytest.raises(E.EngineError) as ei:                        # a segment out of range; a reported group without samples
            arr.group_markers(s, g, rep)
        assert ei.value.code == E.EINVAL and "] markers:" in str(ei.value), str(ei.value)
    rec, _, info = arr.group_markers(seg, G + 1, [1] * G + [0])         # an empty group that is not reported is nobody's business
    assert len(rec) == sum(int(i["presence"]) + int(i["allele"]) for i in info) > 0
    sub, _ = arr.subset_filtered(list(range(S)), min_freq=0.0, filter_type=E.FILTER_NONE)      # an array without split k-mers
    with pytest.raises(E.EngineError) as ei:
        sub.group_markers(seg, G)
    assert ei.value.code == E.EINVAL and "] markers:" in str(ei.value)
    assert all(np.array_equal(x, y) for x, y in zip(arr.export(), source["export"]))


# ---- (d) the executable (k = 31: what sequence files are built with) ----
CLI_GROUPS = [("clade", [4, 5, 6, 7]), ("far", [9, 11, 8, 10]), ("near", [0, 3, 1, 2]), ("solo", [12])]


def _ska(*args):
    r = subprocess.run([SKA, *[str(a) for a in args]], capture_output=True, timeout=120)
    assert r.returncode == 0, (args, r.stderr.decode()[-2000:])
    return r


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    d = tmp_path_factory.mktemp("markers")
    files = []
    for name, recs in zip(M.names_of("k31"), M.records("k31")):
        p = d / f"{name}.fa"
        p.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
        files.append(p)
    _ska("build", "-o", d / "x", *files)
    names = M.names_of("k31")
    rows = [(names[i], label) for label, idx in CLI_GROUPS for i in idx]
    rows = rows[::2] + rows[1::2]                                       # the groups' lines interleaved: the labels' first appearance orders the groups
    gf = d / "groups.csv"
    gf.write_text("id,Cluster__autocolour\n" + "".join(f"{n},{l}\n" for n, l in rows))
    groups, seen = [], {}
    for n, l in rows:
        if l not in seen:
            seen[l] = len(groups)
            groups.append((l, []))
        groups[seen[l]][1].append(n)
    return {"dir": d, "skf": d / "x.skf", "groups_file": gf, "groups": groups, "nk": _ska("nk", "--full-info", d / "x.skf").stdout.decode()}


CLI_RUNS = {
    "defaults": ([], dict()),
    "loose": (["--min-in", "0.5", "--max-out", "0.1", "--min-group-size", "2"], dict(P=0.5, Q=0.1, min_group_size=2)),
    "alleles": (["--kind", "allele", "--min-in", "0.75"], dict(P=0.75, kinds=MM.ALLELE)),
}


@pytest.mark.parametrize("run", sorted(CLI_RUNS))
def test_cli_files_equal_the_model(cli, run):
    flags, kw = CLI_RUNS[run]
    d = cli["dir"]
    _ska("markers", cli["skf"], "--groups", cli["groups_file"], "-o", d / run, "--fasta", *flags)
    want = MM.texts(cli["nk"], cli["groups"], fasta=True, **kw)
    assert sorted(p.name for p in d.iterdir() if p.name.startswith(run + ".")) == sorted(run + suffix for suffix in want)
    for suffix, text in want.items():
        assert (d / (run + suffix)).read_text() == text, suffix
    assert want[".markers.tsv"].count("\n") > 1
    if run == "defaults":
        # `ska weed --reverse` with a group's FASTA keeps exactly the group's marker rows (--min-freq 0: the command's own frequency filter,
        # 0.9 by default, would take the rows of a small group away again)
        for label in ("clade", "solo"):
            fa = d / f"{run}.{label}.markers.fa"
            _ska("weed", cli["skf"], fa, "--reverse", "--min-freq", "0", "-o", d / f"w_{label}.skf")
            nk = _ska("nk", d / f"w_{label}.skf").stdout.decode()
            assert f"\nk-mers={fa.read_text().count('>')}\n" in nk, label
