"""`ska merge` / `ska delete` / `ska weed` on the device at their row-set and key-width edges (`-m gpu`): skx_array_merge,
skx_array_delete_samples, skx_array_weed, skx_keyset_from_fasta and skh_weed against tests/setops_model.py (pinned to the oracle and to
the reference's goldens by tests/test_setops_model.py) on the cases of its list -- 2, 3 and 6 inputs, disjoint / equal / nested / chained
/ empty row sets, 0 ... 70 001 rows around the 256-row granule, 1 ... 130 samples, k = 5 ... 63 on both strand settings, every cell code,
stored counts that differ from the rows -- for every way an input can have come to be: just built, assembled lazily, handed over by the
caller, loaded from an engine-written or an oracle-written file, and mixtures of these inside one merge (128-bit keys on the host beside
packed words on the device).  After every operation the array must still save, load, align and take a further operation."""
import functools
import os
import subprocess

import numpy as np
import pytest

import ora
import setops_model as M
import subset_model as SM

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SKA = os.path.join(os.path.dirname(HERE), "ska.rust_amd", "ska")
SEQ = [n for n in M.CASES if n.startswith("seq-")]
MATRIX = [n for n in M.CASES if not n.startswith("seq-")]
PROVENANCES = [(n, p) for n in MATRIX for p in ("from_host", "loaded", "oracle_file", "mixed")] + \
              [(n, p) for n in SEQ for p in ("built", "lazy", "from_host", "loaded", "oracle_file", "mixed")]
MIX = {True: ("loaded", "built", "lazy", "from_host"), False: ("loaded", "from_host", "oracle_file")}       # by "is a sequence case"


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


@pytest.fixture(scope="module")
def world(E, tmp_path_factory):
    d = tmp_path_factory.mktemp("setops")
    n_files = [0]

    def path(tag="a", ext=".skf"):
        n_files[0] += 1
        return str(d / f"{tag}{n_files[0]}{ext}")

    def o_arr(a):
        return ora.Array.from_rows(a.k, a.rc, a.names, M.key_dt(a.keys), a.var, a.counts.astype(np.uint64))

    def g_input(case, j, prov):
        a = case["inputs"][j]
        if prov in ("built", "lazy"):
            ds = E.DictSet.build([E.record_stream(r) for r in case["records"][j]], a.k, a.rc)
            return ds.merge(a.names) if prov == "built" else ds.assemble_lazy(ds.union_keys(), a.names)
        if prov == "oracle_file":
            p = path("o")
            o_arr(a).save(p)
            return E.Array.load(p)
        g = E.Array.from_host(a.k, a.rc, a.names, M.key_dt(a.keys), a.var, a.counts.astype(np.uint64))
        if prov == "loaded":
            p = path("g")
            g.save(p)
            return E.Array.load(p)
        return g

    def g_one(name, j, prov):
        case = M.make_case(name)
        mix = MIX[case["records"] is not None]
        return g_input(case, j, mix[j % len(mix)] if prov == "mixed" else prov)

    def g_inputs(name, prov):
        return [g_one(name, j, prov) for j in range(len(M.make_case(name)["inputs"]))]

    def g_subject(name, prov):
        ins = g_inputs(name, prov)
        return E.Array.merge(ins) if len(ins) > 1 else ins[0]

    @functools.lru_cache(maxsize=None)
    def weed_files(name):
        """label -> (FASTA path, engine key set): made once per case"""
        e = M.expected(name)
        out = {}
        for lab, (recs, keys) in e["sets"].items():
            p = M.write_fasta(recs, path(lab, ".fa"))
            ks = E.KeySet.from_fasta(p, e["case"]["k"], e["case"]["rc"])
            assert len(ks) == len(keys), (name, lab)                          # skx_keyset_from_fasta = RefSka::new + kmer_iter
            out[lab] = (p, ks)
        return out

    ns = type("World", (), {})()
    ns.path, ns.o_arr, ns.g_inputs, ns.g_subject, ns.weed_files, ns.g_input, ns.g_one = path, o_arr, g_inputs, g_subject, weed_files, g_input, g_one
    return ns


def g_arr(g):
    """an engine array as the model's tuple: cells and counts as exported, nothing normalised"""
    keys, var, counts = g.export()
    return M.Arr(g.k, g.rc, g.names, M.ints(keys), var, counts.astype(np.int64))


def m_arr(o):
    keys, var, counts = o.export()
    return M.Arr(o.k, o.rc, o.names, M.ints(keys), var, counts.astype(np.int64))


def holds(world, g, want, what, usable=True):
    """the engine array equals the model's and is still an array: it saves to a file the oracle reads back to the same rows, and aligns"""
    diff = M.same(g_arr(g), want)
    assert diff is None, (what, diff)
    assert g.nkmers == g.nrows == len(want.keys), what
    assert g.sample_kmers().tolist() == (want.var != M.GAP).sum(axis=0).tolist(), what
    if not usable:
        return
    p = world.path("u")
    g.save(p)
    back = ora.Array.load(p)
    diff = M.same(m_arr(back), want)
    assert diff is None, (what, "saved file", diff)
    got, ref = g.align(filter_type=0, min_freq=0.0), world.o_arr(want).align(filter_type=ora.FILTER_NONE, min_freq=0.0)
    assert got.split(b"\n")[0::2] == ref.split(b"\n")[0::2], (what, "alignment names")
    assert SM.fasta_columns(got) == SM.fasta_columns(ref), (what, "alignment columns")       # (rows in the engine's order: columns compared as a set)
    assert g.nkmers == g.nrows == len(want.keys), (what, "after align")


@pytest.mark.parametrize("name,prov", PROVENANCES)
def test_merge_delete_weed_vs_model(world, name, prov):
    e = M.expected(name)
    case, merged = e["case"], e["merged"]
    usable = name not in M.LARGE or prov == "mixed"                           # the 70 001-row files once
    holds(world, world.g_subject(name, prov), merged, "merge", usable)
    for lab, (req, want) in e["deletions"].items():
        g = world.g_subject(name, prov)
        g.delete_samples(req)
        holds(world, g, want, ("delete", lab), usable)
    files = world.weed_files(name)
    for i, (lab, reverse, opts) in enumerate(e["plan"]):
        keys = e["sets"][lab][1] if lab else None
        g = world.g_subject(name, prov)
        if lab and i % 2:                                                     # through the file, as `ska weed` goes (skh_weed)
            g.weed(files[lab][0], reverse, **opts.kw())
        else:
            if lab:
                want_keys, want_removed = M.weed_keys(merged, keys, reverse)
                assert g.weed_keys(files[lab][1], reverse) == want_removed, (lab, reverse)
                holds(world, g, want_keys, ("weed_keys", lab, reverse), False)
            g.weed(None, False, **opts.kw())
        holds(world, g, M.run_weed(merged, keys, reverse, opts), ("weed", lab, reverse, opts.ident()), usable)


@pytest.mark.parametrize("name,prov", [(n, p) for n, p in PROVENANCES if n not in M.LARGE])
def test_operations_on_an_input_itself(world, name, prov):
    """delete and weed on every input as it came (file order; 128-bit keys still on the host for from_host / loaded inputs), not on a
    merge's result, whose keys are always packed words on the device"""
    e = M.expected(name)
    sets = e["sets"]
    files = world.weed_files(name)
    for j, a in enumerate(e["case"]["inputs"]):
        mine = M.by_key(a)
        if len(a.names) >= 2:
            g = world.g_one(name, j, prov)
            g.delete_samples([a.names[-1]])
            holds(world, g, M.delete_samples(mine, [a.names[-1]]), ("delete", j))
        for lab, reverse in (("subset", False), ("subset", True), ("every-row", False)):
            if lab not in sets:
                continue
            g = world.g_one(name, j, prov)
            want, removed = M.weed_keys(mine, sets[lab][1], reverse)
            assert g.weed_keys(files[lab][1], reverse) == removed, (j, lab, reverse)
            holds(world, g, want, ("weed_keys", j, lab, reverse))
            g.weed(None, False, **M.DEFAULTS.kw())                            # stored counts decide (floor(S * 0.9) of them)
            holds(world, g, M.run_weed(want, None, False, M.DEFAULTS), ("weed defaults", j, lab, reverse), False)


CHAINS = [(n, p) for n, p in PROVENANCES if n not in M.LARGE and len(M.make_case(n)["inputs"]) > 1 and len(M.expected(n)["merged"].keys)
          and len(set(M.expected(n)["merged"].names)) == len(M.expected(n)["merged"].names) and p in ("mixed", "loaded", "built")]


@pytest.mark.parametrize("name,prov", CHAINS)
def test_chain_merge_delete_weed_merge_again(E, world, name, prov):
    """merge -> delete a whole input's samples -> weed a subset -> merge again with what was deleted (+ an untouched input) == the model's chain"""
    e = M.expected(name)
    case, merged = e["case"], e["merged"]
    gone = list(case["inputs"][0].names)
    rest = [n for n in merged.names if n not in gone]
    keys = e["sets"]["subset"][1]
    want = M.delete_samples(merged, gone)
    want, _ = M.weed_keys(want, keys, False)
    deleted = M.delete_samples(merged, rest)
    want = M.merge([want, deleted, case["inputs"][-1]])
    g = world.g_subject(name, prov)
    g.delete_samples(gone)
    g.weed_keys(world.weed_files(name)["subset"][1], False)
    gd = world.g_subject(name, prov)
    gd.delete_samples(rest)
    holds(world, gd, deleted, "the deleted part")
    again = E.Array.merge([g, gd, world.g_one(name, len(case["inputs"]) - 1, prov)])
    holds(world, again, want, "merged again")
    again.delete_samples(gone)                                                # and once more on that: back to the rest (+ the last input)
    holds(world, again, M.delete_samples(want, gone), "deleted again")


@pytest.mark.parametrize("name", ["k31-nested-257-255", "k33-norc-chain", "k63-identical", "seq-k41-norc", "k31-both-empty", "k33-both-empty"])
def test_empty_results_are_inputs(E, world, name):
    """a weed that keeps nothing, a reverse weed with a foreign set and a merge of two empty arrays succeed with 0 rows; the result saves,
    loads, merges with a non-empty array and aligns like the oracle's.  The reference refuses nowhere along this chain: weed pushes no row
    into an Array2 of shape (0, S) (merge_ska_array.rs:452-487), save / load serialise it as it is (:191-204), to_dict + extend + new take a
    dictionary without split k-mers (:209-221, merge_ska_dict.rs:160-193) and write_fasta writes S empty sequences (:499-517)."""
    e = M.expected(name)
    case, merged = e["case"], e["merged"]
    files = world.weed_files(name)
    prov = "mixed"
    runs = [("no-row", True)] + ([("every-row", False)] if "every-row" in files else [])
    for lab, reverse in runs:
        g = world.g_subject(name, prov)
        removed = g.weed_keys(files[lab][1], reverse)
        assert removed == len(merged.keys) and g.nrows == g.nkmers == 0
        want = M.weed_keys(merged, e["sets"][lab][1], reverse)[0]
        holds(world, g, want, ("emptied", lab, reverse))
        p = world.path("empty")
        g.save(p)
        for empty in (g, E.Array.load(p)):                                   # as it stands and from its file
            assert empty.nrows == 0 and empty.names == merged.names
            other = world.g_one(name, 0, prov)
            for order in (0, 1):
                pair, mpair = [empty, other], [want, case["inputs"][0]]
                gm = E.Array.merge(pair[::-1] if order else pair)
                wm = M.merge(mpair[::-1] if order else mpair)
                holds(world, gm, wm, ("empty merged with input 0", lab, order))
                om = ora.Array.merge([world.o_arr(x) for x in (mpair[::-1] if order else mpair)])
                assert M.same(m_arr(om), wm) is None
            both = E.Array.merge([empty, empty])
            holds(world, both, M.merge([want, want]), "two empty arrays")
            assert both.align(filter_type=0, min_freq=0.0) == ora.Array.merge([world.o_arr(want), world.o_arr(want)]).align(filter_type=ora.FILTER_NONE, min_freq=0.0)
            empty.weed(None, False, **M.DEFAULTS.kw())                        # the filter on nothing
            assert empty.nrows == 0
            if len(want.names) > 1:
                empty.delete_samples([want.names[0]])
                holds(world, empty, M.delete_samples(want, [want.names[0]]), "delete on an empty array")


def test_refusals_leave_the_array_usable(E, world):
    name = "k31-nested-257-255"
    e = M.expected(name)
    a, b = world.g_inputs(name, "loaded")
    k15 = world.g_input(M.make_case("k15-64-65-1"), 2, "from_host")
    first = M.make_case(name)["inputs"][0]
    norc = E.Array.from_host(31, False, ["z"], M.key_dt(first.keys[:3]), first.var[:3, :1])
    with pytest.raises(E.EngineError, match="K-mer lengths do not match: 15 31"):
        E.Array.merge([a, b, k15])
    with pytest.raises(E.EngineError, match="Strand use inconsistent"):
        E.Array.merge([a, b, norc])
    for x, want in ((a, M.by_key(first)), (b, M.by_key(M.make_case(name)["inputs"][1]))):
        holds(world, x, want, "after a refused merge")
    holds(world, E.Array.merge([a, b]), e["merged"], "merge after a refused merge")
    # a key set of another k or strand
    files = world.weed_files(name)
    ks15 = world.weed_files("k15-64-65-1")["subset"][1]
    ks_norc = E.KeySet.from_fasta(files["subset"][0], 31, False)
    g = E.Array.merge([a, b])
    with pytest.raises(E.EngineError, match="K-mer lengths do not match"):
        g.weed_keys(ks15)
    with pytest.raises(E.EngineError, match="Strand use inconsistent"):
        g.weed_keys(ks_norc)
    # delete_samples' own refusals (merge_ska_array.rs:232-234,252-254); ["x", "x"] on two samples is two names, on three it is one
    two = E.Array.from_host(31, True, ["x", "y"], M.key_dt(first.keys), first.var[:, :2])
    for req, text in (([], "Invalid number"), (["x", "y"], "Invalid number"), (["x", "x"], "Invalid number"), (["nobody"], "Could not find sample")):
        with pytest.raises(E.EngineError, match=text):
            two.delete_samples(req)
    m_two = M.arr(31, True, ["x", "y"], first.keys, first.var[:, :2])
    holds(world, two, M.by_key(m_two), "after refused deletes")
    three = E.Array.from_host(31, True, ["x", "y", "x"], M.key_dt(first.keys), first.var[:, :3])
    three.delete_samples(["x", "x"])
    holds(world, three, M.delete_samples(M.arr(31, True, ["x", "y", "x"], first.keys, first.var[:, :3]), ["x", "x"]), "a repeated name")
    assert three.names == ["y", "x"]
    holds(world, g, e["merged"], "after refused weeds")
    # filtered for output only (update_kmers = false): split k-mers and rows are out of step, every set operation refuses, and the array
    # still writes the alignment it was filtered for
    removed = g.apply_filters(0.0, filter_type=E.FILTER_NO_CONST)
    assert removed > 0 and g.nkmers == len(e["merged"].keys) != g.nrows
    aln = g.fasta()
    for call in (lambda: E.Array.merge([a, g]), lambda: g.delete_samples([e["merged"].names[0]]), lambda: g.weed_keys(files["subset"][1])):
        with pytest.raises(E.EngineError, match="out of step"):
            call()
    assert g.fasta() == aln and g.nkmers == len(e["merged"].keys) and g.names == e["merged"].names


# ------------------------------------------------------------------------------------------------------------------ command line
def ska(*args, env=None, cwd=None):
    return subprocess.run([SKA, *args], capture_output=True, text=True, timeout=120, cwd=cwd, env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def k9(E, world, tmp_path_factory):
    """six k = 9 files: two written by the engine, two by the oracle, the reference's two k = 9 fixtures saved again (one by each)"""
    import golden_cases as G
    d = tmp_path_factory.mktemp("cli")
    case = M.matrix_case("cli-k9", 9, True, (2, 1, 3, 1), ((0, 300), (200, 257), (250, 600), (0, 0)), 4242)
    files, arrays = [], []
    for j, a in enumerate(case["inputs"]):
        p = str(d / f"in{j}.skf")
        if j < 2:
            E.Array.from_host(a.k, a.rc, a.names, M.key_dt(a.keys), a.var, a.counts.astype(np.uint64)).save(p)
        else:
            world.o_arr(a).save(p)
        files.append(p)
        arrays.append(a)
    for f, by_engine in (("merge_k9.skf", True), ("multidist.skf", False)):
        p = str(d / ("again_" + f))
        (E.Array.load(G.fin(f)) if by_engine else ora.Array.load(G.fin(f))).save(p)
        files.append(p)
        arrays.append(m_arr(ora.Array.load(G.fin(f))))
    return d, files, arrays


def test_cli_merge_of_six_files(k9):
    d, files, arrays = k9
    order = [files[i] for i in (4, 0, 2, 5, 1, 3)]
    want = M.merge([arrays[i] for i in (4, 0, 2, 5, 1, 3)])
    r = ska("merge", "-o", "six", *order, cwd=d)
    assert r.returncode == 0, r.stderr
    r2 = ska("merge", "-o", "six_serial", *order, cwd=d, env={"SKX_KNOBS": "serial_loads"})
    assert r2.returncode == 0, r2.stderr
    with open(d / "six.skf", "rb") as f1, open(d / "six_serial.skf", "rb") as f2:
        assert f1.read() == f2.read()
    back = ora.Array.load(str(d / "six.skf"))
    assert M.same(m_arr(back), want) is None
    om = ora.Array.merge([ora.Array.load(p) for p in order])
    assert M.same(m_arr(om), want) is None
    nk = ska("nk", "--full-info", "six.skf", cwd=d)
    assert nk.returncode == 0, nk.stderr
    # the header as the oracle prints the file's; the rows as a set (`ska nk` lists them by key, the file holds them in the engine's order)
    assert nk.stdout.split("\n\n")[0] == back.nk(True).decode().split("\n\n")[0]
    assert sorted(nk.stdout.split("\n")) == sorted(back.nk(True).decode().split("\n"))
    assert sorted(M.nk_lines(nk.stdout).split("\n")) == sorted(M.nk_lines(om.nk(True)).split("\n")) == sorted(M.nk(want, True).split("\n"))


def test_cli_merge_refuses_a_later_file_of_another_k(k9, world):
    """a later file whose k needs the other key width does not load as the first file's integer type: the reference's expect() line
    (generic_modes.rs:99-100); one of another k of the same width loads and is refused by extend (merge_ska_dict.rs:161-163)"""
    d, files, _ = k9
    for name, j, text in (("k41-six-inputs", 2, "Failed to load input file"), ("k15-chain-256-1-300", 1, "K-mer lengths do not match: 15 9")):
        p = str(d / f"{name}.skf")
        world.o_arr(M.make_case(name)["inputs"][j]).save(p)
        r = ska("merge", "-o", "bad", files[0], files[2], p, files[1], cwd=d)
        assert r.returncode != 0 and text in r.stderr, (name, r.stderr)
        assert not os.path.exists(d / "bad.skf")


def test_cli_delete_with_a_list_file(k9):
    d, files, arrays = k9
    assert ska("merge", "-o", "del_in", files[2], files[0], cwd=d).returncode == 0
    merged = M.merge([arrays[2], arrays[0]])
    gone = [merged.names[3], merged.names[0]]
    with open(d / "list.txt", "w") as f:                                       # blank lines, a second column, a repeated name
        f.write(f"\n{gone[0]}\tsomething/else.fa\n\n{gone[1]}\n{gone[0]} x y\n\n")
    r = ska("delete", "-s", "del_in.skf", "-f", "list.txt", "-o", "del_out", cwd=d)
    assert r.returncode == 0, r.stderr
    assert M.same(m_arr(ora.Array.load(str(d / "del_out.skf"))), M.delete_samples(merged, gone + [gone[0]])) is None
    assert M.same(m_arr(ora.Array.load(str(d / "del_in.skf"))), merged) is None        # -o given: the input stays


def test_cli_weed_without_a_weed_file(E, world, tmp_path):
    # one sample: floor(1 * 0.9) = 0, nothing is filtered and the same rows are written again
    one = M.make_case("k31-one-sample")["inputs"][0]
    p1 = str(tmp_path / "one.skf")
    world.o_arr(one).save(p1)
    r = ska("weed", p1)
    assert r.returncode == 0, r.stderr
    assert M.same(m_arr(ora.Array.load(p1)), M.by_key(one)) is None and (one.var == M.GAP).all(axis=1).any()       # its all-'-' rows too
    # ten samples: the default 0.9 is a threshold of 9 on the stored counts
    ten_case = M.matrix_case("cli-ten", 15, False, (10,), ((0, 300),), 777)
    ten = M.by_key(ten_case["inputs"][0])
    p10 = str(tmp_path / "ten.skf")
    world.o_arr(ten).save(p10)
    want = M.weed(ten, None)
    assert 0 < len(want.keys) < len(ten.keys) and want.counts.min() == 9
    out = str(tmp_path / "ten_out.skf")
    r = ska("weed", p10, "-o", out)
    assert r.returncode == 0, r.stderr
    assert M.same(m_arr(ora.Array.load(out)), want) is None
    assert M.same(m_arr(ora.Array.load(p10)), ten) is None                     # -o: the input stays
    # in place, with a weed file and options
    sets = M.weed_sets(ten_case, ten)
    fa = M.write_fasta(sets["subset"][0], str(tmp_path / "w.fa"))
    r = ska("weed", p10, fa, "--reverse", "--min-freq", "0.3", "--filter", "no-const", "--no-gap-only-sites")
    assert r.returncode == 0, r.stderr
    assert M.same(m_arr(ora.Array.load(p10)), M.weed(ten, sets["subset"][1], True, 0.3, False, 1, False, True)) is None
