"""skx_array_subset_filtered / skh_align_groups / `ska align --groups | --samples` (`-m gpu`), through skx_engine.py and the executable.
A subset's alignment must be, byte for byte, what the engine's own chain writes -- delete_samples(everybody else) + apply_filters + fasta on a
second array of the same dictionaries -- its columns the multiset the oracle chain gives (tests/subset_model.py; row order differs between
engine and oracle), its counts the model's, and the source array must come out of the calls unchanged.  Inputs, groups and the option grid
are the model's (tests/test_subset_model.py holds the model against the oracle on the CPU and shows that every verdict class occurs)."""
import os
import subprocess

import numpy as np
import pytest

import subset_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
FILTERS = M.FILTER_NAMES


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


def _export_equal(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def _kw(o):
    return dict(min_freq=o.min_freq, filter_ambig_as_missing=o.filter_ambig_as_missing, filter_type=o.filter_type, mask_ambig=o.mask_ambig,
                ignore_const_gaps=o.ignore_const_gaps)


@pytest.fixture(scope="module")
def skf31(E, tmp_path_factory):
    """the k = 31 case as FASTA files and as the .skf `ska build` makes of them"""
    d = tmp_path_factory.mktemp("align_groups")
    files = []
    for name, recs in zip(M.names_of("k31"), M.records("k31")):
        p = d / f"{name}.fa"
        p.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
        files.append(str(p))
    r = subprocess.run([SKA, "build", "-o", str(d / "x"), *files], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return {"dir": d, "files": files, "skf": str(d / "x.skf")}


# (case, where the array comes from): DictSet.merge leaves it held as pieces, Array.load as a matrix
SOURCES = [("k31", "merge"), ("k31", "load"), ("k9", "merge"), ("k41", "merge"), ("tiny", "merge")]


@pytest.fixture(scope="module", params=SOURCES, ids=lambda p: f"{p[0]}-{p[1]}")
def source(request, E, skf31):
    case, how = request.param
    k, names = M.CASES[case]["k"], M.names_of(case)
    streams = [E.record_stream(r) for r in M.records(case)]

    def fresh():
        return E.Array.load(skf31["skf"]) if how == "load" else E.DictSet.build(streams, k, True).merge(names)

    arr = fresh()
    print(case, how, "merge path:", E.default_context().merge_path() if how == "merge" else "-", "bytes of pieces:", arr.pieces_info()[0])
    group0 = M.CASES[case]["groups"][0]
    first = arr.subset_filtered(group0, **_kw(M.GRID[0]))               # on the array as it came
    first = (first[0].fasta(), first[1])
    before = arr.export()
    assert arr.names == names and _export_equal(before, fresh().export())
    return {"case": case, "how": how, "arr": arr, "fresh": fresh, "before": before, "names": names, "first": first}


def _chain(src, group, o):
    """the parent's code on a second array: delete_samples(everybody else) + apply_filters + fasta -> (bytes, rows after the delete, removed)"""
    b = src["fresh"]()
    others = [nm for i, nm in enumerate(src["names"]) if i not in group]
    if others:                                                          # (the group of all samples: the delete refuses to remove nothing)
        b.delete_samples(others)
    nrows = b.nrows
    removed = b.apply_filters(o.min_freq, o.filter_ambig_as_missing, o.filter_type, o.mask_ambig, o.ignore_const_gaps)
    return b.fasta(), nrows, removed


def _check_group(src, group, grid):
    var = src["before"][1]
    for o in grid:
        where = (src["case"], src["how"], group, o.ident())
        sub, info = src["arr"].subset_filtered(group, **_kw(o))
        aln = sub.fasta()
        want, nrows, removed = _chain(src, group, o)
        cols, counts = M.model(var, group, o)
        print(where, info)
        assert aln == want, where
        assert sub.names == [src["names"][i] for i in sorted(group)] and sub.nsamples == len(group) and sub.nrows == counts["kept"], where
        assert info == {"rows_present": counts["rows_present"], "removed": counts["removed"], "silent": counts["silent"], "sites": counts["kept"]}, where
        assert (nrows, removed) == (info["rows_present"], info["removed"]), where
        assert M.fasta_columns(aln) == cols, where
        assert cols == M.oracle_chain(src["case"], tuple(group), o)[0], where
        _, only = src["arr"].subset_filtered(group, counts_only=True, **_kw(o))
        assert only == info, where


@pytest.mark.parametrize("g", range(7))
def test_subset_equals_the_chain(source, g):
    groups = M.CASES[source["case"]]["groups"]
    if g >= len(groups):
        return                                                          # (the tiny case has three groups)
    group = groups[g]
    if g == 0:
        aln, info = source["first"]
        assert aln == _chain(source, group, M.GRID[0])[0] and info["sites"] == M.model(source["before"][1], group, M.GRID[0])[1]["kept"]
    _check_group(source, group, M.GRID)
    assert _export_equal(source["arr"].export(), source["before"])     # the source array keeps its content


def test_listing_order_does_not_matter(source):
    rng = np.random.default_rng(7)
    for group in M.CASES[source["case"]]["groups"]:
        if len(group) < 2:
            continue
        o = M.GRID[1 + len(group) % (len(M.GRID) - 1)]
        a, ia = source["arr"].subset_filtered(sorted(group), **_kw(o))
        shuffled = [int(x) for x in rng.permutation(group)]
        if shuffled == sorted(group):
            shuffled = shuffled[::-1]
        b, ib = source["arr"].subset_filtered(shuffled, **_kw(o))
        assert a.fasta() == b.fasta() and ia == ib and a.names == b.names, (group, shuffled)


def test_result_has_no_keys_and_refusals(source, E, tmp_path):
    arr, S = source["arr"], len(source["names"])
    sub, _ = arr.subset_filtered([0, 1] if S > 1 else [0], min_freq=0.0, filter_type=E.FILTER_NONE)
    with pytest.raises(E.EngineError) as ei:
        sub.save(str(tmp_path / "sub.skf"))
    assert ei.value.code == E.EINVAL
    bad = [([], {}), ([0, S], {}), ([-1], {}), ([1, 0, 1], {}), ([0], {"two_stage": True}), ([0], {"min_freq": 1.5}), ([0], {"min_freq": -0.1}),
           ([0], {"min_freq": float("nan")})]
    for samples, kw in bad:
        with pytest.raises(E.EngineError) as ei:
            arr.subset_filtered(samples, **kw)
        assert ei.value.code == E.EINVAL and "] subset:" in str(ei.value), (samples, kw, str(ei.value))
    assert _export_equal(arr.export(), source["before"])


# ---- through the executable (k = 31: what sequence files are built with) ----
CLI_GROUPS = [("clade", [4, 5, 7]), ("pair", [9, 11]), ("trunc", [0, 3]), ("mixed", [12, 1, 8, 2, 10]), ("solo", [6])]
OPTS_A = M.Opts((0.9, False, 1, False, False))                         # the command's defaults
OPTS_B = M.Opts((0.6, True, 3, True, False))
FLAGS_B = ["--min-freq", "0.6", "--filter-ambig-as-missing", "--filter", "no-ambig-or-const", "--ambig-mask"]


def _ska(*args, **kw):
    r = subprocess.run([SKA, *[str(a) for a in args]], capture_output=True, timeout=120, **kw)
    assert r.returncode == 0, (args, r.stderr.decode()[-2000:])
    return r


@pytest.fixture(scope="module")
def cli(E, skf31):
    d = skf31["dir"]
    names = M.names_of("k31")
    rows = [(names[i], label) for label, idx in CLI_GROUPS for i in idx]
    rows = rows[::2] + rows[1::2]                                        # the groups' lines interleaved: a group's order is the file's
    gf = d / "groups.csv"
    gf.write_text("id,Cluster__autocolour\n" + "".join(f"{n},{l}\n" for n, l in rows))
    _ska("align", skf31["skf"], "--groups", gf, "-o", d / "A")
    _ska("align", skf31["skf"], "--groups", gf, "-o", d / "B", "--min-group-size", "1", *FLAGS_B)
    var = E.Array.load(skf31["skf"]).export()[1]
    return {"dir": d, "groups_file": gf, "var": var, "names": names, "labels": [l for l, _ in E.read_groups(str(gf))]}


def _chain_cli(skf31, tmp, group, flags):
    names = M.names_of("k31")
    cut = tmp / "cut.skf"
    cut.write_bytes(open(skf31["skf"], "rb").read())
    _ska("delete", "-s", cut, *[nm for i, nm in enumerate(names) if i not in group])
    out = tmp / "chain.aln"
    _ska("align", cut, "-o", out, *flags)
    return out.read_bytes()


def test_cli_writes_exactly_the_expected_files(cli):
    d = cli["dir"]
    assert sorted(p.name for p in d.iterdir() if p.name.startswith(("A.", "B."))) == sorted(
        [f"A.{l}.aln" for l, _ in CLI_GROUPS if l != "solo"] + ["A.groups.tsv"] + [f"B.{l}.aln" for l, _ in CLI_GROUPS] + ["B.groups.tsv"])
    for prefix, o, min_size in (("A", OPTS_A, 2), ("B", OPTS_B, 1)):
        want = "Group\tSamples\tSplit k-mers\tRemoved\tSites\tFile\n"
        for label in cli["labels"]:                                      # in the order the labels first appear in the file
            group = dict(CLI_GROUPS)[label]
            c = M.model(cli["var"], group, o)[1]
            if len(group) < min_size:
                want += f"{label}\t{len(group)}\t{c['rows_present']}\t-\t-\t-\n"
            else:
                want += f"{label}\t{len(group)}\t{c['rows_present']}\t{c['removed']}\t{c['kept']}\t{d / (prefix + '.' + label + '.aln')}\n"
        assert (d / f"{prefix}.groups.tsv").read_text() == want, prefix
    assert cli["labels"] == [l for l, _ in CLI_GROUPS]


@pytest.mark.parametrize("label,which", [("clade", "A"), ("pair", "A"), ("trunc", "A"), ("mixed", "A"), ("mixed", "B"), ("solo", "B")])
def test_cli_group_equals_delete_then_align(cli, skf31, tmp_path, label, which):
    group = dict(CLI_GROUPS)[label]
    o, flags = (OPTS_A, []) if which == "A" else (OPTS_B, FLAGS_B)
    got = (cli["dir"] / f"{which}.{label}.aln").read_bytes()
    assert got == _chain_cli(skf31, tmp_path, group, flags)
    cols, counts = M.model(cli["var"], group, o)
    assert M.fasta_columns(got) == cols and got.count(b">") == len(group)


def test_cli_samples_equals_the_chain(cli, skf31, tmp_path):
    names, group = cli["names"], [12, 1, 8, 2, 10]
    want = _chain_cli(skf31, tmp_path, group, FLAGS_B)
    r = _ska("align", skf31["skf"], "--samples", ",".join(names[i] for i in group), *FLAGS_B)
    assert r.stdout == want
    lst = tmp_path / "names.txt"
    lst.write_text("".join(names[i] + "\r\n" for i in group) + "\n" + names[group[0]] + "\n")      # CRLF, a blank line, a repeat
    out = tmp_path / "s.aln"
    _ska("align", skf31["skf"], "--samples-file", lst, "-o", out, *FLAGS_B)
    assert out.read_bytes() == want
    r = subprocess.run([SKA, "align", skf31["skf"], "--samples", "s01,nobody"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 101 and 'Could not find sample(s): {"nobody"}' in r.stderr and r.stdout == ""


def test_cli_sequence_files_in_equal_the_skf_form(cli, skf31):
    d = cli["dir"]
    _ska("align", *skf31["files"], "--groups", cli["groups_file"], "-o", d / "F")
    for label, group in CLI_GROUPS:
        if len(group) >= 2:
            assert (d / f"F.{label}.aln").read_bytes() == (d / f"A.{label}.aln").read_bytes(), label
    assert not (d / "F.solo.aln").exists()
    assert (d / "F.groups.tsv").read_text() == (d / "A.groups.tsv").read_text().replace(str(d / "A."), str(d / "F."))


def test_plain_align_is_what_it_was(E, cli, skf31):
    """`ska align x.skf` without the new options keeps its one-pass path: the bytes of load + apply_filters + fasta in this process (code
    the feature does not touch), which the subset of all samples -- defined by the same rules -- must equal as well."""
    plain = _ska("align", skf31["skf"]).stdout
    a = E.Array.load(skf31["skf"])
    a.apply_filters(0.9)
    assert plain == a.fasta()
    assert _ska("align", skf31["skf"], "--samples", ",".join(cli["names"])).stdout == plain
    assert M.fasta_columns(plain) == M.model(cli["var"], list(range(13)), OPTS_A)[0]
