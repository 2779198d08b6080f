"""`ska distance --tree / --clusters` (the executable).  The table on stdout must not change; the Newick file must parse, hold every
sample once and carry the splits and lengths the model's writer gives for the engine's joins; the clusters must be the union-find of the
very TSV text the same command wrote.  A synthetic outbreak with two planted clades must show the split between them, and two ranks on
one device must write the same three files as the single process.  The refusals and the help need no device and run everywhere."""
import os
import subprocess

import pytest

import nj_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
GOLD = os.path.join(ROOT, "tests", "golden")


def _ska(*args, cwd, env=None, ok=True):
    r = subprocess.run([SKA, *args], cwd=cwd, capture_output=True, env=dict(os.environ, **(env or {})), timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr[-1500:].decode(errors="replace")
    return r


def _engine_joins(skf):
    """the joins of the table `ska distance <skf>` prints, through skx_engine.py"""
    import skx_engine as E
    arr = E.Array.load(skf)
    d, _, _ = arr.distance_filtered()
    joins = arr.ctx.dist_nj(d, arr.nsamples)
    arr.free()
    return d, joins


def _check_tree(text, names, joins):
    got, (d0, d1) = M.newick_splits(text, names)                       # (asserts: one line, every sample once, children by lowest leaf)
    want, _ = M.newick_splits(M.newick(names, joins), names)
    assert set(got) == set(want) and len(got) == max(2 * len(names) - 3, 1)
    assert all(abs(got[s] - want[s]) < 1e-9 for s in want), [(sorted(s), got[s], want[s]) for s in want if got[s] != want[s]]
    assert abs(d0 - d1) <= 2e-5 * len(names)                          # midpoint: the deepest leaves of the two sides, to the printed decimals
    return got


def _check_cluster_files(wd, prefix, tsv_text, snps, mism):
    names, rows = M.parse_tsv(tsv_text)
    part, csv, dot = M.clusters(names, rows, snps, mism)
    assert open(os.path.join(wd, prefix + ".clusters.csv")).read() == csv
    got_dot = open(os.path.join(wd, prefix + ".graph.dot")).read()
    assert got_dot == dot
    lines = got_dot.splitlines()
    assert lines[0] == "strict graph {" and lines[-1] == "}" and lines[1:1 + len(names)] == [f'\t"{n}";' for n in names]
    assert all(" -- " in ln and ln.startswith("\t") and ln.endswith(";") for ln in lines[1 + len(names):-1])
    assert csv.splitlines()[0] == "id,Cluster__autocolour" and len(csv.splitlines()) == len(names) + 1
    return part


@pytest.mark.gpu
@pytest.mark.parametrize("skf, golden, between", [("multidist.skf", "multidist.stdout", ("1", "0.5")), ("merge.skf", "merge.dist.stdout", None)])
def test_golden_arrays_tree_and_clusters(tmp_path, skf, golden, between):
    wd, src = str(tmp_path), os.path.join(GOLD, "input", skf)
    want = open(os.path.join(GOLD, "correct", golden), "rb").read()
    plain = _ska("distance", src, cwd=wd)
    assert plain.stdout == want
    # everything merges at the defaults (every pair is within 10 SNPs), nothing at a mismatch threshold below the table's smallest
    r = _ska("distance", src, "--tree", "t.nwk", "--clusters", "all", cwd=wd)
    assert r.stdout == want
    names, rows = M.parse_tsv(r.stdout.decode())
    assert max(x[2] for x in rows) <= 10 and min(x[3] for x in rows) > 0.2
    assert len(_check_cluster_files(wd, "all", r.stdout.decode(), 10.0, 1.0)) == 1
    r = _ska("distance", src, "--clusters", "none", "--cluster-mismatches", "0.2", "-o", "table.tsv", cwd=wd)
    assert r.stdout == b"" and open(os.path.join(wd, "table.tsv"), "rb").read() == want
    assert len(_check_cluster_files(wd, "none", want.decode(), 10.0, 0.2)) == len(names)
    if between:
        r = _ska("distance", src, "--clusters", "some", "--cluster-snps", between[0], "--cluster-mismatches", between[1], cwd=wd)
        assert r.stdout == want
        assert 1 < len(_check_cluster_files(wd, "some", r.stdout.decode(), float(between[0]), float(between[1]))) < len(names)
    # the tree
    d, joins = _engine_joins(src)
    text = open(os.path.join(wd, "t.nwk")).read()
    _check_tree(text, names, joins)
    if len(names) == 2:
        half = d["distance"][0] / 2
        assert text == f"({names[0]}:{half:.5f},{names[1]}:{half:.5f});\n"


def _outbreak(tmp_path, n=8, length=60_000, seed=31):
    import synth
    anc = synth.ancestor(length, seed=seed)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for i in range(n):
            p = str(tmp_path / f"ob{i}.fa")
            # synth's clades: the first half of the samples shares one set of SNPs, the second half another
            synth.to_fasta(synth.sample_stream(anc, i, n, private_snps=8, shared_snps=40, seed=seed), p)
            f.write(f"ob{i}\t{p}\n")
    return lst


@pytest.mark.gpu
def test_outbreak_clades_and_two_ranks(tmp_path):
    wd, n = str(tmp_path), 8
    lst = _outbreak(tmp_path, n)
    _ska("build", "-f", lst, "-o", "ob", "--threads", "4", cwd=wd)
    r = _ska("distance", "ob.skf", "--tree", "one.nwk", "--clusters", "one", "--cluster-snps", "60", cwd=wd)
    names, rows = M.parse_tsv(r.stdout.decode())
    assert names == [f"ob{i}" for i in range(n)]
    _, joins = _engine_joins(os.path.join(wd, "ob.skf"))
    got = _check_tree(open(os.path.join(wd, "one.nwk")).read(), names, joins)
    clade = frozenset(range(n // 2, n))
    assert clade in got and got[clade] > 10, sorted((sorted(s), v) for s, v in got.items())
    _check_cluster_files(wd, "one", r.stdout.decode(), 60.0, 1.0)
    # two ranks on the one device, host-staged transport: rank 0 holds the table and writes the same three files
    r2 = _ska("distance", "--gpus", "2", "-f", lst, "--threads", "2", "--tree", "two.nwk", "--clusters", "two", "--cluster-snps", "60", cwd=wd,
              env={"SKX_COMM": "local", "SKX_DEVICE": "0"})
    assert r2.stdout == r.stdout
    for a, b in (("one.nwk", "two.nwk"), ("one.clusters.csv", "two.clusters.csv"), ("one.graph.dot", "two.graph.dot")):
        assert open(os.path.join(wd, a), "rb").read() == open(os.path.join(wd, b), "rb").read(), (a, b)


def test_refusals_in_claps_wording(tmp_path):
    wd = str(tmp_path)
    hint = "\n\nFor more information, try '--help'.\n"
    inval = "error: invalid value '{}' for '{}': {}" + hint
    cases = [
        (["distance", "x.skf", "--clusters", "p", "--cluster-snps", "ten"], inval.format("ten", "--cluster-snps <N>", "invalid float literal")),
        (["distance", "x.skf", "--clusters", "p", "--cluster-snps", "-1"], inval.format("-1", "--cluster-snps <N>", "Threshold must be zero or higher")),
        (["distance", "x.skf", "--clusters", "p", "--cluster-mismatches", "0.1x"], inval.format("0.1x", "--cluster-mismatches <P>", "invalid float literal")),
        (["distance", "x.skf", "--clusters", "p", "--cluster-mismatches", "-0.5"], inval.format("-0.5", "--cluster-mismatches <P>", "Threshold must be zero or higher")),
        (["distance", "x.skf", "--cluster-snps", "3"],
         "error: the following required arguments were not provided:\n  --clusters <PREFIX>\n\nUsage: ska distance [OPTIONS] <SKF_FILE>" + hint),
        (["distance", "x.skf", "--tree", "t", "--cluster-mismatches", "0.3"],
         "error: the following required arguments were not provided:\n  --clusters <PREFIX>\n\nUsage: ska distance [OPTIONS] <SKF_FILE>" + hint),
        (["align", "x.skf", "--tree", "t"], "error: unexpected argument '--tree' found\n\nUsage: ska align [OPTIONS]" + hint),
    ]
    for args, want in cases:
        r = _ska(*args, cwd=wd, ok=False)
        assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", want), (args, r.stderr)


def test_empty_thresholds_and_a_file_that_is_not_there(tmp_path):
    wd = str(tmp_path)
    for flag, arg in (("--cluster-snps", "--cluster-snps <N>"), ("--cluster-mismatches", "--cluster-mismatches <P>")):
        r = _ska("distance", "x.skf", "--clusters", "p", flag, "", cwd=wd, ok=False)
        assert (r.returncode, r.stdout, r.stderr.decode()) == (2, b"", f"error: invalid value '' for '{arg}': cannot parse float from empty string\n\nFor more information, try '--help'.\n")
    # what stands goes on to the banner and ends as a Rust panic would, at the missing device or the missing file, and writes nothing
    r = _ska("distance", "x.skf", "--tree", "t.nwk", "--clusters", "p", cwd=wd, ok=False)
    assert r.returncode == 101 and r.stdout == b"" and r.stderr.decode().startswith("SKA: Split K-mer Analysis") and os.listdir(wd) == []
    assert r.stderr.decode().splitlines()[-1].startswith("error: ")


def test_help_lists_the_new_options():
    out = _ska("distance", "--help", cwd=ROOT).stdout.decode()
    for f in ("--tree <FILE>", "--clusters <PREFIX>", "--cluster-snps <N>", "--cluster-mismatches <P>", "[default: 10]", "[default: 1.0]"):
        assert f in out, f
    assert out.index("--allow-ambiguous") < out.index("--tree <FILE>") < out.index("-v, --verbose")
