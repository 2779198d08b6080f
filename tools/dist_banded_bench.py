"""`ska distance --no-table` at BASELINE size through the executable: tools/dist_banded_bench.py [n_genomes [n_large [n_same]]] [--parent DIR]
Builds n (1 000) x 5 Mbp into one .skf and times, for the outputs `--clusters`, `--tree` and both, `ska distance all.skf --no-table <outputs>`
against the table path `ska distance all.skf -o full.tsv <outputs>` (three runs each behind one untimed run, medians): process wall time, the
phases distance.pair_sweep / distance.nj / distance.tree_text / distance.clusters / distance.table_text (SKX_PHASES), what the -v line reports
(bands, samples per band, count buffer, edges, clusters) and whether the files are the table path's, byte for byte.  --cluster-snps is the
table's 1 % distance quantile.  The consumers' and the sweep's kernel times are read from one `rocprofv3 --kernel-trace --stats` run (no
counters) of the form with both outputs.
The same array with --cluster-snps 1e9, and n_same (1 000) copies of one 50 kbp genome (where no row varies and the sweep has nothing to
count), are the union kernel's worst case -- every pair is an edge: wall time, equality and kernel times, those of the plain union
(SKX_KNOBS=union_per_edge=1: one link per edge instead of one per distinct root of a wave's part of the row) beside them.
Then a larger, cheap array -- n_large (8 000) samples x 50 kbp -- with one run of each form and output.
--parent DIR: a directory holding another build's `ska` and libskx.so; `ska distance all.skf` (the plain table, which this form does not touch)
is then timed against it, alternating, five timed runs each behind one untimed run (the criterion: new median pair_sweep within the parent's own
min-max).  A size of 0 leaves that part out."""
import atexit, csv, glob, os, re, subprocess, sys, time, json, tempfile, shutil, statistics
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
args = sys.argv[1:]
parent = args[args.index("--parent") + 1] if "--parent" in args else None
sizes = [int(x) for x in args[: args.index("--parent") if "--parent" in args else len(args)] if x.isdigit()]
n, n_large, n_same = (sizes + [1000, 8000, 1000][len(sizes):])[:3]
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # 5 GB of FASTA and as much .skf: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PHASES = ("distance.pair_sweep", "distance.nj", "distance.tree_text", "distance.clusters", "distance.table_text")
def run(args, ska=SKA):
    env = dict(os.environ, SKX_PHASES=os.path.join(td, "ph.json"))
    t = time.perf_counter(); r = subprocess.run([ska, *args], cwd=td, capture_output=True, env=env); dt = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-300:]
    ph = json.load(open(os.path.join(td, "ph.json")))
    m = re.search(rb"No table: (\d+) bands of (\d+) samples, count buffer of (\d+) bytes; (\d+) pairs within the cluster thresholds, (\d+) clusters", r.stderr)
    if m: ph["info"] = dict(zip(("bands", "band_rows", "count_buffer_bytes", "edges", "clusters"), map(int, m.groups())))
    return dt, ph
def timed(args, runs=3, ska=SKA):
    run(args, ska)
    return [run(args, ska) for _ in range(runs)]
def med(rs, key=None): return statistics.median([dt if key is None else ph.get(key, 0.0) for dt, ph in rs])
def report(tag, rs):
    print(f"{tag:<34} wall {med(rs):6.2f} s   " + "   ".join(f"{k.split('.')[1]} {med(rs, k) * 1e3:8.1f} ms" for k in PHASES) +
          f"   (nj.steps {med(rs, 'nj.steps') * 1e3:.1f} ms, hipMalloc {med(rs, 'alloc.hipMalloc_all_threads') * 1e3:.1f} ms)   load {med(rs, 'load.stream_decode_filter'):5.2f} s", flush=True)
def build(count, length, out, same=False):
    anc = synth.ancestor(length, seed=1)
    files = []
    for i in range(1 if same else count):
        # (synth's 500 private and 50 shared SNPs are meant for 5 Mbp: the same rates at any length, or a short genome is all variants)
        p = os.path.join(td, f"g{i}.fa"); synth.to_fasta(synth.sample_stream(anc, i, count, max(1, length // 10_000), max(1, length // 100_000)), p); files.append(p)
        if i % 100 == 99: print(f"#   {i + 1} genomes written", flush=True)
    open(os.path.join(td, "list.txt"), "w").write("".join(f"g{i}\t{files[0 if same else i]}\n" for i in range(count)))
    run(["build", "-f", "list.txt", "-o", out, "-k", "31", "--threads", "32"])
    print(f"# built {out}.skf: {count} samples x {length} bases" + (", all the same genome" if same else ""), flush=True)
    for f in files: os.unlink(f)
OUTPUTS = {"clusters": ["--clusters", "c"], "tree": ["--tree", "t.nwk"], "both": ["--tree", "t.nwk", "--clusters", "c"]}
FILES = {"clusters": ["c.clusters.csv"], "tree": ["t.nwk"], "both": ["t.nwk", "c.clusters.csv"]}
def files_of(which):
    """the output files of the run just made, which are then removed"""
    got = {f: open(os.path.join(td, f), "rb").read() for f in FILES.get(which, [])}
    for f in ("t.nwk", "c.clusters.csv", "c.graph.dot"):
        if os.path.exists(os.path.join(td, f)): os.unlink(os.path.join(td, f))
    return got
def compare(skf, snps, runs, which_ones=("clusters", "tree", "both")):
    sweeps = {}
    for which in which_ones:
        extra = OUTPUTS[which] + (["--cluster-snps", repr(snps)] if which != "tree" else [])
        table = timed(["distance", skf, "-o", "full.tsv", *extra], runs) if runs > 1 else [run(["distance", skf, "-o", "full.tsv", *extra])]
        dot = os.path.exists(os.path.join(td, "c.graph.dot"))
        want = files_of(which)
        banded = timed(["distance", skf, "-v", "--no-table", *extra], runs) if runs > 1 else [run(["distance", skf, "-v", "--no-table", *extra])]
        no_dot = not os.path.exists(os.path.join(td, "c.graph.dot"))
        same = files_of(which) == want
        report(f"table      {' '.join(OUTPUTS[which])}", table)
        report(f"--no-table {' '.join(OUTPUTS[which])}", banded)
        print(f"    info {banded[0][1].get('info')}; files equal to the table path's: {same}; graph.dot written by the table path only: {(dot and no_dot) or which == 'tree'}", flush=True)
        sweeps[which] = (med(table, "distance.pair_sweep") * 1e3, med(banded, "distance.pair_sweep") * 1e3)
    return sweeps
KERNEL = re.compile(r"(\w+_kernel)")
def kernels(skf, extra, tag, knobs=None, runs=1):
    """the kernels of one --no-table run under rocprofv3 (a run of its own, kernel trace only, no counters); knobs: SKX_KNOBS of that run"""
    if runs > 1:
        for x in range(runs): kernels(skf, extra, f"{tag}, run {x + 1}", knobs)
        return
    d = os.path.join(td, "prof")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", SKA, "distance", skf, "--no-table", *extra], cwd=td, capture_output=True, timeout=600,
                       env=dict(os.environ, SKX_KNOBS=knobs) if knobs else None)
    assert r.returncode == 0, r.stderr[-300:]
    nj = [0, 0.0]
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for ln in open(f).read().splitlines()[1:]:
            x = next(csv.reader([ln]))                             # Name, Calls, TotalDurationNs, ...
            if "nj_" in x[0]: nj[0] += int(x[1]); nj[1] += int(x[2]) / 1e6
            elif "cluster_" in x[0] or "dist_fill" in x[0] or "pair_counts" in x[0]:
                print(f"    rocprofv3 {tag}: {KERNEL.search(x[0]).group(1)}  calls {x[1]}  total {int(x[2]) / 1e6:.3f} ms", flush=True)
    if nj[0]: print(f"    rocprofv3 {tag}: the nj_* kernels  calls {nj[0]}  total {nj[1]:.3f} ms", flush=True)
    shutil.rmtree(d, True)
    files_of(None)
def snps_quantile(path, q):
    return float(np.quantile(np.loadtxt(path, delimiter="\t", skiprows=1, usecols=2), q, method="lower"))
def clean():
    for f in os.listdir(td):
        f = os.path.join(td, f); shutil.rmtree(f) if os.path.isdir(f) else os.unlink(f)

if n:
    build(n, 5_000_000, "all")
    print(f"# {n} samples x 5 Mbp, k = 31; every command: 3 runs behind one untimed run; medians", flush=True)
    run(["distance", "all.skf", "-o", "full.tsv"])
    snps = snps_quantile(os.path.join(td, "full.tsv"), 0.01)
    print(f"# --cluster-snps {snps!r} (the table's 1 % distance quantile)", flush=True)
    compare("all.skf", snps, 3)
    if parent:
        print(f"# unchanged path: `ska distance all.skf` of {parent} (parent) against this build, alternating, 5 timed runs each behind one untimed run", flush=True)
        bins = {"parent": os.path.join(os.path.abspath(parent), "ska"), "new": SKA}
        res = {k: [] for k in bins}
        for k, b in bins.items(): run(["distance", "all.skf", "-o", f"ab_{k}.tsv"], b)
        for _ in range(5):
            for k, b in bins.items(): res[k].append(run(["distance", "all.skf", "-o", f"ab_{k}.tsv"], b))
        print("    same bytes:", open(os.path.join(td, "ab_parent.tsv"), "rb").read() == open(os.path.join(td, "ab_new.tsv"), "rb").read(), flush=True)
        for key, unit, tag in ((None, 1.0, "wall s"), ("distance.pair_sweep", 1e3, "pair_sweep ms")):
            v = {k: sorted((dt if key is None else ph[key]) * unit for dt, ph in res[k]) for k in res}
            print(f"    {tag:<14} parent {['%.3f' % x for x in v['parent']]} median {statistics.median(v['parent']):.3f}   new {['%.3f' % x for x in v['new']]} median {statistics.median(v['new']):.3f}"
                  f"   parent min-max [{v['parent'][0]:.3f}, {v['parent'][-1]:.3f}]: {'within' if statistics.median(v['new']) <= v['parent'][-1] else 'ABOVE'}", flush=True)
    kernels("all.skf", OUTPUTS["both"] + ["--cluster-snps", repr(snps)], f"{n} x 5 Mbp, both outputs")
    # a fully connected band behind a sweep that has rows to count: the same array with a threshold no pair exceeds
    rs = timed(["distance", "all.skf", "-v", "--no-table", "--clusters", "c", "--cluster-snps", "1e9"])
    report("--no-table --clusters c, 1e9 SNPs", rs)
    print(f"    info {rs[0][1].get('info')}", flush=True)
    kernels("all.skf", ["--clusters", "c", "--cluster-snps", "1e9"], f"{n} x 5 Mbp, every pair an edge", runs=3)
    kernels("all.skf", ["--clusters", "c", "--cluster-snps", "1e9"], f"{n} x 5 Mbp, every pair an edge, one link per edge", "union_per_edge=1", runs=3)
clean()
if n_same:
    build(n_same, 50_000, "same", same=True)
    print(f"# {n_same} copies of one genome: every pair is an edge (no row varies, so the sweep itself has nothing to count)", flush=True)
    compare("same.skf", 0.0, 3, ("clusters",))
    kernels("same.skf", ["--clusters", "c", "--cluster-snps", "0"], f"{n_same} identical, clusters", runs=3)
    kernels("same.skf", ["--clusters", "c", "--cluster-snps", "0"], f"{n_same} identical, clusters, one link per edge", "union_per_edge=1", runs=3)
clean()
if n_large:
    build(n_large, 50_000, "large")
    print(f"# {n_large} samples x 50 kbp, k = 31: one run of each command; the table path holds {n_large * n_large * 128} bytes of counters on the device and on the host", flush=True)
    run(["distance", "large.skf", "-o", "full.tsv"])
    snps = snps_quantile(os.path.join(td, "full.tsv"), 0.01)
    print(f"# --cluster-snps {snps!r} (the table's 1 % distance quantile)", flush=True)
    compare("large.skf", snps, 1)
    kernels("large.skf", OUTPUTS["both"] + ["--cluster-snps", repr(snps)], f"{n_large} x 50 kbp, both outputs")
