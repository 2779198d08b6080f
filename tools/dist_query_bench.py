"""`ska distance --query` at BASELINE size through the executable: tools/dist_query_bench.py [n_genomes] [--parent DIR]
Builds n (1 000) x 5 Mbp into one .skf, then times `ska distance all.skf` against `--query` with Q = 1, 8, 64 and 500 (500 drawn at random) and
one `--query-skf` run with 8 samples split off into a second file: process wall time and the distance.pair_sweep / distance.table_text phases
(SKX_PHASES), medians of three runs behind one untimed run.  Each query output is compared with the full table's lines that name a query.
--parent DIR: a directory holding another build's `ska` and libskx.so; `ska distance all.skf` (no query option) is then timed against it,
alternating, five timed runs each behind one untimed run (NOTEBOOK's criterion: new median <= parent median + parent (max - min)), and the
plane builders' and the sweep's kernel times are read from one `rocprofv3 --kernel-trace --stats` run of each."""
import atexit, os, subprocess, sys, time, json, tempfile, shutil, statistics
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
args = sys.argv[1:]
parent = args[args.index("--parent") + 1] if "--parent" in args else None
n = int(args[0]) if args and args[0].isdigit() else 1000
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # 5 GB of FASTA and as much .skf: gone however the run ends
anc = synth.ancestor(5_000_000, seed=1)
files = []
for i in range(n):
    p = os.path.join(td, f"g{i}.fa"); synth.to_fasta(synth.sample_stream(anc, i, n), p); files.append(p)
open(os.path.join(td, "list.txt"), "w").write("".join(f"g{i}\t{p}\n" for i, p in enumerate(files)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
def run(args, ska=SKA):
    env = dict(os.environ, SKX_PHASES=os.path.join(td, "ph.json"))
    t = time.perf_counter(); r = subprocess.run([ska, *args], cwd=td, capture_output=True, env=env); dt = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-300:]
    return dt, json.load(open(os.path.join(td, "ph.json")))
def timed(args, runs=3, ska=SKA):
    run(args, ska)
    return [run(args, ska) for _ in range(runs)]
def med(rs, key=None): return statistics.median([dt if key is None else ph.get(key, 0.0) for dt, ph in rs])
def report(tag, rs):
    print(f"{tag:<34} wall {med(rs):6.2f} s   pair_sweep {med(rs, 'distance.pair_sweep') * 1e3:8.1f} ms   table_text {med(rs, 'distance.table_text') * 1e3:7.1f} ms   "
          f"load {med(rs, 'load.stream_decode_filter'):5.2f} s", flush=True)
def restrict(table, qs):
    return [table[0]] + [ln for ln in table[1:] if ln.split("\t", 2)[0] in qs or ln.split("\t", 2)[1] in qs]
run(["build", "-f", "list.txt", "-o", "all", "-k", "31", "--threads", "32"])
for f in files: os.unlink(f)
print(f"# {n} samples x 5 Mbp, k = 31; medians of 3 runs behind one untimed run", flush=True)
full = timed(["distance", "all.skf", "-o", "full.tsv"])
report("full table", full)
table = open(os.path.join(td, "full.tsv")).read().splitlines()
rng = np.random.default_rng(7)
for q in (1, 8, 64, 500):
    if q >= n: continue
    pick = sorted(rng.choice(n, size=q, replace=False).tolist()) if q == 500 else [int(x) for x in np.rint(np.linspace(0, n - 1, q + 2))[1:-1]]
    names = [f"g{i}" for i in pick]
    open(os.path.join(td, "q.txt"), "w").write("".join(x + "\n" for x in names))
    rs = timed(["distance", "all.skf", "--query-file", "q.txt", "-o", "q.tsv"])
    same = open(os.path.join(td, "q.tsv")).read().splitlines() == restrict(table, set(names))
    report(f"--query, Q = {q}{' (random)' if q == 500 else ''}", rs)
    print(f"    {len(restrict(table, set(names))) - 1} lines, equal to the full table's: {same}; pair_sweep {med(rs, 'distance.pair_sweep') / max(med(full, 'distance.pair_sweep'), 1e-9):.2f} x the full table's", flush=True)
    assert same
if n > 16:
    eight = [f"g{i}" for i in [int(x) for x in np.rint(np.linspace(0, n - 1, 10))[1:-1]]]
    run(["delete", "-s", "all.skf", "-o", "rest", *eight])
    run(["delete", "-s", "all.skf", "-o", "eight", *[f"g{i}" for i in range(n) if f"g{i}" not in eight]])
    rs = timed(["distance", "rest.skf", "--query-skf", "eight.skf", "-o", "qs.tsv"])
    report("--query-skf, 8 samples", rs)
    got = open(os.path.join(td, "qs.tsv")).read().splitlines()
    print(f"    {len(got) - 1} lines (expected {8 * (n - 8) + 28}); merge phases: " + ", ".join(f"{k} {med(rs, k):.2f} s" for k in rs[0][1] if k.startswith("merge.")), flush=True)
    assert len(got) - 1 == 8 * (n - 8) + 28
    for f in ("rest.skf", "eight.skf"): os.unlink(os.path.join(td, f))
if parent:
    print(f"# unchanged path: `ska distance all.skf` of {parent} (parent) against this build, alternating, 5 timed runs each behind one untimed run", flush=True)
    bins = {"parent": os.path.join(parent, "ska"), "new": SKA}
    res = {k: [] for k in bins}
    for k, b in bins.items(): run(["distance", "all.skf", "-o", f"ab_{k}.tsv"], b)
    for _ in range(5):
        for k, b in bins.items(): res[k].append(run(["distance", "all.skf", "-o", f"ab_{k}.tsv"], b))
    print("    same bytes:", open(os.path.join(td, "ab_parent.tsv"), "rb").read() == open(os.path.join(td, "ab_new.tsv"), "rb").read(), flush=True)
    for key, unit, tag in ((None, 1.0, "wall s"), ("distance.pair_sweep", 1e3, "pair_sweep ms")):
        v = {k: sorted((dt if key is None else ph[key]) * unit for dt, ph in res[k]) for k in res}
        bound = statistics.median(v["parent"]) + (v["parent"][-1] - v["parent"][0])
        print(f"    {tag:<14} parent {['%.3f' % x for x in v['parent']]} median {statistics.median(v['parent']):.3f}   new {['%.3f' % x for x in v['new']]} median {statistics.median(v['new']):.3f}"
              f"   bound {bound:.3f}: {'within' if statistics.median(v['new']) <= bound else 'ABOVE'}", flush=True)
    # the plane builders under rocprofv3 (a run of its own per binary, kernel trace only, no counters)
    import glob
    for k, b in bins.items():
        d = os.path.join(td, f"prof_{k}")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", b, "distance", "all.skf", "-o", f"prof_{k}.tsv"], cwd=td, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-300:]
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            lines = open(f).read().splitlines()
            print(f"    rocprofv3 {k}: {lines[0]}", flush=True)
            for ln in lines[1:]:
                if "build_planes" in ln or "pair_counts" in ln or "plane_totals" in ln or "pair_fix" in ln: print(f"    rocprofv3 {k}: {ln}", flush=True)
