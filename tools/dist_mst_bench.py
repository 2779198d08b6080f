"""`ska distance --mst` at BASELINE size through the executable: tools/dist_mst_bench.py [n_genomes [n_large]] [--parent DIR]
Builds n (1 000) x 5 Mbp into one .skf, then times `ska distance all.skf` (five runs behind one untimed run) against --mst, --mst with --max-snps at
the table's 10 % distance quantile, and --closest 1 (three runs each behind one untimed run): process wall time, the distance.pair_sweep /
distance.table_text phases (SKX_PHASES), lines, and what the -v line reports (bands, samples per band, candidates, trees, rounds); whether the --mst
output equals the forest the definition (tests/mst_model.py, on the table's columns) picks from the full table's text.  Then a larger, cheap array
-- 8 000 samples x 50 kbp, whose full table needs 8.2 GB of counters on the device and again on the host -- with one run of each command.
--parent DIR: a directory holding another build's `ska` and libskx.so; `ska distance all.skf` (no selection) is then timed against it, alternating,
five timed runs each behind one untimed run (the criterion: new median pair_sweep within the parent's own min-max).
The forest's kernels and the sweep's are read from one `rocprofv3 --kernel-trace --stats` run (no counters) of --mst.
n_genomes = 0 or n_large = 0 leaves that part out."""
import atexit, csv, glob, os, re, subprocess, sys, time, json, tempfile, shutil, statistics
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
args = sys.argv[1:]
parent = args[args.index("--parent") + 1] if "--parent" in args else None
n = int(args[0]) if args and args[0].isdigit() else 1000
n_large = int(args[1]) if len(args) > 1 and args[1].isdigit() else 8000
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # 5 GB of FASTA and as much .skf: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
INFO = (re.compile(rb"Spanning forest of (\d+) lines in (\d+) trees from (\d+) candidate pairs: (\d+) bands of (\d+) samples, count buffer of (\d+) bytes, at most (\d+) rounds a band"),
        ("lines", "trees", "candidates", "bands", "band_rows", "count_buffer_bytes", "rounds"))
SELECTED = (re.compile(rb"Selected (\d+) lines of (\d+) candidate pairs: (\d+) bands of (\d+) samples, count buffer of (\d+) bytes"),
            ("lines", "candidates", "bands", "band_rows", "count_buffer_bytes"))
def run(args, ska=SKA):
    env = dict(os.environ, SKX_PHASES=os.path.join(td, "ph.json"))
    t = time.perf_counter(); r = subprocess.run([ska, *args], cwd=td, capture_output=True, env=env); dt = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-300:]
    ph = json.load(open(os.path.join(td, "ph.json")))
    for pattern, fields in (INFO, SELECTED):
        m = pattern.search(r.stderr)
        if m: ph["info"] = dict(zip(fields, map(int, m.groups())))
    return dt, ph
def timed(args, runs=3, ska=SKA):
    run(args, ska)
    return [run(args, ska) for _ in range(runs)]
def med(rs, key=None): return statistics.median([dt if key is None else ph.get(key, 0.0) for dt, ph in rs])
def report(tag, rs):
    print(f"{tag:<44} wall {med(rs):6.2f} s   pair_sweep {med(rs, 'distance.pair_sweep') * 1e3:8.1f} ms   table_text {med(rs, 'distance.table_text') * 1e3:7.1f} ms   "
          f"load {med(rs, 'load.stream_decode_filter'):5.2f} s", flush=True)
def build(count, length, out):
    anc = synth.ancestor(length, seed=1)
    files = []
    for i in range(count):
        # (synth's 500 private and 50 shared SNPs are meant for 5 Mbp: the same rates at any length, or a short genome is all variants)
        p = os.path.join(td, f"g{i}.fa"); synth.to_fasta(synth.sample_stream(anc, i, count, max(1, length // 10_000), max(1, length // 100_000)), p); files.append(p)
    open(os.path.join(td, "list.txt"), "w").write("".join(f"g{i}\t{p}\n" for i, p in enumerate(files)))
    run(["build", "-f", "list.txt", "-o", out, "-k", "31", "--threads", "32"])
    print(f"# built {out}.skf: {count} samples x {length} bases", flush=True)
    for f in files: os.unlink(f)
def table_of(path):
    """the table's text -> (lines, i, j, distance) with the values as printed"""
    lines = open(path).read().splitlines(keepends=True)
    i, j, d = np.empty(len(lines) - 1, np.int32), np.empty(len(lines) - 1, np.int32), np.empty(len(lines) - 1)
    for x in range(len(i)):                                             # (one pass, no list of fields: the large table has 32 M lines)
        a, b, c, _ = lines[x + 1].split("\t", 3)
        i[x], j[x], d[x] = int(a[1:]), int(b[1:]), float(c)
    return lines, i, j, d
def forest(S, i, j, d, keep):
    """the definition (tests/mst_model.py: Kruskal under (distance, place in the table); the printed distance orders as the key does) on the
    table's columns -> indices of the forest's lines, ascending"""
    idx = np.flatnonzero(keep)
    idx = idx[np.argsort(d[idx], kind="stable")]
    up, out = list(range(S)), []
    for x, a, b in zip(idx.tolist(), i[idx].tolist(), j[idx].tolist()):
        while up[a] != a: up[a] = up[up[a]]; a = up[a]
        while up[b] != b: up[b] = up[up[b]]; b = up[b]
        if a != b:
            up[max(a, b)] = min(a, b); out.append(x)
            if len(out) == S - 1: break
    return sorted(out)
KERNEL = re.compile(r"(\w+_kernel(<\w+>)?)")
def commands(skf, snps):
    return [("--mst", ["distance", skf, "-v", "-o", "sel.tsv", "--mst"]), (f"--mst --max-snps {snps!r}", ["distance", skf, "-v", "-o", "sel.tsv", "--mst", "--max-snps", repr(snps)]),
            ("--closest 1", ["distance", skf, "-v", "-o", "sel.tsv", "--closest", "1"])]

if n:
    build(n, 5_000_000, "all")
    print(f"# {n} samples x 5 Mbp, k = 31; the full table: 5 runs, a selection: 3 runs, each behind one untimed run; medians", flush=True)
    full = timed(["distance", "all.skf", "-o", "full.tsv"], runs=5)
    report("full table", full)
    sweeps = sorted(ph["distance.pair_sweep"] * 1e3 for _, ph in full)
    print(f"    pair_sweep of the five runs: {['%.1f' % x for x in sweeps]} ms", flush=True)
    lines, ti, tj, td_ = table_of(os.path.join(td, "full.tsv"))
    snps = float(np.quantile(td_, 0.10, method="lower"))
    for tag, cmd in commands("all.skf", snps):
        rs = timed(cmd)
        report(tag, rs)
        note = ""
        if "--mst" in cmd:
            want = [lines[0]] + [lines[1 + x] for x in forest(n, ti, tj, td_, td_ <= snps if "--max-snps" in cmd else np.ones(len(td_), bool))]
            note = f", equal to the forest of the full table's text: {open(os.path.join(td, 'sel.tsv')).read().splitlines(keepends=True) == want}"
        print(f"    info {rs[0][1].get('info')}{note}; pair_sweep median "
              f"{'<=' if med(rs, 'distance.pair_sweep') * 1e3 <= sweeps[-1] else 'ABOVE'} the full table's maximum {sweeps[-1]:.1f} ms", flush=True)
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
    # the kernels under rocprofv3 (a run of its own, kernel trace only, no counters)
    d = os.path.join(td, "prof")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", SKA, "distance", "all.skf", "-o", "prof.tsv", "--mst"], cwd=td, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-300:]
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for ln in open(f).read().splitlines()[1:]:
            if "mst_" in ln or "pair_counts" in ln:
                x = next(csv.reader([ln]))                         # Name, Calls, TotalDurationNs, ...
                print(f"    rocprofv3 --mst: {KERNEL.search(x[0]).group(1)}  calls {x[1]}  total {int(x[2]) / 1e6:.3f} ms", flush=True)
    shutil.rmtree(d, True)
for f in os.listdir(td):
    f = os.path.join(td, f); shutil.rmtree(f) if os.path.isdir(f) else os.unlink(f)
if n_large:
    build(n_large, 50_000, "large")
    print(f"# {n_large} samples x 50 kbp, k = 31: one run of each command", flush=True)
    dt_full, ph_full = run(["distance", "large.skf", "-o", "full.tsv"])
    print(f"full table                                   wall {dt_full:6.2f} s   pair_sweep {ph_full['distance.pair_sweep'] * 1e3:8.1f} ms   table_text {ph_full['distance.table_text'] * 1e3:8.1f} ms   "
          f"count buffer {n_large * n_large * 128} bytes on the device and on the host", flush=True)
    os.unlink(os.path.join(td, "full.tsv"))
    for tag, cmd in commands("large.skf", 0.0)[::2]:
        dt, ph = run(cmd)
        print(f"{tag:<44} wall {dt:6.2f} s   pair_sweep {ph['distance.pair_sweep'] * 1e3:8.1f} ms   table_text {ph.get('distance.table_text', 0.0) * 1e3:8.1f} ms   info {ph.get('info')}", flush=True)
