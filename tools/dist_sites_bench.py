"""`ska distance --max-snps N --sites PREFIX` at BASELINE size through the executable: tools/dist_sites_bench.py [n_genomes [genome_length]] [--parent DIR]
Builds n (1 000) x 5 Mbp into one .skf, takes the full table once and picks two --max-snps thresholds from its own distances so that about 1 000 and
about 50 000 lines are selected.  Per threshold: the process wall time without and with --sites (medians of three runs behind one untimed run; the
large selection with --sites: one run behind none, its text is gigabytes), the phases distance.pair_sweep / distance.sites_count / distance.sites_write /
distance.sites_text and the load's (SKX_PHASES), the records and the bytes of PREFIX.sites.tsv.  Then one `rocprofv3 --kernel-trace --stats` run of
the --sites command for the kernels' times and one `rocprofv3 --pmc FETCH_SIZE` run (a run of its own, never combined with tracing) for the bytes
they fetch (FETCH_SIZE counts KB; gfx950 tallies a 128-byte read request as 64 bytes, so bytes read = FETCH_SIZE x 1024 x 2, as bench.py takes it).
The two launches of sites_kernel are set against the algorithmic 2 x U x n_pairs bytes (two samples' cells of every row, per pair) and against the
load's one col_stats_kernel launch in the same run: one read of the same matrix, the yardstick of tools/markers_bench.py.
--parent DIR: a directory holding another build's `ska` and libskx.so; the plain selection (no --sites) at the larger threshold is then timed against
it, alternating, five timed runs each behind one untimed run."""
import atexit, csv, glob, json, os, re, shutil, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
args = sys.argv[1:]
parent = args[args.index("--parent") + 1] if "--parent" in args else None
sizes = [int(x) for x in args if x.isdigit()]
n, length = (sizes + [1000, 5_000_000][len(sizes):])[:2]
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # FASTA, .skf and tables: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PHASES = ("load.stream_decode_filter", "load.read_decode", "distance.pair_sweep", "distance.table_text", "distance.sites_count", "distance.sites_write", "distance.sites_text")
WANTED = ("sites_kernel", "sites_keys_kernel", "pair_totals_kernel", "scan_", "col_stats_kernel", "filter_flags", "pair_counts")
def run(args, ska=SKA):
    env = dict(os.environ, SKX_PHASES=os.path.join(td, "ph.json"))
    t = time.perf_counter(); r = subprocess.run([ska, *args], cwd=td, capture_output=True, env=env); dt = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-300:]
    return dt, json.load(open(os.path.join(td, "ph.json")))
def timed(args, runs=3, warm=True, ska=SKA):
    if warm: run(args, ska)
    return [run(args, ska) for _ in range(runs)]
def med(rs, key=None): return statistics.median([dt if key is None else ph.get(key, 0.0) for dt, ph in rs])
def report(tag, rs):
    print(f"{tag:<34} wall {med(rs):6.2f} s   " + "   ".join(f"{k.split('.')[1]} {med(rs, k) * 1e3:8.1f} ms" for k in PHASES if any(k in ph for _, ph in rs)), flush=True)
def build(count, out):
    anc = synth.ancestor(length, seed=1)
    files = []
    for i in range(count):
        p = os.path.join(td, f"g{i}.fa"); synth.to_fasta(synth.sample_stream(anc, i, count, max(1, length // 10_000), max(1, length // 100_000)), p); files.append(p)
    open(os.path.join(td, "list.txt"), "w").write("".join(f"g{i}\t{files[i]}\n" for i in range(count)))
    t = time.perf_counter(); run(["build", "-f", "list.txt", "-o", out, "-k", "31", "--threads", "16"])
    print(f"# built {out}.skf in {time.perf_counter() - t:.1f} s: {count} samples x {length} bases, {os.path.getsize(os.path.join(td, out + '.skf')) / 1e9:.2f} GB", flush=True)
    for f in files: os.unlink(f)
def short(name):
    m = re.search(r"(\w+)(<[^(]*>)?\(", name)
    return (m.group(1) + (m.group(2) or "")) if m else name[:60]
def profiled(cmd, tag, n_pairs, rows):
    """the kernels of one run: {short name: [calls, total ns]} from --kernel-trace --stats, {short name: bytes fetched} from a --pmc run of its own"""
    d = os.path.join(td, "prof")
    times, fetch = {}, {}
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", SKA, *cmd], cwd=td, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-300:]
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for ln in open(f).read().splitlines()[1:]:
            x = next(csv.reader([ln]))                             # Name, Calls, TotalDurationNs, ...
            e = times.setdefault(short(x[0]), [0, 0]); e[0] += int(x[1]); e[1] += int(x[2])
    shutil.rmtree(d, True)
    r = subprocess.run(["rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--", SKA, *cmd], cwd=td, capture_output=True, timeout=600)
    if r.returncode == 0:
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if row.get("Counter_Name") == "FETCH_SIZE":
                    k = short(row["Kernel_Name"]); fetch[k] = fetch.get(k, 0.0) + float(row["Counter_Value"]) * 1024.0 * 2.0
    else:
        print(f"    rocprofv3 --pmc FETCH_SIZE failed (rc {r.returncode}): {r.stderr[-200:]!r}", flush=True)
    shutil.rmtree(d, True)
    for k in sorted(times, key=lambda k: -times[k][1]):
        if any(w in k for w in WANTED):
            print(f"    rocprofv3 {tag}: {k:<34} calls {times[k][0]:>3}  total {times[k][1] / 1e6:10.3f} ms" + (f"  fetched {fetch[k] / 1e9:8.3f} GB" if k in fetch else ""), flush=True)
    ref = [k for k in times if k.startswith("col_stats_kernel")]
    algorithmic = 2.0 * rows * n_pairs
    for k in ("sites_kernel<false>", "sites_kernel<true>"):
        if k not in times: continue
        t = times[k][1] / 1e9
        line = f"    {tag}: {k} {t * 1e3:.3f} ms; algorithmic 2 x U x n_pairs = {algorithmic / 1e9:.3f} GB -> {algorithmic / t / 1e12:.3f} TB/s of cells"
        if ref:
            t_r = sum(times[r_][1] for r_ in ref) / 1e9
            line += f"; col_stats_kernel {t_r * 1e3:.3f} ms = one read of the matrix"
            if all(r_ in fetch for r_ in ref):
                f_r = sum(fetch[r_] for r_ in ref)
                line += f" ({f_r / 1e9:.3f} GB, {f_r / t_r / 1e12:.3f} TB/s)"
                if k in fetch: line += f"; fetched {fetch[k] / 1e9:.3f} GB = {fetch[k] / f_r:.2f} x the matrix = {fetch[k] / algorithmic:.3f} x algorithmic, {fetch[k] / t / 1e12:.3f} TB/s from memory"
        print(line, flush=True)

build(n, "all")
print(f"# {n} samples x {length} bases, k = 31; medians of three runs behind one untimed run unless said otherwise", flush=True)
run(["distance", "all.skf", "-o", "full.tsv"])
dist = np.sort(np.array([float(ln.split("\t", 3)[2]) for ln in open(os.path.join(td, "full.tsv")).read().splitlines()[1:]]))
os.unlink(os.path.join(td, "full.tsv"))
rows = int(re.search(rb"k-mers=(\d+)", subprocess.run([SKA, "nk", "all.skf"], cwd=td, capture_output=True).stdout).group(1))
print(f"# {len(dist)} pairs, distances {dist[0]:.0f} .. {dist[-1]:.0f} (median {np.median(dist):.0f}); {rows} rows", flush=True)
targets = [t for t in (1000, 50000) if t < len(dist)] or [max(1, len(dist) // 10)]       # (a small trial array: a tenth of its pairs)
thresholds = sorted({float(dist[t - 1]) for t in targets})
for t in thresholds:
    sel = ["distance", "all.skf", "--max-snps", repr(t), "-o", "sel.tsv"]
    plain = timed(sel)
    lines = sum(1 for _ in open(os.path.join(td, "sel.tsv"))) - 1
    report(f"--max-snps {t:g} ({lines} lines)", plain)
    big = lines > 5000
    sites = timed(sel + ["--sites", "S"], runs=1 if big else 3, warm=not big)
    size = os.path.getsize(os.path.join(td, "S.sites.tsv"))
    with open(os.path.join(td, "S.sites.tsv"), "rb") as f: recs = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 24), b"")) - 1
    same = open(os.path.join(td, "sel.tsv"), "rb").read()
    run(sel)
    same = same == open(os.path.join(td, "sel.tsv"), "rb").read()
    report(f"  with --sites" + (" (one run)" if big else ""), sites)
    print(f"    {recs} records ({recs * 16 / 1e6:.1f} MB of records, {recs * 16 / 1e6:.1f} MB of keys), {size / 1e6:.1f} MB of PREFIX.sites.tsv; sum of the lines' distances "
          f"{int(dist[:lines].sum())}; the table's lines equal those without --sites: {same}", flush=True)
    os.unlink(os.path.join(td, "S.sites.tsv"))
    profiled(sel + ["--sites", "S"], f"--max-snps {t:g}", lines, rows)
    os.unlink(os.path.join(td, "S.sites.tsv"))
if parent and thresholds:
    t = thresholds[-1]
    sel = ["distance", "all.skf", "--max-snps", repr(t), "-o"]
    print(f"# unchanged path: `ska distance all.skf --max-snps {t:g}` of {parent} (parent) against this build, alternating, 5 timed runs each behind one untimed run", flush=True)
    bins = {"parent": os.path.join(os.path.abspath(parent), "ska"), "new": SKA}
    res = {k: [] for k in bins}
    for k, b in bins.items(): run(sel + [f"ab_{k}.tsv"], b)
    for _ in range(5):
        for k, b in bins.items(): res[k].append(run(sel + [f"ab_{k}.tsv"], b))
    print("    same bytes:", open(os.path.join(td, "ab_parent.tsv"), "rb").read() == open(os.path.join(td, "ab_new.tsv"), "rb").read(), flush=True)
    for key, unit, tag in ((None, 1.0, "wall s"), ("distance.pair_sweep", 1e3, "pair_sweep ms")):
        v = {k: sorted((dt if key is None else ph[key]) * unit for dt, ph in res[k]) for k in res}
        print(f"    {tag:<14} parent {['%.3f' % x for x in v['parent']]} median {statistics.median(v['parent']):.3f}   new {['%.3f' % x for x in v['new']]} median {statistics.median(v['new']):.3f}"
              f"   parent min-max [{v['parent'][0]:.3f}, {v['parent'][-1]:.3f}]: {'within' if statistics.median(v['new']) <= v['parent'][-1] else 'ABOVE'}", flush=True)
