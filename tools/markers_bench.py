"""`ska markers` through the executable: tools/markers_bench.py [n_genomes [genome_length]]
Builds n (1 000) x 5 Mbp into one .skf and runs `ska markers all.skf --groups FILE -o M` on two partitions of it: groups of 20 by index (50 groups at
1 000) and n singleton groups.  Per partition: the process wall time (one run behind one untimed run), the phases markers.load / markers.pass /
markers.text (SKX_PHASES), the records written; then one `rocprofv3 --kernel-trace --stats` run of the same command for the kernels' times and one
`rocprofv3 --pmc FETCH_SIZE` run (a run of its own) for the bytes they fetch (FETCH_SIZE counts KB; gfx950 tallies a 128-byte read request as 64
bytes, so bytes read = FETCH_SIZE x 1024 x 2, as bench.py takes it).  The yardstick is the one col_stats_kernel launch of the load in the same
run: one read of the same matrix.  Printed: the ratio of the markers kernels' time to it, and of their fetched bytes to it -- the count pass walks
the matrix twice and the write pass once more, so 3 x the yardstick's bytes means nothing was served from cache and less means the re-reads were."""
import atexit, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
sizes = [int(x) for x in sys.argv[1:] if x.isdigit()]
n, length = (sizes + [1000, 5_000_000][len(sizes):])[:2]
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # FASTA, .skf and tables: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PHASES = ("markers.load", "markers.pass", "markers.text")
WANTED = ("markers_kernel", "markers_gather_kernel", "col_stats_kernel", "radix", "rs_")
def run(args):
    env = dict(os.environ, SKX_PHASES=os.path.join(td, "ph.json"))
    t = time.perf_counter(); r = subprocess.run([SKA, *args], cwd=td, capture_output=True, env=env); dt = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-300:]
    return dt, json.load(open(os.path.join(td, "ph.json")))
def build(count, out):
    anc = synth.ancestor(length, seed=1)
    files = []
    for i in range(count):
        p = os.path.join(td, f"g{i}.fa"); synth.to_fasta(synth.sample_stream(anc, i, count, max(1, length // 10_000), max(1, length // 100_000)), p); files.append(p)
        if i % 100 == 99: print(f"#   {i + 1} genomes written", flush=True)
    open(os.path.join(td, "list.txt"), "w").write("".join(f"g{i}\t{files[i]}\n" for i in range(count)))
    t = time.perf_counter(); run(["build", "-f", "list.txt", "-o", out, "-k", "31", "--threads", "16"])
    print(f"# built {out}.skf in {time.perf_counter() - t:.1f} s: {count} samples x {length} bases, {os.path.getsize(os.path.join(td, out + '.skf')) / 1e9:.2f} GB", flush=True)
    for f in files: os.unlink(f)
def short(name):
    m = re.search(r"(\w+)(<[^(]*>)?\(", name)
    return (m.group(1) + (m.group(2) or "")) if m else name[:60]
def profiled(cmd, tag):
    """the kernels of one run: {short name: [calls, total ns]} from --kernel-trace --stats, {short name: bytes fetched} from a --pmc run of its own"""
    d = os.path.join(td, "prof")
    times, fetch = {}, {}
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", SKA, *cmd], cwd=td, capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-300:]
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for ln in open(f).read().splitlines()[1:]:
            x = next(csv.reader([ln]))                             # Name, Calls, TotalDurationNs, ...
            e = times.setdefault(short(x[0]), [0, 0]); e[0] += int(x[1]); e[1] += int(x[2])
    shutil.rmtree(d, True)
    r = subprocess.run(["rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--", SKA, *cmd], cwd=td, capture_output=True, timeout=900)
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
    mk = [k for k in times if k.startswith("markers_kernel")]
    ref = [k for k in times if k.startswith("col_stats_kernel")]
    if mk and ref:
        t_m, t_r = sum(times[k][1] for k in mk), sum(times[k][1] for k in ref)
        line = f"    {tag}: markers kernels {t_m / 1e6:.3f} ms = {t_m / t_r:.2f} x the load's col_stats pass ({t_r / 1e6:.3f} ms, one read of the matrix)"
        if all(k in fetch for k in mk + ref):
            f_m, f_r = sum(fetch[k] for k in mk), sum(fetch[k] for k in ref)
            line += f"; fetched {f_m / 1e9:.3f} GB = {f_m / f_r:.2f} x its {f_r / 1e9:.3f} GB (3 walks: 3.00 x = no walk served from cache)"
        print(line, flush=True)
def case(tag, groups):
    gf = f"{tag}.csv"
    open(os.path.join(td, gf), "w").write("".join(f"g{i},{gi + 1}\n" for gi, g in enumerate(groups) for i in g))
    cmd = ["markers", "all.skf", "--groups", gf, "-o", "M_" + tag]
    run(cmd)
    dt, ph = run(cmd)
    recs = sum(1 for _ in open(os.path.join(td, f"M_{tag}.markers.tsv"))) - 1
    print(f"ska markers, {n} x {length} bases, {len(groups)} groups ({tag}): wall {dt:6.2f} s   " + "   ".join(f"{k.split('.')[1]} {ph.get(k, 0.0):6.3f} s" for k in PHASES)
          + f"   {recs} records, {os.path.getsize(os.path.join(td, f'M_{tag}.markers.tsv')) / 1e6:.1f} MB of table", flush=True)
    profiled(cmd, tag)
build(n, "all")
case("groups_of_20", [list(range(g, min(g + 20, n))) for g in range(0, n, 20)])
case("singletons", [[i] for i in range(n)])
