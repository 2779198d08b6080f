"""`ska curve` through the executable: tools/curve_bench.py [n_genomes [genome_length]]
Builds n (1 000) x 5 Mbp into one .skf and runs `ska curve all.skf -o C --permutations P` at P = 1, 20 and 100.  Per P: the process wall time (one
run behind one untimed run) and the phases curve.load / curve.orders / curve.kernel / curve.text (SKX_PHASES).  Then, at P = 20 and for either
grid order (orders fastest, or tiles fastest with SKX_KNOBS=curve_tiles_fastest: which of the two runs fastest along the grid), one `rocprofv3 --kernel-trace --stats` run for
curve_kernel's time per order and one `rocprofv3 --pmc FETCH_SIZE` run (a run of its own, one counter) for the bytes it fetches (FETCH_SIZE counts
KB; gfx950 tallies a 128-byte read request as 64 bytes, so bytes read = FETCH_SIZE x 1024 x 2, as bench.py takes it).  The yardstick is the one
col_stats_kernel launch of the load in the same run: one read of the same matrix.  Printed: the kernel's time per order against it, and the fetched
bytes against P x its bytes (1.00 x = every order read the whole matrix from memory; less = orders that walked a tile together shared it in cache).
Every run is announced before it starts and runs under `timeout -k 10` of its own; the first failure ends the script.  Rehearse with
`tools/curve_bench.py 16 200000` before the full size."""
import atexit, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
sizes = [int(x) for x in sys.argv[1:] if x.isdigit()]
n, length = (sizes + [1000, 5_000_000][len(sizes):])[:2]
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # FASTA, .skf and tables: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PHASES = ("curve.load", "curve.orders", "curve.kernel", "curve.text")
LIMIT = 600                                        # seconds a single run may take
def checked(cmd, what, env=None):
    """one child under a time limit of its own; anything but success ends the script"""
    print(f"# run: {what}", flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), *cmd], cwd=td, capture_output=True, env=env)
    if r.returncode != 0:
        print(f"# FAILED (rc {r.returncode}): {what}\n{r.stderr.decode(errors='replace')[-600:]}", flush=True)
        sys.exit(1)
    return r
def run(args, grid=None):
    env = dict(os.environ, SKX_PHASES=os.path.join(td, "ph.json"))
    if grid == "tiles": env["SKX_KNOBS"] = "curve_tiles_fastest"
    t = time.perf_counter(); checked([SKA, *args], "ska " + " ".join(args) + (f"  [grid: {grid} fastest]" if grid else ""), env); dt = time.perf_counter() - t
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
def profiled(cmd, P, grid):
    """curve_kernel and the load's col_stats_kernel of one run: time from --kernel-trace --stats, bytes fetched from a --pmc run of its own"""
    d = os.path.join(td, "prof")
    env = dict(os.environ, **({"SKX_KNOBS": "curve_tiles_fastest"} if grid == "tiles" else {}))
    times, fetch = {}, {}
    checked(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", SKA, *cmd], f"rocprofv3 --kernel-trace --stats, P = {P}, {grid} fastest", env)
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for ln in open(f).read().splitlines()[1:]:
            x = next(csv.reader([ln]))                             # Name, Calls, TotalDurationNs, ...
            e = times.setdefault(short(x[0]), [0, 0]); e[0] += int(x[1]); e[1] += int(x[2])
    shutil.rmtree(d, True)
    checked(["rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--", SKA, *cmd], f"rocprofv3 --pmc FETCH_SIZE, P = {P}, {grid} fastest", env)
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row.get("Counter_Name") == "FETCH_SIZE":
                k = short(row["Kernel_Name"]); fetch[k] = fetch.get(k, 0.0) + float(row["Counter_Value"]) * 1024.0 * 2.0
    shutil.rmtree(d, True)
    for k in ("curve_kernel", "col_stats_kernel"):
        if k in times:
            print(f"    rocprofv3 P = {P}, {grid} fastest: {k:<18} calls {times[k][0]:>3}  total {times[k][1] / 1e6:10.3f} ms" + (f"  fetched {fetch[k] / 1e9:8.3f} GB" if k in fetch else ""), flush=True)
    if "curve_kernel" in times and "col_stats_kernel" in times:
        t_c, t_r = times["curve_kernel"][1], times["col_stats_kernel"][1]
        line = f"    P = {P}, {grid} fastest: curve_kernel {t_c / 1e6 / P:.3f} ms an order = {t_c / P / t_r:.2f} x the load's col_stats pass ({t_r / 1e6:.3f} ms, one read of the matrix)"
        if "curve_kernel" in fetch and "col_stats_kernel" in fetch:
            line += f"; fetched {fetch['curve_kernel'] / 1e9:.3f} GB = {fetch['curve_kernel'] / (P * fetch['col_stats_kernel']):.2f} x P x its {fetch['col_stats_kernel'] / 1e9:.3f} GB"
        print(line, flush=True)
    return times.get("curve_kernel", [0, 0])[1]
build(n, "all")
for P in (1, 20, 100):
    cmd = ["curve", "all.skf", "-o", f"C{P}", "--permutations", str(P)]
    run(cmd)
    dt, ph = run(cmd)
    print(f"ska curve, {n} x {length} bases, P = {P}: wall {dt:6.2f} s   " + "   ".join(f"{k.split('.')[1]} {ph.get(k, 0.0):6.3f} s" for k in PHASES), flush=True)
    last = open(os.path.join(td, f"C{P}.curve.tsv")).read().splitlines()[-1].split("\t")
    print(f"    at t = {last[0]}: pan {last[2]}  core {last[6]}  variant {last[10]}  core_variant {last[14]} (medians)", flush=True)
P = 20
cmd = ["curve", "all.skf", "-o", "G", "--permutations", str(P)]
took = {}
for grid in ("orders", "tiles"):
    dt, ph = run(cmd, grid)
    print(f"ska curve, P = {P}, {grid} fastest: wall {dt:6.2f} s   kernel phase {ph.get('curve.kernel', 0.0):6.3f} s", flush=True)
    took[grid] = profiled(cmd, P, grid)
if all(took.values()):
    print(f"grid order at P = {P}: orders fastest {took['orders'] / 1e6:.3f} ms, tiles fastest {took['tiles'] / 1e6:.3f} ms", flush=True)
