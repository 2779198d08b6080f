"""`ska qc` through the executable: tools/qc_bench.py [n_genomes [genome_length]]
Builds n (1 000) x 5 Mbp into one .skf and runs `ska qc all.skf -o Q`.  Printed: the process wall time (one run behind one untimed run) and the
phases qc.load / qc.kernels / qc.text (SKX_PHASES); then, from one `rocprofv3 --kernel-trace --stats` run, the time of qc_rows_kernel and
qc_samples_kernel, and from one `rocprofv3 --pmc FETCH_SIZE` run (a run of its own, one counter) the bytes each fetches (FETCH_SIZE counts KB;
gfx950 tallies a 128-byte read request as 64 bytes, so bytes read = FETCH_SIZE x 1024 x 2, as bench.py takes it).  The yardsticks are one read of
the matrix (samples x rows bytes, from the summary file) and the one col_stats_kernel launch of the load in the same run, which reads the
same matrix once: each kernel's time and bytes against it, and the matrix bytes a second each kernel gets through.
Every run is announced before it starts and runs under `timeout -k 10` of its own; the first failure ends the script.  Rehearse with
`tools/qc_bench.py 16 200000` before the full size."""
import atexit, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
sizes = [int(x) for x in sys.argv[1:] if x.isdigit()]
n, length = (sizes + [1000, 5_000_000][len(sizes):])[:2]
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # FASTA, .skf and tables: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PHASES = ("qc.load", "qc.kernels", "qc.text")
KERNELS = ("qc_rows_kernel", "qc_samples_kernel", "col_stats_kernel")
LIMIT = 600                                        # seconds a single run may take
def checked(cmd, what, env=None):
    """one child under a time limit of its own; anything but success ends the script"""
    print(f"# run: {what}", flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), *cmd], cwd=td, capture_output=True, env=env)
    if r.returncode != 0:
        print(f"# FAILED (rc {r.returncode}): {what}\n{r.stderr.decode(errors='replace')[-600:]}", flush=True)
        sys.exit(1)
    return r
def run(args):
    env = dict(os.environ, SKX_PHASES=os.path.join(td, "ph.json"))
    t = time.perf_counter(); checked([SKA, *args], "ska " + " ".join(args), env); dt = time.perf_counter() - t
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
build(n, "all")
cmd = ["qc", "all.skf", "-o", "Q"]
run(cmd)
dt, ph = run(cmd)
print(f"ska qc, {n} x {length} bases: wall {dt:6.2f} s   " + "   ".join(f"{k.split('.')[1]} {ph.get(k, 0.0):6.3f} s" for k in PHASES), flush=True)
summary = dict(l.split("\t")[:2] for l in open(os.path.join(td, "Q.qc.summary.tsv")).read().splitlines()[:6])
flagged = open(os.path.join(td, "Q.qc.flagged.txt")).read().count("\n")
print("    " + "  ".join(f"{k} {v}" for k, v in summary.items()) + f"  flagged {flagged}", flush=True)
rows, S = int(summary["rows"]), int(summary["samples"])
matrix = S * rows                                  # a byte a cell (the padding of a sample's rows to the pitch left out)
d = os.path.join(td, "prof")
times, fetch = {}, {}
checked(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", SKA, *cmd], "rocprofv3 --kernel-trace --stats")
for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
    for ln in open(f).read().splitlines()[1:]:
        x = next(csv.reader([ln]))                                 # Name, Calls, TotalDurationNs, ...
        e = times.setdefault(short(x[0]), [0, 0]); e[0] += int(x[1]); e[1] += int(x[2])
shutil.rmtree(d, True)
checked(["rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--", SKA, *cmd], "rocprofv3 --pmc FETCH_SIZE")
for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
    for row in csv.DictReader(open(f)):
        if row.get("Counter_Name") == "FETCH_SIZE":
            k = short(row["Kernel_Name"]); fetch[k] = fetch.get(k, 0.0) + float(row["Counter_Value"]) * 1024.0 * 2.0
shutil.rmtree(d, True)
print(f"    one read of the matrix: {matrix / 1e9:.3f} GB ({S} samples x {rows} rows)", flush=True)
for k in KERNELS:
    if k in times:
        t_ms = times[k][1] / 1e6
        line = f"    rocprofv3: {k:<18} calls {times[k][0]:>3}  total {t_ms:10.3f} ms  = {matrix / (times[k][1] / 1e9) / 1e12:5.2f} TB/s of matrix"
        if k in fetch: line += f"  fetched {fetch[k] / 1e9:8.3f} GB = {fetch[k] / matrix:.2f} x the matrix"
        print(line, flush=True)
if "col_stats_kernel" in times:
    t_r = times["col_stats_kernel"][1]
    for k in KERNELS[:2]:
        if k in times:
            line = f"    {k}: {times[k][1] / t_r:.2f} x the time of the load's col_stats_kernel pass"
            if k in fetch and "col_stats_kernel" in fetch: line += f", {fetch[k] / fetch['col_stats_kernel']:.2f} x its bytes"
            print(line, flush=True)
