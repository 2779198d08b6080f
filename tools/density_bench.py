"""`ska density` through the executable: tools/density_bench.py [n_genomes [genome_length]]
Builds n (1 000) x 5 Mbp into one .skf and runs `ska density g0.fa all.skf -o D --snps`, the first genome as the reference.  Printed: the
process wall time (one run behind one untimed run), the phases density.* (SKX_PHASES), records and regions.  Then one process that loads the
file once and calls Array.sample_qc and Array.snp_density (this script as its own child, `--child`), under `rocprofv3 --kernel-trace --stats`
for the time of both launches of density_kernel and of the rows, sort (rs_*) and dense kernels beside qc_samples_kernel and the load's
col_stats_kernel over the same matrix, and under `rocprofv3 --pmc FETCH_SIZE` (a run of its own, one counter) for the bytes each fetches
(FETCH_SIZE counts KB; gfx950 tallies a 128-byte read request as 64 bytes, so a streaming kernel's bytes read = FETCH_SIZE x 1024 x 2, as
bench.py takes it).  Then the design it replaces: `ska screen all.skf g0.fa`, the same reference as a one-record panel, for screen_kernel's time
and hit windows x S x 64 bytes; and `ska map g0.fa all.skf` with its wall time and the bytes it writes.
Every run is announced before it starts and runs under `timeout -k 10` of its own; the first failure ends the script.  Rehearse with
`tools/density_bench.py 16 200000` before the full size."""
import atexit, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
if len(sys.argv) > 1 and sys.argv[1] == "--child":        # one load, then qc and density on the same array
    import skx_engine as E
    E.load_library()
    arr = E.Array.load(sys.argv[2])
    arr.sample_qc(0.9)
    res = arr.snp_density(sys.argv[3], 1000, 5)
    print("child:", {f: int(res["info"][f]) for f in E.DENSITY_INFO_DT.names}, flush=True)
    sys.exit(0)
import synth
sizes = [int(x) for x in sys.argv[1:] if x.isdigit()]
n, length = (sizes + [1000, 5_000_000][len(sizes):])[:2]
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # FASTA, .skf, tables and alignments: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PHASES = ("density.load", "density.kernels", "density.read_reference", "density.windows", "density.lookup", "density.rows", "density.count", "density.write",
          "density.sort", "density.dense", "density.text")
LIMIT = 600 if n * length > 10**9 else 120         # seconds a single run may take (a rehearsal's runs take a second)
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
    for f in files[1:]: os.unlink(f)               # (the first genome stays: the reference)
def short(name):
    m = re.search(r"(\w+)(<[^(]*>)?\(", name)
    return (m.group(1) + (m.group(2) or "")) if m else name[:60]
def profiled(cmd, what):
    """-> ({kernel: [calls, ns]}, {kernel: FETCH_SIZE bytes as counted}) of one command: a --kernel-trace --stats run, then a --pmc run of its own"""
    d = os.path.join(td, "prof")
    times, fetch = {}, {}
    checked(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", *cmd], f"rocprofv3 --kernel-trace --stats, {what}")
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for ln in open(f).read().splitlines()[1:]:
            x = next(csv.reader([ln]))                             # Name, Calls, TotalDurationNs, ...
            e = times.setdefault(short(x[0]), [0, 0]); e[0] += int(x[1]); e[1] += int(x[2])
    shutil.rmtree(d, True)
    checked(["rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--", *cmd], f"rocprofv3 --pmc FETCH_SIZE, {what}")
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row.get("Counter_Name") == "FETCH_SIZE":
                k = short(row["Kernel_Name"]); fetch[k] = fetch.get(k, 0.0) + float(row["Counter_Value"]) * 1024.0
    shutil.rmtree(d, True)
    return times, fetch
build(n, "all")
cmd = ["density", "g0.fa", "all.skf", "-o", "D", "--snps"]
run(cmd)
dt, ph = run(cmd)
print(f"ska density, {n} x {length} bases: wall {dt:6.2f} s   " + "   ".join(f"{k.split('.')[1]} {ph.get(k, 0.0):6.3f} s" for k in PHASES), flush=True)
summary = [l.split("\t") for l in open(os.path.join(td, "D.density.summary.tsv")).read().splitlines()[1:]]
sites, records = int(summary[0][1]), sum(int(x[5]) for x in summary)
regions = open(os.path.join(td, "D.density.regions.tsv")).read().count("\n") - 1
out_bytes = sum(os.path.getsize(p) for p in glob.glob(os.path.join(td, "D.density.*")))
print(f"    {len(summary)} samples, {sites} sites, {records} SNP records, {sum(int(x[6]) for x in summary)} of them dense, {regions} regions; files {out_bytes / 1e6:.1f} MB", flush=True)
times, fetch = profiled([sys.executable, os.path.abspath(__file__), "--child", "all.skf", "g0.fa"], "one load, qc and density")
rows = None
for k in sorted(times):
    if k.startswith(("density_", "qc_", "col_stats", "rs_", "scan_", "compact_", "map_lookup", "mark_repeats")):
        print(f"    rocprofv3: {k:<28} calls {times[k][0]:>3}  total {times[k][1] / 1e6:10.3f} ms" + (f"  FETCH_SIZE x 2 {2 * fetch[k] / 1e9:8.3f} GB" if k in fetch else ""), flush=True)
if "col_stats_kernel" in fetch:
    matrix = 2 * fetch["col_stats_kernel"] / max(1, times["col_stats_kernel"][0])
    print(f"    one read of the matrix (col_stats_kernel's fetch, doubled): {matrix / 1e9:.3f} GB", flush=True)
    for k in ("density_kernel<false>", "density_kernel<true>", "qc_samples_kernel"):
        if k in times:
            line = f"    {k}: {times[k][1] / 1e6:.3f} ms = {matrix / (times[k][1] / 1e9) / 1e12:.2f} TB/s of matrix"
            if k in fetch: line += f", fetched {2 * fetch[k] / matrix:.2f} x the matrix"
            if "qc_samples_kernel" in times: line += f", {times[k][1] / times['qc_samples_kernel'][1]:.2f} x qc_samples_kernel's time"
            line += f", {times[k][1] / times['col_stats_kernel'][1] * times['col_stats_kernel'][0]:.2f} x one col_stats_kernel pass"
            print(line, flush=True)
# the gather design: the same reference as a one-record panel
scmd = ["screen", "all.skf", "g0.fa", "-o", "S"]
dt_s, _ = run(scmd)
hit = sum(int(l.split("\t")[3]) for l in open(os.path.join(td, "S.screen.summary.tsv")).read().splitlines()[1:])
stimes, sfetch = profiled([SKA, *scmd], "ska screen, the reference as a panel")
if "screen_kernel" in stimes:
    print(f"ska screen, the same reference as a panel: wall {dt_s:6.2f} s; screen_kernel {stimes['screen_kernel'][1] / 1e6:.3f} ms for {hit} hit windows x {n} samples; "
          f"hit windows x S x 64 B = {hit * n * 64 / 1e9:.3f} GB" + (f", FETCH_SIZE {sfetch['screen_kernel'] / 1e9:.3f} GB" if "screen_kernel" in sfetch else ""), flush=True)
# the alignment a separate tool would start from
print(f"# run: ska map g0.fa all.skf -o M.aln  ({3 * n * length / 1e9:.1f} GB of device buffers beside the array, {2 * n * length / 1e9:.1f} GB on the host)", flush=True)
t = time.perf_counter(); r = subprocess.run(["timeout", "-k", "10", str(LIMIT), SKA, "map", "g0.fa", "all.skf", "-o", "M.aln"], cwd=td, capture_output=True); dt_map = time.perf_counter() - t
if r.returncode != 0:                              # the engine's own refusal (buffers that do not fit) is a result; anything else ends the script
    print(f"    ska map: rc {r.returncode} after {dt_map:.1f} s: {r.stderr.decode(errors='replace')[-300:]}", flush=True)
    sys.exit(0 if r.returncode == 101 else 1)
print(f"ska map, the same reference, {n} samples: wall {dt_map:6.2f} s, {os.path.getsize(os.path.join(td, 'M.aln')) / 1e9:.3f} GB written (ska density: {dt:6.2f} s, {out_bytes / 1e6:.1f} MB)", flush=True)
