"""`ska mask` through the executable: tools/mask_bench.py [n_genomes [genome_length]]
Builds n (1 000) x 5 Mbp into one .skf and runs, the first genome as the reference, `ska mask g0.fa all.skf -o M.skf --dense --summary M` and
the same with a BED of 500 kbp (a tenth of the genome; scaled for a rehearsal) beside it.  Printed: the process wall time (one run behind one
untimed run), the phases mask.* (SKX_PHASES), the cells masked and the rows removed.  Then `ska mask --dense --bed` under `rocprofv3
--kernel-trace --stats` for the time of the mask kernels beside the statistics and compaction kernels they are followed by, and -- each in a run
of its own, one counter a run -- under `rocprofv3 --pmc FETCH_SIZE` and `rocprofv3 --pmc WRITE_SIZE` for the bytes they move (both count KB).
Then the route it replaces: `ska density g0.fa all.skf -o D --masked-aln D.aln` with its wall time and the bytes it writes.
Every run is announced before it starts and runs under `timeout -k 10` of its own; the first failure ends the script.  Rehearse with
`tools/mask_bench.py 16 200000` before the full size."""
import atexit, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
sizes = [int(x) for x in sys.argv[1:] if x.isdigit()]
n, length = (sizes + [1000, 5_000_000][len(sizes):])[:2]
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # FASTA, .skf files, tables and the alignment: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PHASES = ("mask.load", "mask.density", "mask.read_intervals", "mask.regions", "mask.read_reference", "mask.windows", "mask.lookup", "mask.kernels", "mask.compact",
          "mask.save", "mask.text")
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
    t = time.perf_counter(); checked([SKA, "build", "-f", "list.txt", "-o", out, "-k", "31", "--threads", "16"], "ska build")
    print(f"# built {out}.skf in {time.perf_counter() - t:.1f} s: {count} samples x {length} bases, {os.path.getsize(os.path.join(td, out + '.skf')) / 1e9:.2f} GB", flush=True)
    for f in files[1:]: os.unlink(f)               # (the first genome stays: the reference)
def short(name):
    m = re.search(r"(\w+)(<[^(]*>)?\(", name)
    return (m.group(1) + (m.group(2) or "")) if m else name[:60]
def kernel_times(cmd, what):
    d = os.path.join(td, "prof"); times = {}
    checked(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", *cmd], f"rocprofv3 --kernel-trace --stats, {what}")
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for ln in open(f).read().splitlines()[1:]:
            x = next(csv.reader([ln]))                             # Name, Calls, TotalDurationNs, ...
            e = times.setdefault(short(x[0]), [0, 0]); e[0] += int(x[1]); e[1] += int(x[2])
    shutil.rmtree(d, True)
    return times
def counter(cmd, name, what):
    """one counter, in a run of its own -> {kernel: bytes as counted}"""
    d = os.path.join(td, "prof"); out = {}
    checked(["rocprofv3", "--pmc", name, "--output-format", "csv", "-d", d, "--", *cmd], f"rocprofv3 --pmc {name}, {what}")
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row.get("Counter_Name") == name:
                k = short(row["Kernel_Name"]); out[k] = out.get(k, 0.0) + float(row["Counter_Value"]) * 1024.0
    shutil.rmtree(d, True)
    return out
def summary(prefix):
    lines = [l.split("\t") for l in open(os.path.join(td, prefix + ".mask.summary.tsv")).read().splitlines()[1:]]
    totals = {l[0]: int(l[1]) for l in lines if len(l) == 2}
    return sum(int(l[4]) for l in lines if len(l) == 5), sum(int(l[1]) for l in lines if len(l) == 5), totals
build(n, "all")
bed_len = max(1, length // 10)
ref_id = open(os.path.join(td, "g0.fa")).readline()[1:].split()[0]
open(os.path.join(td, "phage.bed"), "w").write(f"{ref_id}\t{length // 3}\t{length // 3 + bed_len}\n")
for label, extra in (("--dense", []), (f"--dense --bed ({bed_len} bases)", ["--bed", "phage.bed"])):
    cmd = ["mask", "g0.fa", "all.skf", "-o", "M.skf", "--dense", "--summary", "M", *extra]
    run(cmd)
    dt, ph = run(cmd)
    cells, intervals, totals = summary("M")
    print(f"ska mask {label}, {n} x {length} bases: wall {dt:6.2f} s   " + "   ".join(f"{k.split('.')[1]} {ph.get(k, 0.0):6.3f} s" for k in PHASES), flush=True)
    print(f"    {intervals} merged per-sample intervals, {cells} cells masked, {totals.get('rows_all_samples', 0)} rows in BED intervals, {totals.get('rows_emptied', 0)} rows emptied, "
          f"{totals.get('rows_in', 0)} -> {totals.get('rows_out', 0)} rows; M.skf {os.path.getsize(os.path.join(td, 'M.skf')) / 1e9:.2f} GB", flush=True)
pcmd = [SKA, "mask", "g0.fa", "all.skf", "-o", "P.skf", "--dense", "--bed", "phage.bed"]
times = kernel_times(pcmd, "ska mask --dense --bed")
fetch = counter(pcmd, "FETCH_SIZE", "ska mask --dense --bed")
wrote = counter(pcmd, "WRITE_SIZE", "ska mask --dense --bed")
for k in sorted(times):
    if k.startswith(("mask_", "col_stats", "scan_", "compact_", "density_", "map_lookup", "mark_repeats")):
        print(f"    rocprofv3: {k:<28} calls {times[k][0]:>3}  total {times[k][1] / 1e6:10.3f} ms" + (f"  FETCH_SIZE {fetch[k] / 1e9:8.3f} GB" if k in fetch else "") +
              (f"  WRITE_SIZE {wrote[k] / 1e9:8.3f} GB" if k in wrote else ""), flush=True)
# the route through the alignment
dcmd = ["density", "g0.fa", "all.skf", "-o", "D", "--masked-aln", "D.aln"]
print(f"# run: ska {' '.join(dcmd)}  ({3 * n * length / 1e9:.1f} GB of device buffers beside the array, {2 * n * length / 1e9:.1f} GB on the host)", flush=True)
t = time.perf_counter(); r = subprocess.run(["timeout", "-k", "10", str(LIMIT), SKA, *dcmd], cwd=td, capture_output=True); dt_d = time.perf_counter() - t
if r.returncode != 0:                              # the engine's own refusal (buffers that do not fit) is a result; anything else ends the script
    print(f"    ska density --masked-aln: rc {r.returncode} after {dt_d:.1f} s: {r.stderr.decode(errors='replace')[-300:]}", flush=True)
    sys.exit(0 if r.returncode in (1, 101) else 1)
print(f"ska density --masked-aln, the same input: wall {dt_d:6.2f} s, {os.path.getsize(os.path.join(td, 'D.aln')) / 1e9:.3f} GB written (ska mask --dense: {dt:6.2f} s, "
      f"{os.path.getsize(os.path.join(td, 'M.skf')) / 1e9:.2f} GB, which every command reads)", flush=True)
