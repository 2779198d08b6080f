"""`ska screen` through the executable: tools/screen_bench.py [n_genomes [genome_length]]
Builds n (1 000) x 5 Mbp into one .skf and cuts two panels from the inputs: records of 2 kbp taken in turn from the first genomes, about a fifth
of a genome in all (1 Mbp) and about a whole one (5 Mbp); every tenth record is foreign (random bases), so not every record is found.  Per panel:
the process wall time of `ska screen all.skf panel.fa -o S` (one run behind one untimed run) and the phases screen.* (SKX_PHASES); one
`rocprofv3 --kernel-trace --stats` run for screen_kernel's time, beside the load's one col_stats_kernel pass (one read of the matrix); one
`rocprofv3 --pmc FETCH_SIZE` run (a run of its own, one counter) for the bytes screen_kernel fetches, against hit windows x S x 64 bytes and
against one read of the matrix; then the same panel through `ska map` on all n samples (its buffers are S x panel length; a run that does not fit is reported
and the script goes on), with its wall time and the bytes it writes.
FETCH_SIZE counts KB in 64-byte requests.  A streaming 16-bytes-a-lane read is tallied at half its bytes on gfx950 (128-byte requests counted as
64: bench.py doubles it, and so does the col_stats figure here); a one-byte gather asks for one 64-byte line a request, so screen_kernel's figure
is taken as it stands and the granule assumed is 64 bytes.  Every run is announced before it starts and runs under `timeout -k 10` of its own;
the first failure ends the script.  Rehearse with `tools/screen_bench.py 16 200000` before the full size."""
import atexit, csv, glob, json, os, re, shutil, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
sizes = [int(x) for x in sys.argv[1:] if x.isdigit()]
n, length = (sizes + [1000, 5_000_000][len(sizes):])[:2]
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # FASTA, .skf, tables and alignments: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PHASES = ("screen.load", "screen.counts", "screen.read_panel", "screen.windows", "screen.lookup", "screen.kernel", "screen.text")
LIMIT = 600 if n * length > 10**9 else 120         # seconds a single run may take (a rehearsal's runs take a second)
RECORD = 2000                                      # bases a panel record
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
def build(count, out, panels):
    """the genomes, the panels cut from the first of them, the .skf"""
    anc = synth.ancestor(length, seed=1)
    files, taken = [], {name: [] for name in panels}
    rng = np.random.default_rng(7)
    for i in range(count):
        p = os.path.join(td, f"g{i}.fa"); synth.to_fasta(synth.sample_stream(anc, i, count, max(1, length // 10_000), max(1, length // 100_000)), p); files.append(p)
        if i < 8:                                  # records of this genome for the panels: its letters without the headers
            seq = b"".join(l for l in open(p, "rb").read().split(b"\n") if not l.startswith(b">"))
            for name, total in panels.items():
                want = total // RECORD // 8
                for j in range(want):
                    at = (j * 7919 * RECORD + i * 104729) % max(1, len(seq) - RECORD)
                    rec = seq[at:at + RECORD] if (len(taken[name]) % 10) else np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, RECORD)].tobytes()
                    taken[name].append(rec)
        if i % 100 == 99: print(f"#   {i + 1} genomes written", flush=True)
    for name, recs in taken.items():
        with open(os.path.join(td, name + ".fa"), "wb") as f:
            for j, r in enumerate(recs): f.write(b">%s_%05d\n%s\n" % (name.encode(), j, r))
        print(f"# panel {name}.fa: {len(recs)} records, {sum(len(r) for r in recs)} bases", flush=True)
    open(os.path.join(td, "list.txt"), "w").write("".join(f"g{i}\t{files[i]}\n" for i in range(count)))
    t = time.perf_counter(); run(["build", "-f", "list.txt", "-o", out, "-k", "31", "--threads", "16"])
    print(f"# built {out}.skf in {time.perf_counter() - t:.1f} s: {count} samples x {length} bases, {os.path.getsize(os.path.join(td, out + '.skf')) / 1e9:.2f} GB", flush=True)
    for f in files: os.unlink(f)
def short(name):
    m = re.search(r"(\w+)(<[^(]*>)?\(", name)
    return (m.group(1) + (m.group(2) or "")) if m else name[:60]
def profiled(cmd, panel, hits, S):
    """screen_kernel and the load's col_stats_kernel of one run: time from --kernel-trace --stats, bytes fetched from a --pmc run of its own"""
    d = os.path.join(td, "prof")
    times, fetch = {}, {}
    checked(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", SKA, *cmd], f"rocprofv3 --kernel-trace --stats, panel {panel}")
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for ln in open(f).read().splitlines()[1:]:
            x = next(csv.reader([ln]))                             # Name, Calls, TotalDurationNs, ...
            e = times.setdefault(short(x[0]), [0, 0]); e[0] += int(x[1]); e[1] += int(x[2])
    shutil.rmtree(d, True)
    checked(["rocprofv3", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", d, "--", SKA, *cmd], f"rocprofv3 --pmc FETCH_SIZE, panel {panel}")
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row.get("Counter_Name") == "FETCH_SIZE":
                k = short(row["Kernel_Name"]); fetch[k] = fetch.get(k, 0.0) + float(row["Counter_Value"]) * 1024.0
    shutil.rmtree(d, True)
    for k in ("screen_kernel", "screen_pack_kernel", "map_lookup_kernel", "col_stats_kernel"):
        if k in times:
            print(f"    rocprofv3 panel {panel}: {k:<18} calls {times[k][0]:>3}  total {times[k][1] / 1e6:10.3f} ms" + (f"  FETCH_SIZE {fetch[k] / 1e9:8.3f} GB" if k in fetch else ""), flush=True)
    if "screen_kernel" in times and "screen_kernel" in fetch:
        t_s, f_s, bound = times["screen_kernel"][1], fetch["screen_kernel"], hits * S * 64.0
        line = f"    panel {panel}: screen_kernel {t_s / 1e6:.3f} ms for {hits} hit windows x {S} samples = {hits * S / (t_s / 1e9) / 1e9:.2f} G cells/s; fetched {f_s / 1e9:.3f} GB = {f_s / bound:.2f} x hits x S x 64 B ({bound / 1e9:.3f} GB)"
        if "col_stats_kernel" in times and "col_stats_kernel" in fetch:
            line += f"; one read of the matrix: col_stats_kernel {times['col_stats_kernel'][1] / 1e6:.3f} ms, {2 * fetch['col_stats_kernel'] / 1e9:.3f} GB (doubled) -> screen_kernel fetched {f_s / (2 * fetch['col_stats_kernel']):.2f} x that"
        print(line, flush=True)
PANELS = {"small": max(8 * RECORD, length // 5), "large": max(8 * RECORD, length)}
build(n, "all", PANELS)
for panel in PANELS:
    cmd = ["screen", "all.skf", panel + ".fa", "-o", "S_" + panel, "--matrix"]
    run(cmd)
    dt, ph = run(cmd)
    print(f"ska screen, {n} x {length} bases, panel {panel}: wall {dt:6.2f} s   " + "   ".join(f"{k.split('.')[1]} {ph.get(k, 0.0):6.3f} s" for k in PHASES), flush=True)
    summary = [l.split("\t") for l in open(os.path.join(td, f"S_{panel}.screen.summary.tsv")).read().splitlines()[1:]]
    hits, windows = sum(int(x[3]) for x in summary), sum(int(x[2]) for x in summary)
    print(f"    {len(summary)} records, {windows} windows, {hits} hit; {sum(int(x[4]) for x in summary)} (record, sample) pairs pass; "
          f"records nobody carries: {sum(1 for x in summary if x[4] == '0')}; screen.tsv {os.path.getsize(os.path.join(td, f'S_{panel}.screen.tsv')) / 1e6:.1f} MB", flush=True)
    profiled(cmd, panel, hits, n)
    # the same panel through `ska map`: three S x panel-length device buffers beside the matrix, and the alignment on the host
    total = sum(int(x[1]) for x in summary)
    print(f"# run: ska map {panel}.fa all.skf -o M_{panel}.aln  ({3 * n * total / 1e9:.1f} GB of device buffers beside the array, {2 * n * total / 1e9:.1f} GB on the host)", flush=True)
    t = time.perf_counter(); r = subprocess.run(["timeout", "-k", "10", str(LIMIT), SKA, "map", panel + ".fa", "all.skf", "-o", "M_" + panel + ".aln"], cwd=td, capture_output=True); dt_map = time.perf_counter() - t
    if r.returncode != 0:                          # the engine's own refusal (buffers that do not fit) is a result; anything else ends the script
        print(f"    ska map: rc {r.returncode} after {dt_map:.1f} s: {r.stderr.decode(errors='replace')[-300:]}", flush=True)
        if r.returncode != 101: sys.exit(1)
        continue
    size = os.path.getsize(os.path.join(td, f"M_{panel}.aln"))
    print(f"ska map, the same panel, {n} samples: wall {dt_map:6.2f} s, {size / 1e9:.3f} GB written (ska screen: {dt:6.2f} s, "
          f"{sum(os.path.getsize(p) for p in glob.glob(os.path.join(td, f'S_{panel}.screen.*'))) / 1e6:.1f} MB)", flush=True)
    os.unlink(os.path.join(td, f"M_{panel}.aln"))
