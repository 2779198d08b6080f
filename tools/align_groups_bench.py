"""`ska align --groups` through the executable: tools/align_groups_bench.py [n_genomes [n_small]] [--parent DIR]
Builds n (1 000) x 5 Mbp into one .skf, partitions the samples by index into groups of 20 (50 groups at 1 000), and times the one command
`ska align all.skf --groups g.csv -o G` (one run behind one untimed run): process wall time, the phases align.groups_load / groups_verdicts /
groups_rows / groups_write (SKX_PHASES) and the bytes written.  The chain it replaces -- per group `ska delete` of everybody else on a copy of
the file, then `ska align` -- is timed on THREE groups (first, middle, last) and extrapolated to all of them, which the report says; the files
of those groups are compared byte for byte.  Then n_small (100) x 5 Mbp in groups of 10, where the chain is run for every group.
The verdict and compaction kernels are read from one `rocprofv3 --kernel-trace --stats` run of the command (a run of its own, no counters).
--parent DIR: a directory holding another build's `ska` and libskx.so; plain `ska align all.skf -o plain.aln` (which this feature does not
touch) is then timed against it, alternating, five timed runs each behind one untimed run (the criterion: new median wall time within the
parent's own min-max).  A size of 0 leaves that part out."""
import atexit, csv, glob, json, os, re, shutil, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import synth
args = sys.argv[1:]
parent = args[args.index("--parent") + 1] if "--parent" in args else None
sizes = [int(x) for x in args[: args.index("--parent") if "--parent" in args else len(args)] if x.isdigit()]
n_big, n_small = (sizes + [1000, 100][len(sizes):])[:2]
td = tempfile.mkdtemp(dir="/dev/shm")
atexit.register(shutil.rmtree, td, True)          # FASTA, .skf and alignments: gone however the run ends
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
PHASES = ("align.groups_load", "align.groups_verdicts", "align.groups_rows", "align.groups_write")
def run(args, ska=SKA):
    env = dict(os.environ, SKX_PHASES=os.path.join(td, "ph.json"))
    t = time.perf_counter(); r = subprocess.run([ska, *args], cwd=td, capture_output=True, env=env); dt = time.perf_counter() - t
    assert r.returncode == 0, r.stderr[-300:]
    return dt, json.load(open(os.path.join(td, "ph.json")))
def build(count, length, out):
    anc = synth.ancestor(length, seed=1)
    files = []
    for i in range(count):
        p = os.path.join(td, f"g{i}.fa"); synth.to_fasta(synth.sample_stream(anc, i, count, max(1, length // 10_000), max(1, length // 100_000)), p); files.append(p)
        if i % 100 == 99: print(f"#   {i + 1} genomes written", flush=True)
    open(os.path.join(td, "list.txt"), "w").write("".join(f"g{i}\t{files[i]}\n" for i in range(count)))
    run(["build", "-f", "list.txt", "-o", out, "-k", "31", "--threads", "32"])
    print(f"# built {out}.skf: {count} samples x {length} bases, {os.path.getsize(os.path.join(td, out + '.skf')) / 1e9:.2f} GB", flush=True)
    for f in files: os.unlink(f)
def chain(skf, n, members):
    """`ska delete` of everybody else on a copy of the file + `ska align` of the result -> (seconds, the alignment's bytes)"""
    t = time.perf_counter()
    shutil.copyfile(os.path.join(td, skf), os.path.join(td, "cut.skf"))
    open(os.path.join(td, "del.txt"), "w").write("".join(f"g{i}\n" for i in range(n) if i not in members))
    run(["delete", "-s", "cut.skf", "-f", "del.txt"])
    run(["align", "cut.skf", "-o", "chain.aln"])
    dt = time.perf_counter() - t
    return dt, open(os.path.join(td, "chain.aln"), "rb").read()
KERNEL = re.compile(r"(\w+_kernel)")
def kernels(skf, tag):
    d = os.path.join(td, "prof")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", SKA, "align", skf, "--groups", "g.csv", "-o", "P"], cwd=td,
                       capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-300:]
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for ln in open(f).read().splitlines()[1:]:
            x = next(csv.reader([ln]))                             # Name, Calls, TotalDurationNs, ...
            if "subset_verdict" in x[0] or "compact_matrix" in x[0] or "col_stats" in x[0] or "scan_u8" in x[0]:
                print(f"    rocprofv3 {tag}: {KERNEL.search(x[0]).group(1)}  calls {x[1]}  total {int(x[2]) / 1e6:.3f} ms", flush=True)
    shutil.rmtree(d, True)
def case(n, per_group, every_group):
    build(n, 5_000_000, "all")
    groups = [list(range(g, min(g + per_group, n))) for g in range(0, n, per_group)]
    open(os.path.join(td, "g.csv"), "w").write("id,Cluster__autocolour\n" + "".join(f"g{i},{gi + 1}\n" for gi, g in enumerate(groups) for i in g))
    print(f"# {n} samples x 5 Mbp, k = 31, {len(groups)} groups of {per_group}", flush=True)
    run(["align", "all.skf", "--groups", "g.csv", "-o", "G"])
    dt, ph = run(["align", "all.skf", "--groups", "g.csv", "-o", "G"])
    written = sum(os.path.getsize(os.path.join(td, f"G.{gi + 1}.aln")) for gi in range(len(groups)))
    print(f"ska align --groups: wall {dt:6.2f} s   " + "   ".join(f"{k.split('.')[1]} {ph.get(k, 0.0):6.3f} s" for k in PHASES) + f"   {written / 1e6:.1f} MB in {len(groups)} alignments", flush=True)
    ld, lph = run(["align", "all.skf", "-o", "plain.aln"])
    print(f"for scale: plain `ska align all.skf` wall {ld:6.2f} s (load_filtered {lph.get('align.load_filtered', 0.0):.2f} s)", flush=True)
    which = list(range(len(groups))) if every_group else sorted({0, len(groups) // 2, len(groups) - 1})
    secs, same = [], True
    for gi in which:
        s, aln = chain("all.skf", n, set(groups[gi]))
        secs.append(s)
        same &= aln == open(os.path.join(td, f"G.{gi + 1}.aln"), "rb").read()
    total = sum(secs) if every_group else statistics.mean(secs) * len(groups)
    print(f"the chain (copy + ska delete + ska align per group): {len(which)} groups timed, {['%.2f' % s for s in secs]} s; all {len(groups)} groups: {total:.1f} s"
          + ("" if every_group else " (EXTRAPOLATED from the three)") + f"; files equal byte for byte: {same}", flush=True)
    kernels("all.skf", f"{n} x 5 Mbp, {len(groups)} groups")
    if parent:
        print(f"# unchanged path: `ska align all.skf -o plain.aln` of {parent} (parent) against this build, alternating, 5 timed runs each behind one untimed run", flush=True)
        bins = {"parent": os.path.join(os.path.abspath(parent), "ska"), "new": SKA}
        res = {k: [] for k in bins}
        for k, b in bins.items(): run(["align", "all.skf", "-o", f"ab_{k}.aln"], b)
        for _ in range(5):
            for k, b in bins.items(): res[k].append(run(["align", "all.skf", "-o", f"ab_{k}.aln"], b))
        print("    same bytes:", open(os.path.join(td, "ab_parent.aln"), "rb").read() == open(os.path.join(td, "ab_new.aln"), "rb").read(), flush=True)
        for key, tag in ((None, "wall s"), ("align.load_filtered", "load_filtered s")):
            v = {k: sorted((dt if key is None else ph[key]) for dt, ph in res[k]) for k in res}
            print(f"    {tag:<16} parent {['%.3f' % x for x in v['parent']]} median {statistics.median(v['parent']):.3f}   new {['%.3f' % x for x in v['new']]} median {statistics.median(v['new']):.3f}"
                  f"   parent min-max [{v['parent'][0]:.3f}, {v['parent'][-1]:.3f}]: {'within' if statistics.median(v['new']) <= v['parent'][-1] else 'ABOVE'}", flush=True)
    for f in os.listdir(td):
        f = os.path.join(td, f); shutil.rmtree(f) if os.path.isdir(f) else os.unlink(f)
if n_small: case(n_small, 10, True)
if n_big: case(n_big, 20, False)
