"""Times `ska lo`'s device graph (skx_array_lo_graph) phase by phase on a device-resident synthetic array (bench.py's genomes: synth.py,
default 1 000 samples x 5 Mbp), then `ska lo` end to end on a smaller saved array.  Prints one JSON line.

    python tools/lo_bench.py [--genomes 1000] [--genome-len 5000000] [--e2e-genomes 100] [--e2e-len 5000000] [--threads 16]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
import skx_engine as E   # noqa: E402
import synth             # noqa: E402


def build_array(ctx, n, length, seed=1):
    anc = synth.ancestor(length, seed=seed)
    streams = [synth.sample_stream(anc, i, n, seed=seed).tobytes() for i in range(n)]
    ds = E.DictSet.build(streams, 31, True, ctx=ctx)
    return ds.merge([f"s{i}" for i in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=1000)
    ap.add_argument("--genome-len", type=int, default=5_000_000)
    ap.add_argument("--e2e-genomes", type=int, default=100)
    ap.add_argument("--e2e-len", type=int, default=5_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    E.load_library()
    ctx = E.Context(0)
    out = {"genomes": args.genomes, "genome_len": args.genome_len}
    arr = build_array(ctx, args.genomes, args.genome_len)
    out["rows"] = arr.nrows
    out["matrix_bytes"] = arr.nrows * args.genomes
    ctx.lo_graph(arr).close()                                   # warm-up (allocator, code objects)
    best = None
    for _ in range(args.repeats):
        E.phases(reset=True)
        t0 = time.perf_counter()
        g = ctx.lo_graph(arr)
        wall = time.perf_counter() - t0
        ph = {k: v for k, v in E.phases(reset=True).items() if k.startswith("lo.")}
        if best is None or wall < best[0]:
            best = (wall, ph, g.info)
        g.close()
    out["lo_graph_s"], out["lo_graph_phases_s"], out["graph"] = best
    out["colour_GBps"] = out["matrix_bytes"] / best[1].get("lo.colour", float("nan")) / 1e9
    del arr
    with tempfile.TemporaryDirectory() as td:
        arr = build_array(ctx, args.e2e_genomes, args.e2e_len, seed=2)
        skf = os.path.join(td, "e2e")
        arr.save_skf(skf)
        del arr
        ska = os.path.join(ROOT, "ska.rust_amd", "ska")
        env = dict(os.environ, SKX_PHASES=os.path.join(td, "phases.json"))
        t0 = time.perf_counter()
        r = subprocess.run([ska, "lo", skf + ".skf", os.path.join(td, "lo"), "--threads", str(args.threads)], capture_output=True, text=True, env=env)
        out["e2e_s"] = time.perf_counter() - t0
        out["e2e_rc"] = r.returncode
        if os.path.exists(env["SKX_PHASES"]):
            out["e2e_phases_s"] = {k: v for k, v in json.load(open(env["SKX_PHASES"])).items() if k.startswith("lo.") or k == "main.total"}
        out["e2e_genomes"], out["e2e_len"] = args.e2e_genomes, args.e2e_len
    print(json.dumps(out))


if __name__ == "__main__":
    main()
