"""Times device neighbour joining (skx_matrix_nj) on additive matrices made in numpy -- no files -- and prints one JSON line.

    python tools/nj_bench.py [--sizes 1000,4000,10000] [--model-sizes 1000,2000] [--repeats 3] [--cli-genomes 0] [--cli-genome-len 5000000]

Per size: the whole call (check + upload + steps + copy-back), the steps alone (the engine's "nj.steps" phase), time per step, and bytes per
second taking 8 n^2 bytes per step as the algorithmic traffic (n = the nodes active at that step; the row pass reads the upper half of the
live block, so the kernel moves about half of that).  "launch_floor_us_per_step" is the time per step at S = 64 in the same run, where the
four launches of a step have next to nothing to do: what a step costs when only its launches count.  --model-sizes times the numpy model of
tests/nj_model.py on the same matrices.  --cli-genomes N builds an N-genome array the way bench.py makes its genomes (files under /dev/shm)
and times `ska distance` on it with and without --tree."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ska.rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skx_engine as E   # noqa: E402


def additive(S, seed):
    """path lengths of a random binary tree with integer branch lengths 1..20 (the generator of tests/nj_model.py without its bookkeeping)"""
    rng = np.random.default_rng(seed)
    D = np.zeros((S, S))
    cl = [(np.array([i]), np.zeros(1)) for i in range(S)]
    while len(cl) > 1:
        i, j = sorted(rng.choice(len(cl), 2, replace=False))
        (l1, d1), (l2, d2) = cl[i], cl[j]
        b1, b2 = (int(v) for v in rng.integers(1, 21, 2))
        blk = d1[:, None] + (b1 + b2) + d2[None, :]
        D[np.ix_(l1, l2)] = blk
        D[np.ix_(l2, l1)] = blk.T
        cl[i] = (np.concatenate([l1, l2]), np.concatenate([d1 + b1, d2 + b2]))
        del cl[j]
    return D


def time_nj(ctx, D, repeats):
    S = D.shape[0]
    best = None
    for _ in range(repeats):
        E.phases(reset=True)
        t = time.perf_counter()
        joins = ctx.matrix_nj(D)
        total = time.perf_counter() - t
        ph = E.phases()
        if best is None or ph["nj.steps"] < best["steps_s"]:
            best = {"total_s": total, "steps_s": ph["nj.steps"], "check_s": ph.get("nj.check_matrix", 0.0), "upload_s": ph.get("nj.upload", 0.0)}
    steps = max(S - 2, 1)
    traffic = 8.0 * sum(n * n for n in range(3, S + 1))
    best.update(S=S, us_per_step=1e6 * best["steps_s"] / steps, algorithmic_TB_per_s=traffic / best["steps_s"] / 1e12,
                joins_digest=int(np.frombuffer(joins.tobytes(), np.uint8).astype(np.uint64).sum()))
    return best


def cli_leg(n, length):
    import synth
    td = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        anc = synth.ancestor(length, seed=1)
        with open(os.path.join(td, "list.txt"), "w") as f:
            for i in range(n):
                p = os.path.join(td, f"g{i}.fa")
                synth.to_fasta(synth.sample_stream(anc, i, n), p)
                f.write(f"g{i}\t{p}\n")
        ska = os.path.join(ROOT, "ska.rust_amd", "ska")

        def run(args):
            env = dict(os.environ, SKX_PHASES=os.path.join(td, "ph.json"))
            t = time.perf_counter()
            r = subprocess.run([ska, *args], cwd=td, capture_output=True, env=env, timeout=1100)
            dt = time.perf_counter() - t
            assert r.returncode == 0, r.stderr[-400:]
            return dt, json.load(open(os.path.join(td, "ph.json")))
        run(["build", "-f", "list.txt", "-o", "all", "--threads", "16"])
        out = {"genomes": n, "genome_len": length}
        for tag, flags in (("plain", []), ("tree", ["--tree", "t.nwk"]), ("tree_clusters", ["--tree", "t.nwk", "--clusters", "c"])):
            best = None
            for _ in range(2):
                dt, ph = run(["distance", "all.skf", "-o", "d.tsv", *flags])
                if best is None or dt < best[0]:
                    best = (dt, ph)
            out[tag] = {"wall_s": round(best[0], 3), "phases": {k: round(v, 4) for k, v in best[1].items() if k.startswith(("distance.", "nj."))}}
        out["newick_bytes"] = os.path.getsize(os.path.join(td, "t.nwk"))
        return out
    finally:
        shutil.rmtree(td, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,4000,10000")
    ap.add_argument("--model-sizes", default="1000,2000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cli-genomes", type=int, default=0)
    ap.add_argument("--cli-genome-len", type=int, default=5_000_000)
    args = ap.parse_args()
    E.load_library()
    ctx = E.Context(0)
    out = {"device": []}
    ctx.matrix_nj(additive(64, 1))                                         # warm-up: module load, allocator
    floor = time_nj(ctx, additive(64, 2), max(args.repeats, 5))
    out["launch_floor_us_per_step"] = floor["us_per_step"]
    mats = {}
    for S in [int(x) for x in args.sizes.split(",") if x]:
        mats[S] = additive(S, S)
        out["device"].append(time_nj(ctx, mats[S], args.repeats))
        if S > 4000:
            del mats[S]
    if args.model_sizes:
        import nj_model as M
        out["numpy_model"] = []
        for S in [int(x) for x in args.model_sizes.split(",") if x]:
            D = mats[S] if S in mats else additive(S, S)
            t = time.perf_counter()
            M.nj(D)
            out["numpy_model"].append({"S": S, "total_s": time.perf_counter() - t})
    ctx.close()
    if args.cli_genomes:
        out["cli"] = cli_leg(args.cli_genomes, args.cli_genome_len)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
