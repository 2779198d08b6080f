#!/usr/bin/env python3
"""Compare what two `ska` executables answer to a generated corpus of command lines that need no device:

    tools/cli_refusal_diff.py OLD/ska NEW/ska

Every line is run by both in an empty directory of its own, on an input that does not exist, and (exit code, stdout, stderr with the
log lines' timestamps masked, directory listing) is compared.  Lines that are accepted end at the missing device or the missing file the
same way in both and stay in the comparison; where `--gpus N` was accepted, N ranks write to one stderr and the first to fail ends the
others, so there the distinct stderr lines are compared, in sorted order.  Prints the lines that differ, then the two counts; exit code 1 if any differ."""
import itertools
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

# every option of `ska distance`: a good value, then the empty value and bad ones (None: the option takes no value)
DISTANCE = {
    "-o": ["t.tsv", ""], "--min-freq": ["0.5", "", "x", "2"], "-m": ["0.5", "", "-1"], "--allow-ambiguous": None, "--threads": ["1", "", "0", "x"],
    "--gpus": ["2", "", "0"], "--tree": ["t.nwk", ""], "--clusters": ["c", ""], "--cluster-snps": ["5", "", "x", "-1", "nan"],
    "--cluster-mismatches": ["0.5", "", "x", "-1"], "--query": ["a,b", "", ","], "--query-file": ["q.txt", ""], "--query-skf": ["b.skf", ""],
    "--max-snps": ["5", "", "x", "-1", "nan", "inf", "+1e3"], "--max-mismatches": ["0.5", "", "x", "1.5", "nan"],
    "--closest": ["2", "", "x", "0", "+3", "+", "-1", "99999999999999999999"], "--no-table": None, "--mst": None, "--mst-clusters": ["lad", ""],
    "--levels": ["10,5,0", "", "5,,1", "x", "5,5", "-1", ",".join(str(n) for n in range(17))], "--sites": ["p", ""],
    "--sites-max": ["10", "", "x", "0", "+7", "1.5", "99999999999999999999", "18446744073709551615"]}
SELECTING = [["--max-snps", "5"], ["--max-mismatches", "0.5"], ["--closest", "2"], ["--mst"]]
# the conflict and value checks of the other subcommands that share the helpers
OTHERS = [["align", "x.skf", "--groups", "g.csv", "--gpus", "2"], ["align", "x.skf", "--min-group-size", "2", "--gpus", "2"], ["align", "x.skf", "--samples", "a", "--gpus", "2"],
          ["align", "x.skf", "--samples-file", "s.txt", "--gpus", "2"], ["align", "x.skf", "--groups", "g.csv", "--samples", "a"],
          ["align", "x.skf", "--groups", "g.csv", "--samples-file", "s.txt"], ["align", "x.skf", "--samples", "a", "--samples-file", "s.txt"],
          ["align", "x.skf", "--samples-file", "s.txt", "--samples", "a", "--groups", "g.csv", "-o", "p"], ["align", "x.skf", "--min-group-size", "2"],
          ["align", "x.skf", "--groups", "g.csv"], ["align", "x.skf", "--groups", "", "-o", "p"], ["align", "x.skf", "--samples", ""], ["align", "x.skf", "--samples", ","],
          ["align", "a.fa", "b.fa", "--gpus", "2", "-f", "l.txt"], ["align", "--gpus", "2"], ["align", "a.fa", "b.fa", "--gpus", "2", "-k", "30"], ["align"], ["align", "x.skf", "--min-freq", "2"],
          ["build", "a.fa", "-f", "l.txt", "-o", "out"], ["build", "a.fa", "-f", "l.txt"], ["build", "-o", "out"], ["build", "a.fa", "-o", "out", "-k", "x"],
          ["build", "a.fa", "-o", "out", "-k", "32"], ["build", "a.fa", "-o", "out", "--min-count", "0"], ["build", "a.fa", "-o", "out", "--gpus", "2", "-f", "l.txt"],
          ["build", "a.fa", "b.fa", "-o", "out"], ["delete", "-s", "x.skf", "a", "-f", "l.txt"], ["delete", "-s", "x.skf"], ["delete", "a"],
          ["markers", "x.skf", "--groups", "g.csv", "-o", "p", "--gpus", "2"], ["markers", "x.skf", "--groups", "g.csv", "-o", "p"], ["markers", "x.skf", "--groups", "g.csv"],
          ["markers", "x.skf", "-o", "p"], ["markers", "x.skf", "y.skf", "--groups", "g.csv", "-o", "p"], ["markers", "x.skf", "--groups", "", "-o", "p"],
          ["cov", "a.fq", "b.fq", "-k", "4"], ["weed", "x.skf", "--min-freq", "x"], ["lo", "x.skf", "out", "-m", "x"], ["lo", "x.skf", "out", "-d", "x"], ["lo", "x.skf"]]
OTHERS += [["align", "x.skf", "--groups", "g.csv", "-o", "p", "--min-group-size", v] for v in ("", "x", "0", "+2", "+", "3")]
OTHERS += [["markers", "x.skf", "--groups", "g.csv", "-o", "p", "--min-group-size", v] for v in ("", "x", "0", "+2", "3")]
OTHERS += [["markers", "x.skf", "--groups", "g.csv", "-o", "p", o, v] for o in ("--min-in", "--max-out") for v in ("", "x", "-0.1", "1.5", "nan", "0.5")]


def corpus():
    def use(opt, value=None):
        vals = DISTANCE[opt]
        return [opt] if vals is None else [opt, vals[0] if value is None else value]

    tails = [[]]
    for opt, vals in DISTANCE.items():
        tails.append(use(opt))
        tails.append(use(opt) + ["-v"])
        tails += [use(opt, v) for v in (vals or [])[1:]]
        tails += [s + use(opt, v) for s in SELECTING for v in (vals or [])[1:] if opt in ("--sites", "--sites-max", "--mst-clusters", "--levels")]
    tails += [use(x) + use(y) for x, y in itertools.permutations(DISTANCE, 2)]
    # the triples the tests name
    tails += [["--mst", "--closest", "2", "--query", "a"], ["--query", "a", "--closest", "2", "--mst"], ["--mst", "--mst-clusters", "lad", "--sites", "p"]]
    refused = ["--allow-ambiguous", "--no-table", "--query", "--query-file", "--query-skf", "--gpus", "--mst-clusters", "--tree", "--clusters", "-o"]
    for s in SELECTING:
        tails += [s + ["--sites", "p"], s + ["--sites", "p", "--sites-max", "10"], s + ["--sites-max", "10"], ["--sites", "p", "--sites-max", "+7"] + s]
        tails += [order for o in refused for order in (s + ["--sites", "p"] + use(o), use(o) + ["--sites", "p"] + s, ["--sites", "p", "--sites-max", "10"] + use(o) + s)]
    for lv in DISTANCE["--levels"]:
        tails += [["--mst", "--levels", lv], ["--mst", "--mst-clusters", "lad", "--levels", lv], ["--mst-clusters", "lad", "--levels", lv], ["--levels", lv, "--max-snps", "5"]]
    lines = [["distance", "x.skf"] + t for t in tails]
    lines += [ln + ["--gpus", "2"] for ln in lines if "--gpus" not in ln]
    lines += [["distance"] + t for t in ([], ["--mst"], ["--gpus", "2"], ["--gpus", "2", "-f", "l.txt"], ["--gpus", "2", "-f", "l.txt", "--max-snps", "5"])]
    lines += [["distance", "a.fa", "b.fa"] + t for t in ([], ["--gpus", "2"], ["--gpus", "2", "-f", "l.txt"], ["--gpus", "2", "-k", "30"], ["--gpus", "2", "--tree", ""], ["--gpus", "2", "--cluster-snps", "5"])]
    return lines + OTHERS


STAMP = re.compile(rb"^\d{4}-\d\d-\d\dT\d\d:\d\d:\d\d\.\d{3}Z ", re.M)


def answer(exe, line):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SKX_")}
    with tempfile.TemporaryDirectory() as wd:
        r = subprocess.run([exe] + line, cwd=wd, env=env, capture_output=True, timeout=120)
        err = STAMP.sub(b"<time> ", r.stderr)
        if "--gpus" in line and r.returncode != 2:
            err = b"".join(sorted(set(err.splitlines(True))))
        return r.returncode, r.stdout, err, sorted(os.listdir(wd))


def main():
    old, new = (os.path.abspath(p) for p in sys.argv[1:3])
    lines = corpus()
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        got = list(pool.map(lambda ln: (answer(old, ln), answer(new, ln)), lines))
    differ = 0
    for ln, (a, b) in zip(lines, got):
        if a != b:
            differ += 1
            print("DIFFERS: ska " + " ".join(repr(x) if x == "" else x for x in ln), "  old: %r" % (a,), "  new: %r" % (b,), sep="\n")
    codes = {}
    for a, _ in got:
        codes[a[0]] = codes.get(a[0], 0) + 1
    print("exit codes of the first executable: " + ", ".join("%d x %d" % (n, c) for c, n in sorted(codes.items())))
    print("command lines compared: %d\ncommand lines that differ: %d" % (len(lines), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
