"""Model of skx_array_sample_qc / skh_qc_text / skh_qc (`ska qc`): per-sample quality counts and outlier flags.  numpy only.

Definition (restated in include/skx.h).  The array holds S samples and U rows in its current order.  code(cell) is the 4-bit IUPAC set of
skx_array_group_markers (A 1, C 2, T 4, G 8; '-' and the 0 byte are 0).  A cell is present when its code != 0 and unambiguous when
popcount(code) == 1.  Per row r:

    n       = its present cells
    c[b]    = its cells that are exactly the unambiguous base b (b in A, C, T, G)
    unamb   = c[A] + c[C] + c[T] + c[G]
    major   = the base with the largest c[b], ties going to the lowest code (A < C < T < G); undefined when unamb == 0
    core    when n >= thr, thr = max(1, (uint64)ceil(S * min_freq)) computed in doubles exactly so (curve's rule at t = S)
    variant when at least two bases have c[b] > 0

Per sample s six counts over the rows; a cell of s counts into

    kmers            when it is present                                   (equals skx_array_sample_kmers)
    ambiguous        when it is present and popcount(code) >= 2
    singletons       when it is present and n == 1
    core_present     when it is present and the row is core
    private_alleles  when it is unambiguous with base b, c[b] == 1 and unamb >= 2   (another sample carries a different plain base there)
    minor_alleles    when it is unambiguous, the row is core and its base != major

For the whole array: rows = U, rows_present (n >= 1), core_rows, core_variant_rows (core and variant), threshold = thr.

The flag rule (restated in include/skx_host.h), in integers and one double product.  Six metrics per sample: kmers, ambiguous, singletons,
core_missing = core_rows - core_present (0 where a made-up core_present is the larger), private_alleles, minor_alleles.  For a metric with
values x[0..S): med = place (S - 1) // 2 of the sorted values, mad = the same place of the sorted |x - med|, d = max(mad, 1); a sample is high
when x > med and float(x - med) > M * float(d), and low symmetrically.  kmers is flagged on both sides (low_kmers, high_kmers), the other five
on the high side under their own names.  S = 1 has no flags (x = med); at S = 2 med is the smaller value and mad 0, so the larger one is high
once it is more than M above.

Texts.  <PREFIX>.qc.tsv: the header, then a line per sample in the array's order with its flags comma separated in the order of FLAGS, or "-".
<PREFIX>.qc.summary.tsv: samples, rows, rows_present, core_rows, core_variant_rows, threshold, each with its value; the line "metric min median
max mad flagged"; a line per metric.  <PREFIX>.qc.flagged.txt: the names with at least one flag, one per line, in the array's order."""
import math

import numpy as np

from subset_model import CODE

COUNTS = ("kmers", "ambiguous", "singletons", "core_present", "private_alleles", "minor_alleles")
INFO = ("rows", "rows_present", "core_rows", "core_variant_rows", "threshold")
METRICS = ("kmers", "ambiguous", "singletons", "core_missing", "private_alleles", "minor_alleles")
FLAGS = ("low_kmers", "high_kmers", "ambiguous", "singletons", "core_missing", "private_alleles", "minor_alleles")
SAMPLE_DT = np.dtype([(f, "<u8") for f in COUNTS])
INFO_DT = np.dtype([(f, "<u8") for f in INFO])
BASES = (1, 2, 4, 8)
_POP4 = np.array([bin(x).count("1") for x in range(16)], np.uint8)


def threshold(S, min_freq, rounding=math.ceil):
    return max(1, int(rounding(S * float(min_freq))))


def sample_qc(var, min_freq, rounding=math.ceil, ties_to_highest=False, private_ungated=False, ambiguous_are_bases=False):
    """var: [U, S] bytes -> (SAMPLE_DT [S], INFO_DT record).  The keyword arguments make the wrong variants the tests must catch: floor for
    ceil in the threshold, ties for major going to the highest code, private without the unamb >= 2 gate, and an ambiguous cell counted into
    c[b] of every base of its set."""
    var = np.asarray(var, np.uint8)
    U, S = var.shape
    code = CODE[var]
    assert not (code == 255).any(), "a byte outside the alphabet"
    thr = threshold(S, min_freq, rounding)
    present = code != 0
    plain = _POP4[code] == 1
    n = present.sum(axis=1)
    if ambiguous_are_bases:
        c = np.stack([((code & b) != 0).sum(axis=1) for b in BASES], axis=1)
    else:
        c = np.stack([(code == b).sum(axis=1) for b in BASES], axis=1)                      # [U, 4] in the order A, C, T, G
    unamb = c.sum(axis=1)
    if ties_to_highest:
        major_at = 3 - np.argmax(c[:, ::-1], axis=1) if U else np.zeros(0, np.int64)
    else:
        major_at = np.argmax(c, axis=1) if U else np.zeros(0, np.int64)                     # the first of the largest: the lowest code
    major = np.where(unamb > 0, np.array(BASES, np.uint8)[major_at], np.uint8(0))
    core = n >= thr
    variant = (c > 0).sum(axis=1) >= 2
    at = np.zeros((U, S), np.int64)                                                          # the place of a plain cell's base in c
    for j, b in enumerate(BASES):
        at[code == b] = j
    c_own = np.take_along_axis(c, at, axis=1) if U else np.zeros((0, S), np.int64)          # c[b] of the cell's own base (where it is plain)
    private = plain & (c_own == 1) & (True if private_ungated else (unamb >= 2)[:, None])
    minor = plain & core[:, None] & (code != major[:, None])
    out = np.zeros(S, SAMPLE_DT)
    out["kmers"] = present.sum(axis=0)
    out["ambiguous"] = (present & ~plain).sum(axis=0)
    out["singletons"] = (present & (n == 1)[:, None]).sum(axis=0)
    out["core_present"] = (present & core[:, None]).sum(axis=0)
    out["private_alleles"] = private.sum(axis=0)
    out["minor_alleles"] = minor.sum(axis=0)
    info = np.zeros(1, INFO_DT)[0]
    info["rows"], info["rows_present"], info["core_rows"], info["core_variant_rows"], info["threshold"] = U, int((n >= 1).sum()), int(core.sum()), int((core & variant).sum()), thr
    return out, info


def sample_qc_slow(var, min_freq):
    """the definition cell by cell -> ([S][6] as lists, [5] as a list) (the second restatement small inputs are held against)"""
    var = np.asarray(var, np.uint8)
    U, S = var.shape
    thr = max(1, int(math.ceil(S * float(min_freq))))
    counts = [[0] * 6 for _ in range(S)]
    info = [U, 0, 0, 0, thr]
    for row in var:
        codes = [int(CODE[x]) for x in row]
        n = sum(1 for x in codes if x != 0)
        c = {b: sum(1 for x in codes if x == b) for b in BASES}
        unamb = sum(c.values())
        major = None
        for b in BASES:
            if unamb and (major is None or c[b] > c[major]):
                major = b
        core = n >= thr
        variant = sum(1 for b in BASES if c[b] > 0) >= 2
        info[1] += n >= 1
        info[2] += core
        info[3] += core and variant
        for s, x in enumerate(codes):
            if x == 0:
                continue
            counts[s][0] += 1
            counts[s][1] += x not in BASES
            counts[s][2] += n == 1
            counts[s][3] += core
            if x in BASES:
                counts[s][4] += c[x] == 1 and unamb >= 2
                counts[s][5] += core and x != major
    return counts, info


def as_lists(samples, info):
    return [[int(r[f]) for f in COUNTS] for r in samples], [int(info[f]) for f in INFO]


# ---- the flag rule ----
def metric_values(samples, info):
    """-> {metric: [S] python ints}"""
    core_rows = int(info["core_rows"])
    out = {m: [int(x) for x in samples[m]] for m in METRICS if m != "core_missing"}
    out["core_missing"] = [max(0, core_rows - int(x)) for x in samples["core_present"]]
    return out


def outliers(x, M, both_sides):
    """x: python ints -> (per sample 'low' / 'high' / None, (min, med, max, mad))"""
    S = len(x)
    if S == 0:
        return [], (0, 0, 0, 0)
    v = sorted(x)
    med = v[(S - 1) // 2]
    mad = sorted(abs(y - med) for y in x)[(S - 1) // 2]
    bound = float(M) * float(max(mad, 1))
    side = []
    for y in x:
        if y > med and float(y - med) > bound:
            side.append("high")
        elif both_sides and y < med and float(med - y) > bound:
            side.append("low")
        else:
            side.append(None)
    return side, (v[0], med, v[-1], mad)


def flags(samples, info, M=5.0):
    """-> (per sample the list of its flags in the order of FLAGS, {metric: (min, med, max, mad, flagged)})"""
    values = metric_values(samples, info)
    S = len(samples)
    per_sample = [[] for _ in range(S)]
    stats = {}
    for m in METRICS:
        side, st = outliers(values[m], M, both_sides=m == "kmers")
        for s, w in enumerate(side):
            if w:
                per_sample[s].append({"low": "low_kmers", "high": "high_kmers"}[w] if m == "kmers" else m)
        stats[m] = st + (sum(1 for w in side if w),)
    assert all(f == sorted(f, key=FLAGS.index) for f in per_sample)
    return per_sample, stats


def texts(samples, names, info, M=5.0):
    """-> {file suffix: text} as `ska qc` writes them"""
    per_sample, stats = flags(samples, info, M)
    values = metric_values(samples, info)
    lines = ["sample\tkmers\tambiguous\tsingletons\tcore_present\tcore_missing\tprivate_alleles\tminor_alleles\tflags"]
    for s, name in enumerate(names):
        r = samples[s]
        f = [int(r["kmers"]), int(r["ambiguous"]), int(r["singletons"]), int(r["core_present"]), values["core_missing"][s], int(r["private_alleles"]), int(r["minor_alleles"])]
        lines.append("\t".join([name] + [str(x) for x in f] + [",".join(per_sample[s]) or "-"]))
    summary = [f"samples\t{len(names)}"] + [f"{k}\t{int(info[k])}" for k in INFO] + ["metric\tmin\tmedian\tmax\tmad\tflagged"]
    summary += ["\t".join([m] + [str(x) for x in stats[m]]) for m in METRICS]
    flagged = [name for s, name in enumerate(names) if per_sample[s]]
    return {".qc.tsv": "\n".join(lines) + "\n", ".qc.summary.tsv": "\n".join(summary) + "\n", ".qc.flagged.txt": "".join(n + "\n" for n in flagged)}


def texts_of(var, names, min_freq=0.9, M=5.0):
    samples, info = sample_qc(var, min_freq)
    return texts(samples, names, info, M)
