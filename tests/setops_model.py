"""Model of the .skf life-cycle -- `ska merge`, `ska delete`, `ska weed` -- restated from the reference on plain rows, plus the fixed case
list the CPU and the GPU suites share (tests/test_setops_model.py pins the model to the oracle, tests/test_gpu_setops_edges.py holds the
engine to both).

An array is Arr(k, rc, names, keys, var[U, S], counts[U]); keys are Python ints (lo | hi << 64) or a KEY_DT array on the way in, Python
ints on the way out.  Every function returns its rows sorted by key.  The model functions use numpy and Python ints only; the case
builders further down ask the oracle for canonical split k-mers (ora.extract_record / ora.Dict, pinned by the golden tests)."""
import collections
import functools
import itertools
import os

import numpy as np

KEY_DT = np.dtype([("lo", "<u8"), ("hi", "<u8")])
GAP = ord("-")
FILTER_NAMES = ("no-filter", "no-const", "no-ambig", "no-ambig-or-const")
Arr = collections.namedtuple("Arr", "k rc names keys var counts")
_M64 = (1 << 64) - 1


class Refused(Exception):
    """where the reference panics; the text is the panic's"""


def ints(keys):
    if isinstance(keys, np.ndarray) and keys.dtype == KEY_DT:
        return [int(lo) | (int(hi) << 64) for lo, hi in zip(keys["lo"].tolist(), keys["hi"].tolist())]
    return [int(x) for x in keys]


def key_dt(keys):
    out = np.zeros(len(keys), KEY_DT)
    out["lo"] = np.array([x & _M64 for x in keys], np.uint64) if len(keys) else np.zeros(0, np.uint64)
    out["hi"] = np.array([x >> 64 for x in keys], np.uint64) if len(keys) else np.zeros(0, np.uint64)
    return out


def present(var):
    """MergeSkaArray::new's variant_count (merge_ska_array.rs:172): cells that are neither 0 nor '-'"""
    var = np.asarray(var, np.uint8)
    return ((var != GAP) & (var != 0)).sum(axis=1).astype(np.int64)


def arr(k, rc, names, keys, var, counts=None):
    keys = ints(keys)
    var = np.asarray(var, np.uint8).reshape(len(keys), len(names)).copy()
    var[var == 0] = GAP                                                     # :175
    counts = present(var) if counts is None else np.asarray(counts, np.int64).copy()
    return Arr(int(k), bool(rc), list(names), keys, var, counts)


def by_key(a):
    order = sorted(range(len(a.keys)), key=a.keys.__getitem__)
    return Arr(a.k, a.rc, list(a.names), [a.keys[i] for i in order], a.var[order], a.counts[order])


def _rows(a, keep):
    keep = np.asarray(keep, bool)
    return Arr(a.k, a.rc, list(a.names), [key for key, f in zip(a.keys, keep.tolist()) if f], a.var[keep], a.counts[keep])


def is_ambiguous(var):
    """bit_encoding.rs:58-61 on a byte array: anything but ACGTU- in either case"""
    low = np.asarray(var, np.uint8) | 0x20
    return ~np.isin(low, np.frombuffer(b"acgtu-", np.uint8))


# ---- ska merge: to_dict (merge_ska_array.rs:209-221) + MergeSkaDict::extend (merge_ska_dict.rs:160-193) + MergeSkaArray::new (:166-186)
def merge(arrays, drop_empty_rows=False):
    first = arrays[0]
    for a in arrays[1:]:
        if a.k != first.k:
            raise Refused(f"K-mer lengths do not match: {a.k} {first.k}")
        if a.rc != first.rc:
            raise Refused("Strand use inconsistent")
    keys = sorted(set().union(*[a.keys for a in arrays]))                   # rows = the distinct split k-mers over all inputs
    row = {key: i for i, key in enumerate(keys)}
    names = [n for a in arrays for n in a.names]                            # :169, duplicates allowed
    var = np.full((len(keys), len(names)), GAP, np.uint8)                   # absent = 0 -> '-' (:175)
    c0 = 0
    for a in arrays:
        if len(a.keys):
            var[[row[key] for key in a.keys], c0:c0 + len(a.names)] = a.var
        c0 += len(a.names)
    out = Arr(first.k, first.rc, names, keys, var, present(var))            # counts recomputed (:172); rows without any cell stay
    if drop_empty_rows:                                                     # (the wrong variant the mutation check uses)
        out = _rows(out, out.counts > 0)
    return out


# ---- update_counts(false) (merge_ska_array.rs:139-163)
def _update_counts(a, filter_ambig_as_missing):
    ok = a.var != GAP
    if filter_ambig_as_missing:
        ok &= ~is_ambiguous(a.var)
    counts = ok.sum(axis=1).astype(np.int64)
    return _rows(Arr(a.k, a.rc, a.names, a.keys, a.var, counts), counts > 0)


# ---- ska delete: MergeSkaArray::delete_samples (merge_ska_array.rs:231-271)
def delete_samples(a, del_names, last_duplicate=False, carry_counts=False):
    if len(del_names) == 0 or len(del_names) == len(a.names):               # :232 on the raw list
        raise Refused("Invalid number of samples to remove")
    want = set(del_names)                                                   # :237-240
    drop = []
    cols = range(len(a.names) - 1, -1, -1) if last_duplicate else range(len(a.names))      # (last_duplicate: a wrong variant)
    for idx in cols:
        if a.names[idx] in want:                                            # :244-246: the first column of a name goes, later ones stay
            drop.append(idx)
            want.remove(a.names[idx])
    if want:
        raise Refused("Could not find sample(s): {" + ", ".join('"%s"' % n for n in sorted(want)) + "}")
    keep = [i for i in range(len(a.names)) if i not in drop]
    out = Arr(a.k, a.rc, [a.names[i] for i in keep], list(a.keys), a.var[:, keep], a.counts)
    if carry_counts:                                                        # (a wrong variant: stored counts decide which rows stay)
        return by_key(_rows(out, out.counts > 0))
    return by_key(_update_counts(out, False))                               # :270


# ---- MergeSkaArray::weed (merge_ska_array.rs:452-487): kept rows carry their stored counts
def weed_keys(a, keyset, reverse=False, recount=False):
    ks = set(ints(keyset))
    found = np.array([key in ks for key in a.keys], bool)
    keep = found if reverse else ~found                                     # :467
    out = _rows(a, keep)
    if recount:                                                             # (a wrong variant)
        out = Arr(out.k, out.rc, out.names, out.keys, out.var, present(out.var))
    return by_key(out), int(len(a.keys) - keep.sum())


# ---- MergeSkaArray::filter (merge_ska_array.rs:289-402) with update_kmers = true
def filter_rows(a, min_count, filter_ambig_as_missing, filter_type, mask_ambig, ignore_const_gaps):
    if filter_ambig_as_missing:
        a = _update_counts(a, True)                                         # :308-310
    keep = np.zeros(len(a.keys), bool)
    for r in range(len(a.keys)):
        if a.counts[r] < min_count:                                         # :319
            continue
        row = a.var[r].tolist()
        if filter_type == 0:
            keep[r] = True
        elif filter_type == 1:                                              # NoConst :322-333
            keep[r] = len({b for b in row if not ignore_const_gaps or b != GAP}) > 1
        elif filter_type == 2:                                              # NoAmbig :334-343
            keep[r] = not is_ambiguous(a.var[r]).any()
        else:                                                               # NoAmbigOrConst :344-365
            n = 0
            for b in set(row):
                low = b | 0x20
                if low in b"acgtu":
                    n += 1
                elif low == GAP:
                    n += 0 if ignore_const_gaps else 1
            keep[r] = n > 1
    out = _rows(a, keep)
    if mask_ambig:                                                          # :388-399
        var = out.var.copy()
        var[is_ambiguous(var)] = ord("N")
        out = Arr(out.k, out.rc, out.names, out.keys, var, out.counts)
    return out, int(len(a.keys) - keep.sum())


# ---- ska weed: generic_modes::weed (generic_modes.rs:214-266)
def weed(a, keyset, reverse=False, min_freq=0.9, filter_ambig_as_missing=False, filter_type=0, ambig_mask=False, ignore_const_gaps=False,
         ceil_threshold=False, recount=False):
    if keyset is not None:
        a, _ = weed_keys(a, keyset, reverse, recount=recount)
    x = len(a.names) * min_freq                                             # the same IEEE product as `nsamples() as f64 * min_freq`
    threshold = int(np.ceil(x)) if ceil_threshold else int(np.floor(x))     # :249 (ceil: a wrong variant)
    if threshold > 0 or filter_type != 0 or ambig_mask or ignore_const_gaps:           # :250
        a, _ = filter_rows(a, threshold, filter_ambig_as_missing, filter_type, ambig_mask, ignore_const_gaps)
    return by_key(a)


# ---- `ska nk [--full-info]` (Display + Debug, merge_ska_array.rs:649-698) from the `k=` line on: the version line is the writer's, not the rows'
def decode_arm(bits, half):
    return "".join("ACTG"[(bits >> (2 * (half - 1 - i))) & 3] for i in range(half))


def kmer_text(key, k, middle="A"):
    """the k bases whose split k-mer on the forward strand is `key`"""
    half = (k - 1) // 2
    return decode_arm(key >> (2 * half), half) + middle + decode_arm(key & ((1 << (2 * half)) - 1), half)


def nk(a, full_info=False):
    half = (a.k - 1) // 2
    head = [f"k={a.k}", f"k_bits={64 if a.k <= 31 else 128}", f"rc={'true' if a.rc else 'false'}", f"k-mers={len(a.keys)}", f"samples={len(a.names)}",
            "sample_names=[" + ", ".join('"%s"' % n for n in a.names) + "]",
            "sample_kmers=[" + ", ".join(str(int(x)) for x in (a.var != GAP).sum(axis=0)) + "]", ""]
    if full_info:
        for key, row in zip(a.keys, a.var):
            head.append(decode_arm(key >> (2 * half), half) + "\t" + decode_arm(key & ((1 << (2 * half)) - 1), half) + "\t" + ",".join(chr(b) for b in row))
        head.append("")
    return "\n".join(head) + "\n"


def nk_lines(text):
    """an nk text (bytes or str) without its ska_version line"""
    text = text.decode() if isinstance(text, bytes) else text
    assert text.startswith("ska_version=")
    return text.split("\n", 1)[1]


def same(a, b):
    """None when two arrays hold the same names and rows (compared by key), else what differs first"""
    a, b = by_key(a), by_key(b)
    if (a.k, a.rc) != (b.k, b.rc):
        return f"k/rc {(a.k, a.rc)} != {(b.k, b.rc)}"
    if a.names != b.names:
        return f"names {a.names} != {b.names}"
    if a.keys != b.keys:
        return f"keys differ: {len(a.keys)} vs {len(b.keys)} rows, first only-left {sorted(set(a.keys) - set(b.keys))[:2]}, only-right {sorted(set(b.keys) - set(a.keys))[:2]}"
    if a.var.shape != b.var.shape or not np.array_equal(a.var, b.var):
        r = int(np.argwhere((a.var != b.var).any(axis=1))[0][0])
        return f"cells differ first in row {r} (key {a.keys[r]}): {a.var[r].tobytes()} != {b.var[r].tobytes()}"
    if not np.array_equal(np.asarray(a.counts, np.int64), np.asarray(b.counts, np.int64)):
        r = int(np.argwhere(np.asarray(a.counts, np.int64) != np.asarray(b.counts, np.int64))[0][0])
        return f"counts differ first in row {r}: {a.counts[r]} != {b.counts[r]}"
    return None


# ======================================================================================================================== options
class Opts(tuple):
    """(min_freq, filter_ambig_as_missing, filter_type, ambig_mask, ignore_const_gaps) of `ska weed`"""
    min_freq = property(lambda s: s[0])
    filter_ambig_as_missing = property(lambda s: s[1])
    filter_type = property(lambda s: s[2])
    ambig_mask = property(lambda s: s[3])
    ignore_const_gaps = property(lambda s: s[4])

    def kw(self):
        return dict(min_freq=self[0], filter_ambig_as_missing=self[1], filter_type=self[2], ambig_mask=self[3], ignore_const_gaps=self[4])

    def ident(self):
        return f"mf{self[0]}-{FILTER_NAMES[self[2]]}" + ("-ambigmissing" if self[1] else "") + ("-mask" if self[3] else "") + ("-nogaponly" if self[4] else "")


NO_FILTER = Opts((0.0, False, 0, False, False))                             # threshold 0, nothing asked for: the filter step does not run
DEFAULTS = Opts((0.9, False, 0, False, False))                              # `ska weed x.skf` with nothing else
ALL_OPTS = [Opts(o) for o in itertools.product((0.0, 0.5, 0.9, 1.0), (False, True), (0, 1, 2, 3), (False, True), (False, True))]


def option_grid(n=10, seed=20261018):
    """n of the 128 combinations drawn with a fixed seed, redrawn (next seed) until every filter type, both values of each flag and each
    min_freq are among them (the way subset_model.option_grid samples its own)"""
    while True:
        rng = np.random.default_rng(seed)
        pick = [ALL_OPTS[i] for i in rng.permutation(len(ALL_OPTS))[:n]]
        if all(len({o[f] for o in pick}) == w for f, w in ((0, 4), (1, 2), (2, 4), (3, 2), (4, 2))):
            return pick
        seed += 1


GRID = option_grid()

# ========================================================================================================================== cases
# the cells of tests/test_gpu_stream_load.py::_random_array: '-' and ACGT weighted, then every ambiguity code
ALPHA = np.frombuffer(b"ACGT-ACGTACGT-MRWSYKVHDBN", dtype=np.uint8)
CODES = b"-ACGTMRWSYKVHDBN"
# pitch_for (csrc/skx_internal.h) rounds a row count up to a multiple of 256 and adds 256: the matrix pitch changes at every multiple
# of 256 rows, so 255 / 256 / 257 and 511 / 512 / 513 sit just below, at and above the granule; the look-up, flag and scatter kernels
# run 256 rows a block, the same edges.
GRANULE = 256


def random_cells(rng, U, S):
    """constant, variant, gappy and full-IUPAC rows, rows no sample has, and (from 16 samples on, else spread over rows) the whole code set"""
    var = np.empty((U, S), np.uint8)
    if not U:
        return var
    kind = rng.integers(0, 5, size=U)
    var[:] = ALPHA[rng.integers(0, 4, size=U)][:, None]
    mixed = kind >= 2
    var[mixed] = ALPHA[rng.integers(0, 13, size=(int(mixed.sum()), S))]
    amb = kind == 4
    var[amb] = ALPHA[rng.integers(0, len(ALPHA), size=(int(amb.sum()), S))]
    gappy = kind == 1
    g = var[gappy]
    g[rng.random(g.shape) < 0.6] = GAP
    var[gappy] = g
    var[rng.integers(0, U, size=max(1, U // 50))] = GAP
    full = np.frombuffer(CODES, np.uint8)
    for j in range(min(U, 2)):                                             # rows 0 and 1: the 16 codes in turn, from two offsets
        var[j] = full[(np.arange(S) + 5 * j + int(rng.integers(0, 16))) % 16]
    return var


def _canonical(texts, k, rc):
    """the split k-mer key of each k-base text as the reference stores it"""
    import ora
    out = []
    for t in texts:                                                          # (a record needs more than k bases to yield a window, split_kmer.rs:89)
        keys = ints(ora.extract_record((t + "A").encode(), k, rc)[0])
        assert len(keys) == 2, (t, keys)
        out.append(keys[0])
    return out


def key_pool(rng, n, k, rc):
    """n distinct canonical split k-mers in random order.  k = 5: as many of the 256 (rc: fewer) as there are.  k > 31: among them keys with
    hi == 0, pairs that differ only in lo and pairs that differ only in hi (guaranteed without rc, where a key is its text's own)"""
    import ora
    half = (k - 1) // 2
    special = []
    if k > 31 and n >= 8:
        base = "".join("ACGT"[i] for i in rng.integers(0, 4, size=k))
        flip = lambda s, p: s[:p] + "ACGT"[("ACGT".index(s[p]) + 1) % 4] + s[p + 1:]
        lead = "A" * (k - 33 + 1) + base[k - 33 + 1:]                       # 2 (k - 1) - 64 leading zero bits: hi == 0
        special = _canonical([base, flip(base, k - 1), flip(base, 0), lead, flip(lead, k - 2)], k, rc)
    seq = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(4000 if k == 5 else (3 * n if k < 15 else n + n // 8) + k + 8))])
    keys = ints(ora.extract_record(seq, k, rc)[0])
    pool = list(dict.fromkeys(special + keys))
    head, tail = pool[:len(special)], pool[len(special):]
    tail = [tail[i] for i in rng.permutation(len(tail))]
    pool = (head + tail)[:n]
    assert len(pool) == n or k == 5, (k, n, len(pool))
    return [pool[i] for i in rng.permutation(len(pool))]


def _names(sizes, dup=False):
    out = [[f"i{j}s{s}" for s in range(S)] for j, S in enumerate(sizes)]
    if dup and len(out) > 1:                                                # the same name in two inputs (and so twice in the merged array)
        out[-1][0] = out[0][0]
    return out


def matrix_case(name, k, rc, sizes, ranges, seed, dup=False, equal=None, stored=None, extra_opts=(), grid=True, heavy=None):
    """inputs j = rows pool[ranges[j][0]:ranges[j][1]] x sizes[j] samples.  equal=(a, b): input b holds input a's cells (sizes equal);
    stored=j: input j's stored counts differ from its rows; heavy=(j, s): every row of input j has a base in sample s, the others are sparse"""
    rng = np.random.default_rng(seed)
    pool = key_pool(rng, max(hi for _, hi in ranges), k, rc)
    names = _names(sizes, dup)
    inputs = []
    for j, (S, (lo, hi)) in enumerate(zip(sizes, ranges)):
        hi = min(hi, len(pool))
        keys = [pool[i] for i in range(lo, hi)]
        keys = [keys[i] for i in rng.permutation(len(keys))]               # file order, not key order
        var = random_cells(rng, len(keys), S)
        if heavy and heavy[0] == j:
            sparse = rng.random(var.shape) < 0.9
            sparse[:, heavy[1]] = False
            var[sparse] = GAP
            var[:, heavy[1]] = ALPHA[rng.integers(0, 4, size=len(keys))]
        counts = None
        if stored == j:
            counts = present(var) + rng.integers(-1, 3, size=len(keys))     # too low, right, too high; 0 and below among them
            counts = np.maximum(counts, 0)
        inputs.append(arr(k, rc, names[j], keys, var, counts))
    if equal:
        a, b = equal
        inputs[b] = Arr(k, rc, names[b], list(inputs[a].keys), inputs[a].var.copy(), inputs[a].counts.copy())
    return dict(name=name, k=k, rc=rc, inputs=inputs, records=None, extra_opts=[Opts(o) for o in extra_opts], grid=grid, seed=seed,
                stored=stored, heavy=names[heavy[0]][heavy[1]] if heavy else None)


def deletions(case):
    """(label, request) pairs: first column, last column, all but one, a whole input's samples, the heavy / duplicated names, a repeated name"""
    inputs = case["inputs"]
    names = [n for a in inputs for n in a.names]
    out = []
    if len(names) >= 2:
        out += [("first", [names[0]]), ("last", [names[-1]])]
    if len(names) >= 3:
        keep = len(names) // 2
        out.append(("all-but-one", list(dict.fromkeys(n for n in names if n != names[keep]))))     # (a duplicated name loses its first column only)
        out.append(("repeated-name", [names[1], names[1]]))
    if len(inputs) >= 2 and len(set(names)) == len(names):
        big = max(range(len(inputs)), key=lambda j: len(inputs[j].keys))
        out.append((f"whole-input-{big}", list(inputs[big].names)))
        rest = [n for j, a in enumerate(inputs) if j != 0 for n in a.names]
        if len(rest) < len(names) and rest != out[-1][1]:
            out.append(("all-but-input-0", rest))
    if case.get("heavy"):
        out.append(("heavy-sample", [case["heavy"]]))
    if len(set(names)) != len(names):
        d = next(n for n in names if names.count(n) > 1)
        out.append(("duplicate-name", [d]))
    return [(lab, req) for lab, req in out if 0 < len(req) and len(req) != len(names)]


def key_records(keys, k):
    """one record per key: its k bases (the middle one taken in turn from ACGT: the weed ignores it) and one base more, because a record of
    exactly k bases yields no window (split_kmer.rs:89).  The extra base brings a second split k-mer along -- foreign to the array with
    near certainty from k = 15 on, anybody's at k = 5 -- so a set's keys are what its records hold (records_keys), not what was asked for."""
    return [(kmer_text(key, k, "ACGT"[i % 4]) + "ACGT"[(i // 4) % 4]).encode() for i, key in enumerate(keys)]


def weed_sets(case, merged):
    """label -> (records, keys) of the weed sets of a case: no row, every row, exactly one row, a strict subset with foreign keys beside it;
    for a sequence case first of all its own FASTA records"""
    rng = np.random.default_rng(case["seed"] + 7)
    k, rc = case["k"], case["rc"]
    have = set(merged.keys)
    foreign = [x for x in key_pool(rng, 24 if k > 5 else 256, k, rc) if x not in have][:12]
    out = {}
    if case.get("weed_records"):
        out["fasta"] = case["weed_records"]
    if foreign:
        out["no-row"] = key_records(foreign, k)
    if merged.keys:                                                         # (a FASTA file without records is no weed file: needletail refuses it)
        out["every-row"] = key_records(merged.keys, k)
        out["one-row"] = key_records([merged.keys[len(merged.keys) // 2]] + foreign[:3], k)
        out["subset"] = key_records(merged.keys[::3] + foreign[:5], k)
    return {lab: (recs, records_keys(recs, k, rc)) for lab, recs in out.items()}


def write_fasta(records, path):
    with open(path, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">w%d some description\n" % i + r + b"\n")
    return path


def weed_plan(case, merged):
    """the weed runs of a case: every set in both directions without a filter, then the sampled options, each on the next set in turn
    (None = no weed file)"""
    sets = weed_sets(case, merged)
    plan = [(lab, rev, NO_FILTER) for lab in sets for rev in (False, True)]
    labels = [None] + list(sets)
    opts = list(case["extra_opts"]) + (GRID if case["grid"] else [])
    plan += [(labels[i % len(labels)], bool((i // len(labels)) & 1), o) for i, o in enumerate(opts)]
    return sets, plan


# ---- sequence cases: related samples as records, inputs built from them, a weed FASTA with awkward records
def _mutated(rng, anc, n):
    s = bytearray(anc)
    for p in rng.integers(0, len(s), size=n):
        s[p] = b"ACGT"[(b"ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def sequence_case(name, k, rc, split, seed, length=1500):
    """len(split) inputs of split[j] samples each, all derived from one ancestor (so the inputs share most rows); sample 1 carries a stretch
    with ambiguity codes, the last sample is half as long (rows only the others have)"""
    import ora
    rng = np.random.default_rng(seed)
    anc = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=length)])
    records, inputs, n = [], [], 0
    for j, S in enumerate(split):
        recs, dicts = [], []
        for s in range(S):
            seq = _mutated(rng, anc, 12)
            if n == 1:
                seq = seq[:300] + b"R" + seq[301:700] + b"N" + seq[701:]
            if n == sum(split) - 1:
                seq = seq[: length // 2]
            two = [seq[: len(seq) // 2 + k], seq[len(seq) // 2:]]         # two records with a shared stretch: repeats inside a sample
            recs.append(two)
            d = ora.Dict.new(k, rc)
            for r in two:
                d.add_record(r)
            dicts.append(d)
            n += 1
        names = [f"q{j}s{s}" for s in range(S)]
        keys, var, counts = ora.Array.from_dicts(dicts, names).export()
        records.append(recs)
        inputs.append(arr(k, rc, names, keys, var, counts))
    foreign = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=200)])
    weed_records = [anc[200:200 + k - 1],                                   # shorter than k: no split k-mer
                    anc[100:400], anc[900:1000] + b"NN" + anc[1002:1100].lower(),         # N and lower case
                    anc[150:350].translate(_COMP)[::-1],                    # the reverse complement of a stretch already there
                    foreign]
    return dict(name=name, k=k, rc=rc, inputs=inputs, records=records, weed_records=weed_records, extra_opts=[DEFAULTS], grid=False, seed=seed)


def records_keys(records, k, rc):
    """the same from the records themselves"""
    import ora
    d = ora.Dict.new(k, rc, ora.qual(1, 0, ora.QUAL_NOFILTER))
    for r in records:
        d.add_record(r)
    return ints(d.export()[0])


def fasta_keys(path, k, rc):
    """the split k-mers RefSka::new + kmer_iter take from a FASTA file = the keys of its dictionary (ora.Dict, pinned by the golden tests)"""
    import ora
    return ints(ora.Dict.from_files(k, path, rc=rc, q=ora.qual(1, 0, ora.QUAL_NOFILTER)).export()[0])


_MATRIX = {
    # name: (k, rc, samples per input, pool ranges per input, keyword arguments)
    # two inputs, nested rows, 257 / 255 rows around the 256-row granule; min_freq 0.6 on 5 + ... samples
    "k31-nested-257-255": (31, True, (5, 2), ((0, 257), (1, 256)), dict(extra_opts=[(0.6, False, 0, False, False)])),
    # three inputs in a chain (each shares rows only with its neighbour), 256 / 1 / 300 rows; S = 10 with 0.3: exactly 3.0
    "k15-chain-256-1-300": (15, False, (3, 2, 5), ((0, 256), (255, 256), (255, 555)), dict(extra_opts=[(0.3, False, 0, False, False), (0.3, True, 1, False, True)])),
    # six inputs over the 256 keys of k = 5: one without rows, two equal ones, the key space exhausted by the weed set
    "k5-six-inputs": (5, True, (1, 2, 1, 5, 2, 1), ((0, 100), (0, 256), (0, 0), (60, 256), (0, 256), (10, 11)), dict(equal=(1, 4))),
    "k5-norc-identical": (5, False, (2, 2), ((0, 256), (0, 256)), dict(dup=True, grid=False)),
    # 63 + 65 and 64 + 65 + 1 samples: 128 and 130 columns, the scatter's grid.y and the 64-sample words of the statistics
    "k31-norc-63-65": (31, False, (63, 65), ((0, 300), (200, 513)), dict(grid=False, extra_opts=[(0.5, True, 3, True, False)])),
    "k15-64-65-1": (15, True, (64, 65, 1), ((0, 120), (100, 200), (0, 511)), {}),
    # 128-bit keys: disjoint inputs; chains; six inputs; duplicate names
    "k33-disjoint": (33, True, (2, 1), ((0, 255), (255, 512)), {}),
    "k33-norc-chain": (33, False, (1, 64, 2), ((0, 200), (150, 400), (350, 512)), dict(dup=True)),
    "k41-six-inputs": (41, True, (1, 2, 5, 1, 2, 1), ((0, 300), (290, 513), (100, 101), (0, 300), (0, 0), (500, 600)), dict(equal=(0, 3))),
    "k41-norc-nested": (41, False, (5, 5), ((0, 600), (100, 355)), dict(stored=0, extra_opts=[(0.3, False, 0, False, False), (0.9, False, 0, False, False)], grid=False)),
    "k63-identical": (63, True, (2, 3), ((0, 257), (0, 257)), {}),
    "k63-norc-disjoint-empty": (63, False, (1, 1, 63), ((0, 130), (0, 0), (130, 260)), dict(grid=False)),
    # stored counts that differ from the rows: weed carries them (and its filter reads them), merge and delete recount
    "k31-stored-counts": (31, True, (5,), ((0, 300),), dict(stored=0, extra_opts=[(0.6, False, 0, False, False), (0.6, True, 1, False, False), (1.0, False, 0, False, False)])),
    "k31-stored-counts-merge": (31, True, (5, 5), ((0, 300), (100, 400)), dict(stored=1, grid=False, extra_opts=[(0.3, False, 0, False, False), (0.5, False, 2, False, False)])),
    # 50 samples: 50 * 0.58 = 28.999999999999996 (floor 28, not 29) and 50 * 0.28 = 14.000000000000002 (floor 14, ceil 15)
    "k31-25-25": (31, True, (25, 25), ((0, 120), (60, 180)), dict(grid=False, extra_opts=[(0.58, False, 0, False, False), (0.28, False, 0, False, False)])),
    # one sample: floor(1 * 0.9) = 0, `ska weed x.skf` filters nothing
    "k31-one-sample": (31, True, (1,), ((0, 257),), dict(grid=False, extra_opts=[DEFAULTS, (1.0, False, 0, False, False)])),
    # two inputs without rows
    "k31-both-empty": (31, True, (2, 1), ((0, 0), (0, 0)), dict(grid=False, extra_opts=[DEFAULTS])),
    "k33-both-empty": (33, False, (1, 1), ((0, 0), (0, 0)), dict(grid=False)),
    # about 70 000 rows: the look-ups and the scatter span hundreds of blocks; sample i0s1 alone holds most of input 0's rows
    "k31-70k": (31, True, (2, 1), ((0, 45000), (20000, 70001)), dict(grid=False, heavy=(0, 1), extra_opts=[(0.5, False, 1, False, False)])),
    "k41-70k": (41, True, (1, 1), ((0, 40000), (30000, 70001)), dict(grid=False)),
}
_SEQUENCE = {
    "seq-k15": (15, True, (2, 2, 1)),
    "seq-k31-norc": (31, False, (3, 2)),
    "seq-k33": (33, True, (2, 2)),
    "seq-k41-norc": (41, False, (1, 2, 1)),
    "seq-k63": (63, True, (2, 1)),
}
CASES = list(_MATRIX) + list(_SEQUENCE)
LARGE = ("k31-70k", "k41-70k")


@functools.lru_cache(maxsize=None)
def make_case(name):
    seed = 1 + sorted(CASES).index(name)
    if name in _MATRIX:
        k, rc, sizes, ranges, kw = _MATRIX[name]
        return matrix_case(name, k, rc, sizes, ranges, 8800 + seed, **kw)
    k, rc, split = _SEQUENCE[name]
    return sequence_case(name, k, rc, split, 9900 + seed)


@functools.lru_cache(maxsize=None)
def expected(name):
    """the model's results of a case, computed once and shared: the merged array (key "merged": the subject of the deletions and weeds), label -> (request, result) of the deletions,
    label -> (records, keys) of the weed sets and the weed runs (label | None, reverse, options)"""
    case = make_case(name)
    # a single input is the subject itself (its stored counts reach the weed); several are merged first
    merged = merge(case["inputs"]) if len(case["inputs"]) > 1 else by_key(case["inputs"][0])
    dels = {}
    for lab, req in deletions(case):
        dels[lab] = (req, delete_samples(merged, req))
    sets, plan = weed_plan(case, merged)
    return dict(case=case, merged=merged, deletions=dels, sets=sets, plan=plan)


def run_weed(merged, keys, reverse, opts, **wrong):
    return weed(merged, keys, reverse, *opts, **wrong)


def data_path(*parts):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", *parts)
