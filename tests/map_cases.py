"""Seeded inputs of the `ska map` edge tests (tests/test_map_model.py on the CPU, tests/test_gpu_map_edges.py and
tests/test_cli_map_edges.py on the device): per case one set of samples (ancestor + point mutations, planted multi-allelic sites,
samples without the head / a middle piece / the tail, extra records that turn middle bases into ambiguity codes) and one reference
of 9-10 kbp laid out from the same ancestor so that the edges of the map kernels exist in it.  What can be checked on the layout
alone is asserted here; what needs the mapped cells is asserted in tests/test_map_model.py."""
import functools
import gzip
import os

import numpy as np

import ora

ACGT = b"ACGT"
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
WRAP = 61                                  # sequence lines of the reference: an odd width
ANC_LEN = 8600
SMALL_LENS = [23, 9, 31, 15, 14, 16, 27, 38, 12, 29, 11, 18, 22, 17]

# tile: where the record separator behind the padded foreign chromosome lands in the record stream (the window kernel's tile is
# 4096 positions); off32: output offset of the longest mapped chromosome mod 32 (presence words; mod 4: the flank kernel's groups
# of four positions); total4: total output length mod 4
CASES = {
    "C5": dict(k=5, rc=True, S=5, tile=4095, off32=0, total4=1),
    "C9": dict(k=9, rc=True, S=5, tile=4096, off32=1, total4=2),
    "C21": dict(k=21, rc=False, S=5, tile=4097, off32=31, total4=3, gz=True),
    "C31": dict(k=31, rc=True, S=67, tile=4095, off32=2, total4=1),
    "C33": dict(k=33, rc=True, S=5, tile=4096, off32=0, total4=2, repeat_at_zero=True),
    "C63": dict(k=63, rc=True, S=5, tile=4097, off32=31, total4=3),
    "C63s": dict(k=63, rc=False, S=5, tile=4095, off32=1, total4=0),
    "L40": dict(k=15, rc=True, S=9, tile=4096, off32=3, total4=1, small=22),
}
GRID = [(fmt, ambig_mask, repeat_mask) for fmt in ("aln", "vcf") for ambig_mask in (False, True) for repeat_mask in (False, True)]

# extra records: which other bases join a sample's own middle base (as shifts in ACGT) -- one copy: the six two-base codes, two
# copies: the four three-base codes, three copies: N
AMBIG_SHIFTS = [(1,), (2,), (3,), (1, 2), (1, 3), (2, 3), (1, 2, 3)]


def first_difference(got, want):
    """where two texts part, for an assertion's message"""
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (x, y) in enumerate(zip(g, w)):
        if x != y:
            j = next((j for j in range(min(len(x), len(y))) if x[j] != y[j]), min(len(x), len(y)))
            return "line %d of %d/%d, column %d of %d/%d: got %r, want %r" % (i, len(g), len(w), j, len(x), len(y), x[max(j - 8, 0):j + 24], y[max(j - 8, 0):j + 24])
    return "%d lines, want %d" % (len(g), len(w))


def revcomp(s):
    return bytes(s).translate(_COMP)[::-1]


def _shift(base, d):
    return ACGT[(ACGT.index(base) + d) % 4]


def _random(rng, n):
    return bytes(np.frombuffer(ACGT, np.uint8)[rng.integers(0, 4, size=n)].tolist())


class Case:
    def __init__(self, name, k, rc, S, ref, samples, gz, layout):
        self.name, self.k, self.rc, self.S, self.gz = name, k, rc, S, gz
        self.half = (k - 1) // 2
        self.ref = ref                      # [(id, description, bytes)]
        self.samples = samples              # [[record bytes]] per sample
        self.names = ["s%02d" % i for i in range(S)]
        self.layout = layout                # chromosome index by role, stretch positions: for the preconditions

    def model_ref(self):
        return [(i, s) for i, _, s in self.ref]

    def write_ref(self, directory):
        path = os.path.join(str(directory), self.name + (".fa.gz" if self.gz else ".fa"))
        with (gzip.open if self.gz else open)(path, "wb") as f:
            for i, desc, s in self.ref:
                f.write(b">" + i.encode() + b"\t" + desc.encode() + b"\n")
                for o in range(0, len(s), WRAP):
                    f.write(s[o:o + WRAP] + b"\n")
        return path

    def write_samples(self, directory):
        """one FASTA file per sample -> [(name, path, None)] as Array.build takes them"""
        inputs = []
        for n, recs in zip(self.names, self.samples):
            p = os.path.join(str(directory), "%s_%s.fa" % (self.name, n))
            with open(p, "wb") as f:
                for j, r in enumerate(recs):
                    f.write(b">r%d\n" % j + r + b"\n")
            inputs.append((n, p, None))
        return inputs

    def oracle_array(self):
        dicts = []
        for recs in self.samples:
            d = ora.Dict.new(self.k, self.rc)
            for r in recs:
                d.add_record(r)
            dicts.append(d)
        return ora.Array.from_dicts(dicts, self.names)

    def oracle_texts(self, ref_path, oa=None):
        oa = oa or self.oracle_array()
        return {g: oa.map(ref_path, fmt=g[0], ambig_mask=g[1], repeat_mask=g[2]) for g in GRID}


@functools.lru_cache(maxsize=None)
def make_case(name):
    spec = CASES[name]
    k, rc, S = spec["k"], spec["rc"], spec["S"]
    half = (k - 1) // 2
    rng = np.random.default_rng(1000 + 7 * k + S + (0 if rc else 1))
    anc = bytearray(_random(rng, ANC_LEN))
    T = 4 * k + 6
    unit = b"ACCGTAG"
    anc[7100:7100 + T] = (unit * (T // 7 + 1))[:T]                          # a tandem repeat the samples carry too
    anc = bytes(anc)

    # ---- samples
    planted = [150, 330, 510, 690, 870, 5950, 6100, 6250]                   # three different alternative bases over the samples
    samples = []
    for i in range(S):
        s = bytearray(anc)
        for p in rng.integers(0, ANC_LEN, size=12):
            s[p] = ACGT[rng.integers(0, 4)]
        for p in planted:
            s[p] = _shift(anc[p], i % 4)
        s = bytes(s)
        kind = i % 5
        if kind == 2:
            recs = [s[1400:]]                                               # lacks the head
        elif kind == 3:
            recs = [s[:5200], s[5600:]]                                     # lacks a middle piece
        elif kind == 4:
            recs = [s[:7400]]                                               # truncated at the tail
        else:
            recs = [s[:4000], s[4000 - (k - 1):]]                           # whole, in two overlapping records
        if kind == 1 and i < 10:
            # copies of the sample's own windows with another middle base, closed by an N (a clean run of exactly k letters at
            # the end of a record gives no window)
            for j, p in enumerate(range(60 + half + i, ANC_LEN - k, 23)):
                for d in AMBIG_SHIFTS[j % len(AMBIG_SHIFTS)]:
                    recs.append(s[p - half:p] + bytes([_shift(s[p], d)]) + s[p + 1:p + half + 1] + b"N")
        samples.append(recs)

    # ---- reference
    body = bytearray(anc[2000:5200])
    stretches, pairs = {}, {}
    gap = 2 * k + 4
    cur = gap

    def foreign_at(at, n):
        for x in range(at, at + n):
            body[x] = _shift(body[x], 1)

    for L in (1, 2, half, half + 1, k - 1, k, k + 1, 2 * k):               # foreign stretches: every base differs from the ancestor's
        foreign_at(cur, L)
        stretches[L] = cur
        cur += L + gap
    for d in (half + 1, half + 2, 2 * half + 1):                            # two changed bases d apart: d - 1 windows between them lost
        foreign_at(cur, 1)
        foreign_at(cur + d, 1)
        pairs[d] = cur
        cur += d + gap
    n_single = cur
    body[cur] = ord("N")
    cur += 1 + gap
    n_run = cur
    body[cur:cur + 11] = b"N" * 11
    cur += 11 + gap
    lower = cur
    body[cur:cur + 90] = bytes(body[cur:cur + 90]).lower()
    cur += 90 + gap
    assert cur < len(body) - gap, (name, cur)

    r0 = _random(rng, 3 * k) if spec.get("repeat_at_zero") else b""
    chroms = [
        ("f_first", r0 + _random(rng, 97)),                                 # foreign, in the first place
        ("head", anc[0:1300]),                                              # the first mapped chromosome
        ("e0", anc[1400:1400 + 3 * k + 5]),                                 # first present position: half
        ("e1", bytes([_shift(anc[1700], 1)]) + anc[1701:1700 + 3 * k + 5]),  # first present position: half + 1
        ("len_km1", anc[5600:5600 + k - 1]),
        ("len_k", anc[5700:5700 + k]),
        ("len_kp1", anc[5800:5800 + k + 1]),
        ("mid", anc[5250:5550]),                                            # inside the piece that every fifth sample lacks
        ("rc1", revcomp(anc[5900:6300])),
        ("rc2", anc[6300:6500] + revcomp(anc[6500:6700])),
        ("f_mid", None),                                                    # foreign, padded to the tile edge
        ("all_n", None),                                                    # no window at all, before the repeats below
        ("body", bytes(body)),
        ("rep", anc[6700:7100] + anc[6800:6800 + 3 * k]),                   # a copy inside one chromosome
        ("rep2", anc[300:300 + 3 * k] + _random(rng, 20) + revcomp(anc[600:600 + 3 * k])),   # of another chromosome; reverse-complemented
        ("tandem", anc[7060:7100 + T + 40]),
    ]
    o = 8000 if "small" in spec else ANC_LEN
    for j in range(spec.get("small", 0)):                                   # (cut from behind the tail chromosome's stretch)
        n = SMALL_LENS[j % len(SMALL_LENS)]
        chroms.append(("small%02d" % j, anc[o:o + n]))
        o += n
    chroms += [("tail", anc[7500:o]), ("f_last", None)]                  # the last mapped chromosome; foreign, in the last place
    seqs = dict(chroms)
    order = [n for n, _ in chroms]
    i_mid = order.index("f_mid")
    before = sum(len(seqs[n]) for n in order[:i_mid]) + i_mid               # record stream: one separator behind every chromosome
    assert spec["tile"] - before > 2 * k, (name, before)
    seqs["f_mid"] = _random(rng, spec["tile"] - before)
    off = sum(len(seqs[n]) for n in order[:i_mid + 1])
    seqs["all_n"] = b"N" * (30 + (spec["off32"] - off - 30) % 32)
    rest = sum(len(s) for s in seqs.values() if s is not None) + len(r0)
    seqs["f_last"] = _random(rng, 56 + (spec["total4"] - rest - 56) % 4) + r0     # (r0: the repeat that starts at output coordinate 0)
    ref = [("%s_%02d_%s" % (name, c, n), "case %s, chromosome %d" % (name, c), seqs[n]) for c, n in enumerate(order)]

    # ---- what the layout alone shows
    lens = [len(s) for _, _, s in ref]
    offs = [sum(lens[:c]) for c in range(len(ref))]
    assert sum(lens[:i_mid + 1]) + i_mid == spec["tile"]                    # that separator's place in the record stream
    assert offs[order.index("body")] % 32 == spec["off32"] and sum(lens) % 4 == spec["total4"]
    assert [lens[order.index(n)] for n in ("len_km1", "len_k", "len_kp1")] == [k - 1, k, k + 1]
    assert 9000 <= sum(lens) <= 10500 and sum(lens) + len(lens) > 2 * 4096, (name, sum(lens))
    assert set(seqs["all_n"]) == {ord("N")} and order.index("all_n") < order.index("rep")
    if "small" in spec:
        assert len(ref) == 40 and sum(n < k for n in lens) >= 3 and sum(n < 100 for n in lens) > 20
    layout = dict(order=order, offs=offs, lens=lens, stretches=stretches, pairs=pairs, n_single=n_single, n_run=n_run, lower=lower)
    return Case(name, k, rc, S, ref, samples, bool(spec.get("gz")), layout)
