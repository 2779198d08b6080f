"""Test-only restatement of `ska lo` (the reference's src/skalo/*.rs) with the engine's fixed orders:

  * neighbour lists ascending by node value; entry / exit nodes visited ascending; compaction: entry pass, then exit pass,
    edges rewritten in ascending order of the chain's first node
  * a tie for the most common path length goes to the shortest length
  * variant groups by (paths / length) descending, then (entry, exit) ascending; indels written in (entry, exit) order
  * SNPs of a group in ascending position; ALT bases of `_snps.vcf` in A, C, G, T order
  * k-mer colours: the first writer is the lowest (split k-mer, middle base code)

Nodes and k-mers are Python ints in the reference's 2-bit code (A=0, C=1, T=2, G=3, first base in the high bits,
bit_encoding.rs:123-166); colours are ints used as sample bitsets.  Reads arrays through tests/ora.py (the CPU oracle)."""
import collections

CODE = "ACTG"
IUPAC = {"A": "A", "T": "T", "G": "G", "C": "C", "M": "AC", "S": "CG", "W": "AT", "R": "AG", "Y": "CT", "K": "GT",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
NO_ENTRY = "Error: there is no entry node in this graph, hence no variant.\n"


class NoEntry(Exception):
    pass


def enc_base(c):
    return (ord(c) >> 1) & 3


BASE4 = str.maketrans({chr(c): str((c >> 1) & 3) for c in range(256)})     # enc_base as a base-4 digit


def encode(s):
    return int(s.translate(BASE4), 4) if s else 0


def windows(s, n):
    """[encode(s[i:i + n]) for i in range(len(s) - n + 1)], cut from encode(s) as one integer"""
    L = len(s)
    if n > L:
        return []
    v = encode(s)
    mask = (1 << (2 * n)) - 1
    return [(v >> (2 * (L - n - i))) & mask for i in range(L - n + 1)]


def decode(v, n):
    return "".join(CODE[(v >> (2 * (n - 1 - i))) & 3] for i in range(n))


def rc(v, n):
    out = 0
    for _ in range(n):
        out = (out << 2) | ((v & 3) ^ 2)
        v >>= 2
    return out


def rev_compl(s):
    return s[::-1].translate(str.maketrans("ACTG", "TGAC"))


def build_graph(keys, variants, k):
    """read_graph.rs:build_graph.  keys: split k-mer ints per row; variants: rows x samples of ASCII codes.
    Returns (edges: node -> ascending list with repeats, colours: K -> sample bitset, present: [(row, b, bitset)])."""
    half = (k - 1) // 2
    edges = collections.defaultdict(list)
    colours = {}
    present = []
    order = sorted(range(len(keys)), key=lambda r: keys[r])
    for r in order:
        key = keys[r]
        left, right = key >> (2 * half), key & ((1 << (2 * half)) - 1)
        sets = [0, 0, 0, 0]
        for s, cell in enumerate(variants[r]):
            for c in IUPAC.get(chr(cell), ""):
                sets[enc_base(c)] |= 1 << s
        for b in range(4):
            if not sets[b]:
                continue
            K = (left << (2 * (half + 1))) | (b << (2 * half)) | right
            src, dst = K >> 2, K & ((1 << (2 * (k - 1))) - 1)
            edges[src].append(dst)
            edges[rc(dst, k - 1)].append(rc(src, k - 1))
            colours.setdefault(K, sets[b])
            colours.setdefault(rc(K, k), sets[b])
            present.append((r, b, sets[b]))
    for v in edges.values():
        v.sort()
    return dict(edges), colours, present


def extremities(edges, colours, kg):
    """extremities.rs:identify_good_kmers"""
    entries = set()
    for node, nxt in edges.items():
        if len(nxt) > 1:
            full = [colours[(node << 2) | (c & 3)] for c in nxt]
            if any(full[i] != full[j] for i in range(len(full)) for j in range(i + 1, len(full))):
                entries.add(node)
    return entries, {rc(e, kg) for e in entries}


def compact(edges, entries, exits):
    """compaction.rs:compact_graph (edges modified in place)"""
    compacted = {}
    for group in (sorted(entries), sorted(exits)):
        for node in group:
            for s in edges.get(node, ()):
                cur, seen, chain = s, set(), []
                while True:
                    nxt = edges.get(cur)
                    if nxt is not None and len(nxt) == 1 and nxt[0] not in seen:
                        cur = nxt[0]
                        chain.append(cur)
                        seen.add(cur)
                        if cur in exits or cur in entries:
                            break
                    else:
                        break
                if len(chain) > 1:
                    compacted[s] = chain
    for s in sorted(compacted):
        chain = compacted[s]
        edges[s] = [n for n in edges[s] if n != chain[0]]
        for a, b in zip(chain[:-2], chain[1:-1]):
            edges[a] = [n for n in edges[a] if n != b]
        edges[s].append(chain[-1])
        chain.pop()
    return compacted


def most_abundant_length(paths):
    counts = collections.Counter(len(p) for p in paths)
    best = max(counts.values())
    return min(n for n, c in counts.items() if c == best)


def traverse(entry, edges, compacted, entries, exits, kg, max_depth):
    """read_graph.rs:build_variant_groups, one entry node: {(entry, exit): [(sequence, snp positions)]}"""
    found = {}
    for s in edges[entry]:
        stack = [(s, {entry, s}, [entry, s] + compacted.get(s, []), 0)]
        while stack:
            cur, seen, path, depth = stack.pop()
            if depth > max_depth:
                continue
            while True:
                good = [n for n in edges.get(cur, ()) if n not in seen]
                if len(good) == 1:
                    nx = good[0]
                    seen.add(nx)
                    path.append(nx)
                    cur = nx
                    path.extend(compacted.get(nx, ()))
                    if nx in exits:
                        found.setdefault(nx, []).append(list(path))
                elif len(good) > 1:
                    for nx in good:
                        nseen = set(seen)
                        nseen.add(nx)
                        npath = path + [nx] + compacted.get(nx, [])
                        if nx in exits:
                            found.setdefault(nx, []).append(list(npath))
                        stack.append((nx, nseen, npath, depth + 1))
                    break
                else:
                    break
    out = {}
    if not any(len(v) > 1 for v in found.values()):
        return out
    for ex, paths in found.items():
        if len({p[1] for p in paths}) > 1 and len({p[-2] for p in paths}) > 1:
            mcl = most_abundant_length(paths)
            keep = paths if len(paths) == 2 else [p for p in paths if len(p) == mcl]
            group = []
            for p in keep:
                seq = decode(entry, kg) + "".join([CODE[n & 3] for n in p[1:]])
                snps = []
                for i, n in enumerate(p):
                    if n in entries and (len(p) < kg or i <= len(p) - kg):
                        snps.append(i + kg)
                    elif n in exits:
                        snps.append(i - 1)
                group.append((seq, snps))
            out[(entry, ex)] = group
    return out


def _colour(colours, s):
    if len(s) == 0:
        raise KeyError("empty k-mer")
    return colours[encode(s)]


def extract_middle_bases(seqs, kg):
    reduced = [s[kg:] for s in seqs]
    n = 0
    identical = True
    while identical:
        n += 1
        ends = set()
        for s in reduced:
            if n > len(s):
                identical = False
            else:
                ends.add(s[len(s) - n:])
        if len(ends) > 1:
            identical = False
    n -= 1
    last = reduced[0][len(reduced[0]) - n:]
    if len(last) > kg:
        last = last[:kg]
    middles = [(s[:len(s) - n] or "-") for s in reduced]
    return middles, last


def process_indels(indels, colours, names, kg, max_missing):
    """process_indels.rs: (vcf text, entries_indels, count)"""
    S = len(names)
    taken, final = set(), {}
    for key, _ in sorted(((key, sum(len(s) for s, _ in v)) for key, v in indels.items()), key=lambda t: (t[1], t[0])):
        if key[0] not in taken:
            taken |= {key[0], rc(key[0], kg), key[1], rc(key[1], kg)}
            final[key] = indels[key]
    lines = ["##fileformat=VCFv4.2", "# REF corresponds to the most frequent variant among samples",
             "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names)]
    n_indels = 0
    for key in sorted(final):
        group = final[key]
        bits = [colours[encode(s[:kg + 1])] for s, _ in group if encode(s[:kg + 1]) in colours]
        missing, ref_p, alt_p = 0, False, False
        for i in range(S):
            a, b = (bits[0] >> i) & 1, (bits[1] >> i) & 1
            if a == b:
                missing += 1
            elif a:
                ref_p = True
            else:
                alt_p = True
        if f32(missing / S) <= f32(max_missing) and ref_p and alt_p:
            n_indels += 1
            middles, last = extract_middle_bases([s for s, _ in group], kg)
            first = group[0][0][:kg]
            var = sorted(zip(middles, [bin(b).count("1") for b in bits], bits), key=lambda t: -t[1])
            (ra, _, rb), (aa, _, ab) = var[0], var[1]
            calls = []
            for i in range(S):
                x, y = (rb >> i) & 1, (ab >> i) & 1
                calls.append("0/1" if x and y else "0" if x else "1" if y else ".")
            lines.append(f".\t.\t.\t{ra}\t{aa}\t.\tbefore={first};after={last}\t.\tGT\t" + "\t".join(calls))
    return "\n".join(lines) + "\n", taken, n_indels


def f32(x):
    import struct
    return struct.unpack("f", struct.pack("f", x))[0]


def read_reference(path, kg):
    """positioning.rs:extract_genomic_kmers (one record; more -> the reference panics)"""
    recs = []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            if line.startswith(b">"):
                recs.append([line[1:].split()[0].decode() if line[1:].split() else "", []])
            elif recs:
                recs[-1][1].append(line)
    if len(recs) > 1:
        raise ValueError("more than one sequence detected in the reference genome file")
    name, seq = recs[0][0], bytes(b for b in b"".join(recs[0][1]) if not chr(b).isspace()).upper()
    kmap = {}
    for n in range(len(seq) - kg + 1) if len(seq) >= kg else ():
        w = seq[n:n + kg]
        if all((c & 0xF) != 14 for c in w):
            e = encode(w.decode("latin-1"))
            p = kmap.setdefault(e, [])
            if len(p) < 3:
                p.append(n + kg)
    return kmap, seq.decode("latin-1"), name


def most_frequent_position(nums):
    counts = collections.Counter(nums)
    best = max(counts.values())
    top = [n for n, c in counts.items() if c == best]
    if len(top) > 1 or best < 10:
        return 0, 0
    return top[0], best


def scan_variants(seqs, kg, kmap):
    fwd, rev = [], []
    for seq in seqs:
        for s, out in ((seq, fwd), (rev_compl(seq), rev)):
            for pos, w in enumerate(windows(s, kg)):
                for p in kmap.get(w, ()):
                    out.append((p - pos) & 0xFFFFFFFF)
    f = most_frequent_position(fwd) if fwd else (0, 0)
    r = most_frequent_position(rev) if rev else (0, 0)
    f = f if f[1] else None
    r = r if r[1] else None
    if f and r:
        if f[1] == r[1]:
            return None
        return (f[0], True) if f[1] > r[1] else (r[0], False)
    if f:
        return f[0], True
    if r:
        return r[0], False
    return None


def check_missing(col):
    present = {c for c in col if c in "ATGC"}
    miss = sum(1 for c in col if c not in "ATGC")
    return len(present) >= 2, f32(miss / len(col))


def run(keys, variants, k, names, reference=None, missing=0.1, depth=4, indel_kmers=2, log=None):
    """Steps 1-6.  Returns {suffix: text} for `_snps.fas` (+ `_pseudo_genomes.fas`, `_snps.vcf` with a reference) and
    `_indels.vcf`, plus the counts the reference logs.  Raises NoEntry when the graph has no entry node."""
    kg = k - 1
    S = len(names)
    edges, colours, _ = build_graph(keys, variants, k)
    counts = {"nodes": len(edges)}
    entries, exits = extremities(edges, colours, kg)
    if not entries:
        raise NoEntry(NO_ENTRY)
    counts["entries"] = len(entries)
    compacted = compact(edges, entries, exits)
    groups = {}
    for e in sorted(entries):
        groups.update(traverse(e, edges, compacted, entries, exits, kg, depth))
    counts["groups"] = len(groups)
    final_groups, indels = {}, {}
    for key, vv in groups.items():
        if len(vv) < 2:
            continue
        if len(vv) == 2 and len(vv[0][0]) != len(vv[1][0]):
            if any(len(s) <= 2 * kg for s, _ in vv):
                indels[key] = vv
        else:
            final_groups[key] = vv
    kmap, genome, gname = read_reference(reference, kg) if reference else ({}, "", "")
    out = {}
    out["_indels.vcf"], entries_indels, counts["indels"] = process_indels(indels, colours, names, kg, missing)
    for key in final_groups:
        final_groups[key] = [(s, p) for s, p in final_groups[key]
                             if sum(1 for w in windows(s, kg)[:-1] if w in entries_indels) <= indel_kmers]
    order = sorted(((key, len(v) / len(v[0][0])) for key, v in final_groups.items() if v), key=lambda t: (-t[1], t[0]))
    done, snps, not_positioned, counter = set(), {}, 0, 0
    for key, _ in order:
        if key[0] in entries_indels or rc(key[1], kg) in entries_indels:
            continue
        vv = final_groups[key]
        if len(vv) < 2:
            continue
        cand = set()
        for _, p in vv:
            cand.update(p)
        real = sorted(pos for pos in cand if len({s[pos] for s, _ in vv if pos < len(s)}) > 1)
        to_save, found = set(), {}
        for pos in real:
            col = ["-"] * S
            tmp = set()
            new = True
            for s, _ in vv:
                before, after = s[pos - kg:pos + 1], s[pos:pos + kg + 1]
                if pos < kg or len(before) != kg + 1 or len(after) != kg + 1:
                    raise IndexError("SNP flank outside the path")
                fb, fa = encode(before), encode(after)
                ra = rc(fa, kg + 1)
                if fb not in done and ra not in done:
                    last = CODE[fb & 3]
                    bits = colours[fb]
                    for i in range(S):
                        if (bits >> i) & 1:
                            col[i] = last if col[i] in ("-", last) else "N"
                    tmp |= {fb, rc(fb, kg + 1), fa, ra}
                else:
                    new = False
            if new:
                ok, ratio = check_missing(col)
                if ok and ratio <= f32(missing):
                    to_save |= tmp
                    found[pos] = col
        done |= to_save
        if not found:
            continue
        if reference:
            where = scan_variants([s for s, _ in vv], kg, kmap)
            if where is None:
                not_positioned += len(found)
                continue
            position, fwd = where
            L = len(vv[0][0])
            comp = str.maketrans("ATCG-N", "TAGC-N")
            for pos in sorted(found):
                fp = (position + (pos - kg if fwd else L - pos - kg - 1)) & 0xFFFFFFFF
                col = found[pos] if fwd else [c.translate(comp) for c in found[pos]]
                if fp in snps:
                    not_positioned += 1
                else:
                    snps[fp] = col
        else:
            for pos in sorted(found):
                counter += 1
                snps[counter] = found[pos]
    counts["snps"], counts["unpositioned"] = len(snps), not_positioned
    out.update(write_snps(snps, names, genome, gname))
    return out, counts


def write_snps(snps, names, genome, gname):
    """output_snps.rs:create_fasta_and_vcf"""
    genome = "".join(c if c in "ATGCN" else "N" for c in genome)
    ordered = sorted(snps.items())
    length = len(genome) if genome else (ordered[-1][0] + 1 if ordered else 0)
    seqs = [[] for _ in names]
    aln = [[] for _ in names] if genome else None
    vcf = []
    cur = 0
    for pos in range(length):
        if cur < len(ordered) and ordered[cur][0] == pos:
            col = ordered[cur][1]
            if aln is not None:
                vcf.append((pos, genome[pos], col))
                for i, c in enumerate(col):
                    aln[i].append(c)
            for i, c in enumerate(col):
                seqs[i].append(c)
            cur += 1
        elif aln is not None:
            for a in aln:
                a.append(genome[pos])
    out = {"_snps.fas": "".join(f">{n}\n{''.join(s)}\n" for n, s in zip(names, seqs))}
    if genome:
        out["_pseudo_genomes.fas"] = "".join(f">{n}\n{''.join(s)}\n" for n, s in zip(names, aln))
        lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names)]
        for pos, ref, col in vcf:
            alts = [c for c in "ACGT" if c != ref and c in col]
            gts = ["0" if c == ref else "." if c in "-N" else str(alts.index(c) + 1) if c in alts else "." for c in col]
            lines.append(f"{gname}\t{pos + 1}\t.\t{ref}\t{','.join(alts)}\t.\t.\t.\tGT\t" + "\t".join(gts))
        out["_snps.vcf"] = "\n".join(lines) + "\n"
    return out


def array_inputs(arr):
    """(keys, variants, k, names) of an ora.Array (or anything with export / k / names)"""
    keys, var, _ = arr.export()
    ints = [int(lo) | (int(hi) << 64) for lo, hi in zip(keys["lo"], keys["hi"])]
    return ints, [bytes(r) for r in var], arr.k, arr.names


def run_skf(path, **kw):
    import ora
    a = ora.Array.load(path)
    keys, var, k, names = array_inputs(a)
    return run(keys, var, k, names, **kw)


def graph_skf(path):
    """the device graph's counterpart: (sorted nodes, {node: neighbours}, sorted entries, sorted exits, colours)"""
    import ora
    keys, var, k, names = array_inputs(ora.Array.load(path))
    return graph_of(keys, var, k)


def graph_of(keys, var, k):
    edges, colours, present = build_graph(keys, var, k)
    entries, exits = extremities(edges, colours, k - 1)
    return sorted(edges), edges, sorted(entries), sorted(exits), colours
