"""`ska map` on the CPU: the closed-form model (tests/map_model.py) against the oracle's literal restatement of the reference's
sequential writer (oracle/ora_map.c), on the inputs of tests/map_cases.py -- and the preconditions that show those inputs reach the
edges the device tests (tests/test_gpu_map_edges.py) are there for.

The model has no term for writer state left over at a chromosome change (last_mapped / last_written are not reset there).  That it
equals the walk on every case says none is needed: after a chromosome's closing fill, last_written = last_mapped + half + 1 (a
window's middle lies at most at len - 1 - half), so every fill's overhang saturates to 0 until the next chromosome's first write."""
import functools

import numpy as np
import pytest

import map_cases as MC
import map_model as MM

CODES2, CODES3 = b"RYKMSW", b"BDHV"
ALL_CODES = CODES2 + CODES3 + b"N"
NAMES = list(MC.CASES)
RANDOM_HITS_RARE = [n for n in NAMES if MC.CASES[n]["k"] >= 15]       # below that a 9 kbp sample holds a good part of all 4^(k-1) split
#                                                                        k-mers (k = 9: one in seven), so "foreign" sequence maps too


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("map_model")

    @functools.lru_cache(maxsize=None)
    def get(name):
        c = MC.make_case(name)
        oa = c.oracle_array()
        keys, var, _ = oa.export()
        texts = c.oracle_texts(c.write_ref(d), oa)
        return c, (keys, var), texts, MM.MapModel(keys, var, c.names, c.k, c.rc, c.model_ref())
    return get


def _runs(mask):
    """lengths of the runs of False between two True"""
    p = np.flatnonzero(mask)
    return set((np.diff(p) - 1).tolist()) - {0}


def _present_by_chrom(m, s):
    return {int(c): m.m_pos[m.present(s) & (m.m_chrom == c)] for c in np.unique(m.m_chrom[m.present(s)])}


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_oracle(world, name):
    c, _, texts, m = world(name)
    for g in MC.GRID:
        assert m.text(*g) == texts[g], (name, g)


def test_cases_tell_mutants_apart(world):
    for mutant in MM.MUTANTS:
        told = False
        for name in NAMES:
            c, (keys, var), texts, m = world(name)
            mm = MM.MapModel(keys, var, c.names, c.k, c.rc, c.model_ref(), mutant=mutant, windows_from=m)
            if any(mm.text(*g) != texts[g] for g in MC.GRID):
                told = True
                break
        assert told, mutant


def test_repeat_quirk_is_reached(world):
    """a chromosome without windows before a repeat: true chromosome offsets give other coordinates than the reference's"""
    differs = []
    for name in NAMES:
        c, (keys, var), texts, m = world(name)
        mm = MM.MapModel(keys, var, c.names, c.k, c.rc, c.model_ref(), mutant="repeat_true_offsets", windows_from=m)
        if mm.text("aln", False, True) != texts[("aln", False, True)]:
            differs.append(name)
    assert differs


@pytest.mark.parametrize("name", [n for n in NAMES if MC.CASES[n]["k"] >= 9])
def test_ambiguity_codes_on_both_strands(world, name):
    c, _, _, m = world(name)
    assert set(ALL_CODES) <= set(np.unique(m.cells).tolist())
    if c.rc:
        for strand in (m.m_rc, ~m.m_rc):
            missing = set(ALL_CODES) - set(np.unique(m.cells[strand]).tolist())
            assert not missing, (name, bytes(sorted(missing)))
    else:
        assert not m.m_rc.any()


@pytest.mark.parametrize("name", RANDOM_HITS_RARE)
def test_per_sample_missing_chromosomes(world, name):
    c, _, _, m = world(name)
    mapped = sorted(set(m.m_chrom.tolist()))
    order = c.layout["order"]
    assert order[mapped[0]] == "head" and order[mapped[-1]] == "tail" and order.index("mid") in mapped[1:-1]
    pres = [set(_present_by_chrom(m, s)) for s in range(c.S)]
    assert any(mapped[0] not in p for p in pres)
    assert any(order.index("mid") not in p for p in pres)
    assert any(mapped[-1] not in p for p in pres)
    assert any(p == set(mapped) for p in pres)


@pytest.mark.parametrize("name", NAMES)
def test_vcf_lines_and_repeat_mask(world, name):
    c, _, texts, m = world(name)
    lines = [l.split("\t") for l in texts[("vcf", False, False)].decode().splitlines() if not l.startswith("#")]
    if c.k >= 9:                                                                 # (k = 5: 256 split k-mers, each seen with every middle base: all N)
        assert sum("," in l[4] for l in lines) >= 3                              # two or more ALT alleles
    assert any("N" in l[4].split(",") for l in lines)
    assert any("." in l[9:] for l in lines)
    assert any(l[3] == "N" for l in lines)                                       # a lower-case or N reference base
    assert texts[("aln", False, True)] != texts[("aln", False, False)]           # --repeat-mask changes something
    if c.k >= 9:
        assert texts[("aln", True, False)] != texts[("aln", False, False)]       # and so does --ambig-mask


@pytest.mark.parametrize("name", NAMES)
def test_layout_windows_and_repeats(world, name):
    c, _, _, m = world(name)
    k, half, order, lens = c.k, c.half, c.layout["order"], c.layout["lens"]
    ix = order.index
    # a record of k - 1 or k letters gives no window (the iterator asks for k + 1 letters where a run starts), k + 1 letters give
    # two: the first at half, the last at len - 1 - half
    assert m.win[ix("len_km1")] == [] and m.win[ix("len_k")] == [] and m.win[ix("all_n")] == []
    assert [w[0] for w in m.win[ix("len_kp1")]] == [half, half + 1] and half + 1 == lens[ix("len_kp1")] - 1 - half
    # repeats: a copy inside one chromosome, of another chromosome, reverse-complemented, tandem
    count = {}
    for ws in m.win:
        for _, split, _ in ws:
            count[split] = count.get(split, 0) + 1
    rep = {n: np.array([count[w[1]] > 1 for w in m.win[ix(n)]]) for n in order}
    if k >= 15:
        assert rep["rep"][100:100 + k].all() and rep["rep"][-k:].all() and not rep["rep"][:60].any()
        assert rep["head"][300:300 + k].all() and rep["rep2"][:k].all() and not rep["mid"].any()
        both = np.concatenate([rep["head"][600:600 + k], rep["rep2"][-k:]])
        assert both.all() if c.rc else not both.any()                            # single strand: the reverse copy is no repeat
    assert rep["tandem"][40:40 + 3 * k - 1].all()                                    # consecutive repeat windows: overlapping ranges
    if MC.CASES[name].get("repeat_at_zero"):
        assert m.repeat_coords()[0] == 0
    assert len(m.repeat_coords()) > 0


@pytest.mark.parametrize("name", RANDOM_HITS_RARE)
def test_layout_present_positions(world, name):
    c, _, _, m = world(name)
    k, half, order, offs = c.k, c.half, c.layout["order"], c.layout["offs"]
    ix = order.index
    mapped = set(m.m_chrom.tolist())
    assert not mapped & {ix("f_first"), ix("f_mid"), ix("f_last"), ix("all_n"), ix("len_km1"), ix("len_k")}
    assert (ix("rc1") in mapped) == c.rc and ix("rc2") in mapped
    firsts = {n: {int(_present_by_chrom(m, s)[ix(n)][0]) for s in range(c.S) if ix(n) in _present_by_chrom(m, s)} for n in ("e0", "e1")}
    assert half in firsts["e0"] and firsts["e1"] and min(firsts["e1"]) == half + 1
    # runs of positions without a present mapped k-mer, between two that have one: a changed base alone (half), two of them
    # half + 2 and k apart (half + 1 and 2 * half: flanks that just touch), one N (2 * half + 1: one position uncovered), L foreign
    # bases (L + 2 * half)
    body = ix("body")
    runs = set()
    for s in range(c.S):
        p = _present_by_chrom(m, s).get(body)
        if p is not None:
            mask = np.zeros(c.layout["lens"][body], bool)
            mask[p] = True
            runs |= _runs(mask)
    want = {half, half + 1, 2 * half, 2 * half + 1, 2 * half + 2, 11 + 2 * half} | {L + 2 * half for L in c.layout["stretches"] if L >= 2}
    assert want <= runs, (name, sorted(want - runs))
    seq = c.ref[body][2]
    assert seq[c.layout["lower"]:c.layout["lower"] + 90].islower() and seq[c.layout["n_run"]:c.layout["n_run"] + 11] == b"N" * 11


def test_offsets_and_tile_edges_over_the_cases(world):
    off32, off4, total4, tiles = set(), set(), set(), set()
    for name in NAMES:
        c, _, _, m = world(name)
        for ch in set(m.m_chrom.tolist()):
            off32.add(c.layout["offs"][ch] % 32)
            off4.add(c.layout["offs"][ch] % 4)
        total4.add(sum(c.layout["lens"]) % 4)
        stream = np.cumsum(np.array(c.layout["lens"]) + 1) - 1                   # the separators' places in the record stream
        tiles |= set(stream.tolist()) & {4095, 4096, 4097}
        assert c.layout["offs"][c.layout["order"].index("body")] % 32 == MC.CASES[name]["off32"]
        assert len(stream) + int(stream[-1]) > 2 * 4096 and sum(c.layout["lens"]) > 2 * 4096       # > 2 window tiles, 3 VCF blocks
    assert {0, 1, 31} <= off32 and {1, 2, 3} <= off4 and {1, 2, 3} <= total4 and tiles == {4095, 4096, 4097}


@pytest.mark.parametrize("k", [5, 7, 15, 31, 63])
def test_random_layouts_need_no_stale_state_term(tmp_path, k):
    """1-6 chromosomes of k - 1, k, k + 1 or a random number of letters, single windows of them given to the samples at densities
    from 0.02 to 1: the walk, which carries last_mapped / last_written over every chromosome change, writes the union of the
    windows and nothing else"""
    import ora
    rng = np.random.default_rng(k)
    compared = 0
    for trial in range(40):
        lens = [int(rng.choice([k - 1, k, k + 1, k + 2, int(rng.integers(k, 4 * k + 40))])) for _ in range(int(rng.integers(1, 7)))]
        chroms = [MC._random(rng, n) for n in lens]
        density = float(rng.choice([0.02, 0.1, 0.3, 0.6, 1.0]))
        dicts = []
        for s in range(3):
            d = ora.Dict.new(k, True)
            for seq in chroms:
                for p in range(len(seq) - k + 1):
                    if rng.random() < density:
                        d.add_record(seq[p:p + k] + b"N")
            dicts.append(d)
        oa = ora.Array.from_dicts(dicts, ["a", "b", "c"])
        rp = str(tmp_path / ("r%d.fa" % trial))
        with open(rp, "wb") as f:
            for c, seq in enumerate(chroms):
                f.write(b">c%d\n" % c + seq + b"\n")
        keys, var, _ = oa.export()
        try:
            want = oa.map(rp)
        except ora.OracleError:                              # no window in the reference, or none mapped: nothing to compare
            continue
        assert MM.MapModel(keys, var, oa.names, k, True, [("c%d" % c, s) for c, s in enumerate(chroms)]).text() == want, (k, trial, lens)
        compared += 1
    assert compared >= 20                                   # (the rest: a lone chromosome too short for a window, or no hit at 0.02)
