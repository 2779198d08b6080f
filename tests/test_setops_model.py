"""tests/setops_model.py (the plain restatement of `ska merge` / `ska delete` / `ska weed`) against the CPU oracle on every case of its
list, on the reference's own .skf fixtures and goldens, and against deliberately wrong variants of itself -- before anything on the device
is compared with it (tests/test_gpu_setops_edges.py)."""
import os

import numpy as np
import pytest

import golden_cases as G
import ora
import setops_model as M


def o_arr(a):
    """a model array as an oracle array (rows in the model's order)"""
    return ora.Array.from_rows(a.k, a.rc, a.names, M.key_dt(a.keys), a.var, a.counts.astype(np.uint64))


def m_arr(o):
    keys, var, counts = o.export()
    return M.arr(o.k, o.rc, o.names, keys, var, counts)


def o_subject(case):
    ins = [o_arr(a) for a in case["inputs"]]
    if len(ins) == 1:
        ins[0].sort_rows()
        return ins[0]
    return ora.Array.merge(ins)


def agree(o, m, what, full_info=True):
    diff = M.same(m_arr(o), m)
    assert diff is None, (what, diff)
    assert o.nkmers == o.nrows == len(m.keys), what
    # rows of an oracle merge / delete / weed stay sorted by key, as the model's are: the nk texts are comparable line by line
    assert M.nk_lines(o.nk(full_info)) == M.nk(m, full_info), what


@pytest.mark.parametrize("name", M.CASES)
def test_model_equals_oracle(name, tmp_path):
    e = M.expected(name)
    case, merged = e["case"], e["merged"]
    full = name not in M.LARGE
    agree(o_subject(case), merged, "merge", full)
    for lab, (req, want) in e["deletions"].items():
        o = o_subject(case)
        o.delete_samples(req)
        agree(o, want, ("delete", lab), full)
    paths = {lab: M.write_fasta(recs, str(tmp_path / f"{lab}.fa")) for lab, (recs, _) in e["sets"].items()}
    for lab, (recs, keys) in e["sets"].items():
        assert sorted(M.fasta_keys(paths[lab], case["k"], case["rc"])) == sorted(keys), lab      # the file's dictionary = the records'
    for lab, reverse, opts in e["plan"]:
        keys = e["sets"][lab][1] if lab else None
        want = M.run_weed(merged, keys, reverse, opts)
        o = o_subject(case)
        if lab:
            before = o.nrows
            o.weed_keys(M.key_dt(keys), reverse)
            want_keys, removed = M.weed_keys(merged, keys, reverse)
            assert before - o.nrows == removed, (lab, reverse)
            agree(o, want_keys, ("weed_keys", lab, reverse), False)
        o.weed(None, False, **opts.kw())
        agree(o, want, ("weed", lab, reverse, opts.ident()), full)
        o2 = o_subject(case)                                             # the same through the FASTA file, as `ska weed` goes
        o2.weed(paths[lab] if lab else None, reverse, **opts.kw())
        agree(o2, want, ("weed file", lab, reverse, opts.ident()), False)


def test_the_case_list_holds_what_it_claims():
    shapes = {n: M.make_case(n) for n in M.CASES}
    per_input = {len(a.names) for c in shapes.values() for a in c["inputs"]}
    assert {1, 2, 5, 63, 64, 65} <= per_input
    assert max(sum(len(a.names) for a in c["inputs"]) for c in shapes.values()) == 130
    assert {2, 3, 6} <= {len(c["inputs"]) for c in shapes.values()}
    rows = {len(a.keys) for c in shapes.values() for a in c["inputs"]} | {len(M.expected(n)["merged"].keys) for n in M.CASES}
    g = M.GRANULE
    assert {0, 1, g - 1, g, g + 1, 2 * g - 1, 2 * g, 2 * g + 1} <= rows and any(r >= 70000 for r in rows)
    assert {(c["k"], c["rc"]) for c in shapes.values()} >= {(k, rc) for k in (5, 15, 31, 33, 41, 63) for rc in (True, False)}
    cells = set()
    for c in shapes.values():
        for a in c["inputs"]:
            cells |= set(np.unique(a.var).tolist())
            if len(a.names) >= 16 and len(a.keys):
                assert any(set(r.tolist()) == set(M.CODES) for r in a.var[:2]), c["name"]        # a row with the full code set
    assert cells == set(M.CODES)
    # rows no sample has, in inputs and in merged arrays; stored counts that differ from the rows
    assert any((a.var == M.GAP).all(axis=1).any() for c in shapes.values() for a in c["inputs"])
    st = shapes["k31-stored-counts"]["inputs"][0]
    assert (st.counts != M.present(st.var)).sum() > 50 and (st.counts == 0).any()
    # wide keys: hi == 0, pairs that differ only in lo, pairs that differ only in hi; k = 33 is 64 key bits in a 128-bit array: hi == 0
    # throughout, the top bit of lo in use
    for n in ("k33-norc-chain", "k41-norc-nested", "k63-norc-disjoint-empty"):
        keys = sorted({key for a in shapes[n]["inputs"] for key in a.keys})
        hi, lo = [x >> 64 for x in keys], [x & (2**64 - 1) for x in keys]
        assert 0 in hi and any(lo.count(v) > 1 for v in set(lo)) == (shapes[n]["k"] > 33), n
        assert (max(hi) > 0) == (shapes[n]["k"] > 33) and max(lo) >> 63 == 1, n
        assert any(a ^ b < 4 for a, b in zip(keys, keys[1:])), n          # two keys that differ in their last base only
    # the key space of k = 5 exhausted by a weed set; exact thresholds where S * min_freq rounds above an integer
    assert len(M.expected("k5-norc-identical")["merged"].keys) == 256
    assert 50 * 0.58 < 29 and int(np.floor(50 * 0.58)) == 28 and 50 * 0.28 > 14 and int(np.floor(10 * 0.3)) == 3 and int(np.floor(5 * 0.6)) == 3 and int(np.floor(1 * 0.9)) == 0
    for n in M.CASES:
        e = M.expected(n)
        if e["case"]["k"] >= 15 and e["merged"].keys:                       # from k = 15 on the second window of a record is foreign
            assert M.weed_keys(e["merged"], e["sets"]["one-row"][1])[1] == 1, n
            assert M.weed_keys(e["merged"], e["sets"]["no-row"][1])[1] == 0, n
            assert 0 < M.weed_keys(e["merged"], e["sets"]["subset"][1])[1] < len(e["merged"].keys), n
        if e["merged"].keys:
            assert M.weed_keys(e["merged"], e["sets"]["every-row"][1])[1] == len(e["merged"].keys), n
    for n in [x for x in M.CASES if x.startswith("seq-")]:
        e = M.expected(n)
        removed = M.weed_keys(e["merged"], e["sets"]["fasta"][1])[1]
        assert 0 < removed < len(e["merged"].keys) and len(e["sets"]["fasta"][1]) > removed, n       # some foreign keys too


# ---- refusals: the same on both sides, the texts the reference panics with
def _refusal(model_call, oracle_call, text):
    with pytest.raises(M.Refused, match=text):
        model_call()
    with pytest.raises(ora.OracleError, match=text):
        oracle_call()


def test_refusals_agree():
    a, b = M.make_case("k31-nested-257-255")["inputs"]
    other_k = M.make_case("k15-64-65-1")["inputs"][2]
    other_strand = M.Arr(31, False, ["z"], a.keys[:3], a.var[:3, :1], a.counts[:3])
    # a mismatch as the third input
    _refusal(lambda: M.merge([a, b, M.Arr(15, True, *other_k[2:])]), lambda: ora.Array.merge([o_arr(a), o_arr(b), o_arr(M.Arr(15, True, *other_k[2:]))]),
             "K-mer lengths do not match: 15 31")
    _refusal(lambda: M.merge([a, b, other_strand]), lambda: ora.Array.merge([o_arr(a), o_arr(b), o_arr(other_strand)]), "Strand use inconsistent")
    two, three = by_names(a, ["a", "b"]), by_names(a, ["a", "b", "a"])
    for arr_, req, text in ((two, [], "Invalid number of samples to remove"), (two, ["a", "b"], "Invalid number of samples to remove"),
                            (two, ["a", "a"], "Invalid number of samples to remove"),           # the length test is on the raw list
                            (two, ["zzz"], r'Could not find sample\(s\): \{"zzz"\}'), (three, ["a", "q"], "Could not find sample")):
        _refusal(lambda: M.delete_samples(arr_, req), lambda: o_arr(arr_).delete_samples(req), text)
    # ["a", "a"] on three samples is one name: the first column called a goes, the second stays
    want = M.delete_samples(three, ["a", "a"])
    assert want.names == ["b", "a"] and np.array_equal(want.var[:, 1], M.by_key(_present_rows(three, [1, 2])).var[:, 1])
    o = o_arr(three)
    o.delete_samples(["a", "a"])
    agree(o, want, "repeated name", False)


def by_names(a, names):
    return M.Arr(a.k, a.rc, names, a.keys, a.var[:, :len(names)], M.present(a.var[:, :len(names)]))


def _present_rows(a, cols):
    sub = M.Arr(a.k, a.rc, [a.names[c] for c in cols], a.keys, a.var[:, cols], a.counts)
    return M._update_counts(sub, False)


# ---- the reference's own files
FIXTURES = ("merge.skf", "merge_k9.skf", "merge_k41.skf", "multidist.skf")


def _fixture(f):
    o = ora.Array.load(G.fin(f))
    return o, m_arr(o)


@pytest.mark.parametrize("fixture", FIXTURES)
def test_fixture_chains_model_equals_oracle(fixture, tmp_path):
    o, m = _fixture(fixture)
    partner = {"merge_k9.skf": "multidist.skf", "multidist.skf": "merge_k9.skf"}.get(fixture, fixture)     # same k; names repeat either way
    o2, m2 = _fixture(partner)
    om, mm = ora.Array.merge([o, o2, o]), M.merge([m, m2, m])
    agree(om, mm, "merge")
    first = mm.names[0]
    om.delete_samples([first, mm.names[1]])
    md = M.delete_samples(mm, [first, mm.names[1]])
    assert md.names[len(m.names) - 2:][:len(m2.names)] == m2.names       # the partner's columns stay: the first of each repeated name went
    agree(om, md, "delete")
    keys = md.keys[::2]
    for reverse in (False, True):
        for opts in (M.NO_FILTER, M.DEFAULTS, M.Opts((1.0, False, 1, False, False)), M.Opts((0.5, True, 3, True, True))):
            ow = ora.Array.merge([o, o2, o])
            ow.delete_samples([first, mm.names[1]])
            ow.weed_keys(M.key_dt(keys), reverse)
            ow.weed(None, False, **opts.kw())
            agree(ow, M.run_weed(md, keys, reverse, opts), ("weed", reverse, opts.ident()))


def _same_lines(text, golden):
    assert sorted(M.nk_lines(text).split("\n")) == sorted(M.nk_lines(golden).split("\n"))


def test_goldens_come_out_of_the_model():
    """the chains of tests/golden_cases.py::case_weed (skf_ops.rs:163-290) through the model: the reference's own outputs"""
    _, m = _fixture("merge.skf")
    wk = M.fasta_keys(G.fin("weed.fa"), m.k, m.rc)
    weeded = M.weed(m, wk)                                                 # default min_freq 0.9: floor(2 * 0.9) = 1
    again = M.weed(weeded, None, min_freq=1.0, filter_type=1)
    _same_lines("ska_version=x\n" + M.nk(again, True), G.correct("weed_nk.stdout").decode())
    _, m9 = _fixture("merge_k9.skf")
    _same_lines("ska_version=x\n" + M.nk(M.weed(m9, None, ambig_mask=True)), G.correct("weed_nk_k9.stdout").decode())
    _, m41 = _fixture("merge_k41.skf")
    got = M.weed(m41, None, min_freq=1.0, filter_type=3)
    _same_lines("ska_version=x\n" + M.nk(got, True), G.correct("weed_nk_k41.stdout").decode())
    # the alignments: columns in any order (the reference's rows are in hash order)
    import subset_model as SM
    for reverse, gold in ((False, "weed_align.stdout"), (True, "weed_align_reverse.stdout")):
        o = ora.Array.load(G.fin("merge.skf"))
        o.weed(G.fin("weed.fa"), reverse)
        assert M.same(m_arr(o), M.weed(m, wk, reverse)) is None, gold         # (a loaded file's rows are in its own order: no nk comparison)
        assert SM.fasta_columns(o.align()) == SM.fasta_columns(G.correct(gold))


# ---- mutation check: a wrong variant of each rule must disagree with the oracle on some case, or the case list cannot see the rule
def _first_catch(wrong):
    """the first (case, step) at which `wrong(case name)` -- a list of (step, model result, oracle result) -- differs"""
    for name in M.CASES:
        if name in M.LARGE:
            continue
        for step, mres, ores in wrong(name):
            if M.same(m_arr(ores), mres) is not None:
                return name, step
    return None


def _weed_variants(**wrong):
    def run(name):
        e = M.expected(name)
        for lab, reverse, opts in e["plan"]:
            keys = e["sets"][lab][1] if lab else None
            o = o_subject(e["case"])
            if lab:
                o.weed_keys(M.key_dt(keys), reverse)
            o.weed(None, False, **opts.kw())
            yield (lab, reverse, opts.ident()), M.run_weed(e["merged"], keys, reverse, opts, **wrong), o
    return run


def _delete_variants(**wrong):
    def run(name):
        e = M.expected(name)
        for lab, (req, _) in e["deletions"].items():
            o = o_subject(e["case"])
            o.delete_samples(req)
            yield lab, M.delete_samples(e["merged"], req, **wrong), o
    return run


def _merge_variant(name):
    case = M.make_case(name)
    if len(case["inputs"]) > 1:
        yield "merge", M.merge(case["inputs"], drop_empty_rows=True), o_subject(case)


@pytest.mark.parametrize("rule,wrong", [
    ("weed recounts instead of carrying the stored counts", _weed_variants(recount=True)),
    ("delete carries the stored counts instead of recounting", _delete_variants(carry_counts=True)),
    ("ceil instead of floor of S * min_freq", _weed_variants(ceil_threshold=True)),
    ("the last instead of the first column of a repeated name goes", _delete_variants(last_duplicate=True)),
    ("merge drops the rows no sample has", _merge_variant),
])
def test_a_wrong_rule_is_caught(rule, wrong):
    caught = _first_catch(wrong)
    print(f"{rule}: caught by {caught}")
    assert caught is not None, rule
