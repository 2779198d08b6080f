"""`ska map` on the device at its kernel, layout and option edges (`-m gpu`): Array.map against the oracle's text, byte for byte, on
the cases of tests/map_cases.py -- k = 5 ... 63 (half = 2 ... 31: a flank window over three presence words), 64- and 128-bit keys,
67 samples, 40 chromosomes, chromosome offsets on the presence-word and four-byte-group boundaries, record separators on the window
tile's edge, chromosomes without windows or without mapped k-mers, samples that miss whole chromosomes, every ambiguity code on both
strands, repeats of every kind.  tests/test_map_model.py shows on the CPU that the cases hold those edges and that the oracle's walk
equals the closed form the kernels compute.  All eight (format, --ambig-mask, --repeat-mask) combinations per case and array form."""
import functools

import pytest

import map_cases as MC

pytestmark = pytest.mark.gpu
NAMES = list(MC.CASES)


@pytest.fixture(scope="module")
def E():
    import skx_engine as eng
    eng.load_library()
    eng.default_context()
    return eng


@pytest.fixture(scope="module")
def world(E, tmp_path_factory):
    d = tmp_path_factory.mktemp("map_edges")

    @functools.lru_cache(maxsize=None)
    def get(name):
        c = MC.make_case(name)
        ref_path = c.write_ref(d)
        texts = c.oracle_texts(ref_path)
        ga = E.DictSet.build([E.record_stream(r) for r in c.samples], c.k, c.rc).merge(c.names)
        skf = str(d / (name + ".skf"))
        ga.save(skf)
        return c, ref_path, texts, {"engine_order": ga, "file_order": E.Array.load(skf)}
    return get


def _check(arr, ref_path, texts, **kw):
    for fmt, ambig_mask, repeat_mask in MC.GRID:
        got = arr.map(ref_path, fmt=fmt, ambig_mask=ambig_mask, repeat_mask=repeat_mask, **kw)
        want = texts[(fmt, ambig_mask, repeat_mask)]
        assert got == want, (fmt, ambig_mask, repeat_mask, MC.first_difference(got, want))


@pytest.mark.parametrize("form", ["engine_order", "file_order"])          # file order: the look-up kernels' `perm` path
@pytest.mark.parametrize("name", NAMES)
def test_map_edges_vs_oracle(world, name, form):
    c, ref_path, texts, arrays = world(name)
    _check(arrays[form], ref_path, texts)


@pytest.mark.parametrize("name", ["C31", "C33"])                          # one 64-bit and one 128-bit case
def test_map_materialises_a_lazily_held_array(E, world, tmp_path, name):
    c, ref_path, texts, _ = world(name)
    lazy = E.Array.build(c.write_samples(tmp_path), k=c.k, rc=c.rc, threads=2)
    _check(lazy, ref_path, texts)


def test_vcf_blocks_assembled_by_several_threads(world):
    c, ref_path, texts, arrays = world("C31")
    assert sum(c.layout["lens"]) > 2 * 4096                                # three blocks of 4 096 columns
    for g in [g for g in MC.GRID if g[0] == "vcf"]:
        one = arrays["engine_order"].map(ref_path, fmt="vcf", ambig_mask=g[1], repeat_mask=g[2], threads=1)
        five = arrays["engine_order"].map(ref_path, fmt="vcf", ambig_mask=g[1], repeat_mask=g[2], threads=5)
        assert one == five == texts[g], g
