"""`ska map REFERENCE X.skf` through the executable (`-m gpu`) on the 64-bit case with more than 64 samples and on the narrowest
128-bit case of tests/map_cases.py: stdout is the oracle's text, and -o FILE holds the same bytes."""
import os
import subprocess

import pytest

import map_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKA = os.path.join(ROOT, "ska.rust_amd", "ska")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(SKA), reason="ska executable not built")]
OPTIONS = {"plain": ((), ("aln", False, False)), "vcf_masked": (("-f", "vcf", "--ambig-mask", "--repeat-mask"), ("vcf", True, True))}


def _run(*args, cwd=None):
    return subprocess.run([SKA, *args], cwd=cwd, capture_output=True, timeout=300)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_map_edges")
    out = {}
    for name in ("C31", "C33"):
        c = MC.make_case(name)
        oa = c.oracle_array()
        ref_path, skf = c.write_ref(d), str(d / (name + ".skf"))
        oa.save(skf)
        out[name] = (ref_path, skf, {o: oa.map(ref_path, fmt=g[0], ambig_mask=g[1], repeat_mask=g[2]) for o, (_, g) in OPTIONS.items()})
    return out


@pytest.mark.parametrize("options", list(OPTIONS))
@pytest.mark.parametrize("name", ["C31", "C33"])
def test_cli_map_edges(files, tmp_path, name, options):
    ref_path, skf, want = files[name]
    flags = OPTIONS[options][0]
    r = _run("map", ref_path, skf, *flags, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert r.stdout == want[options]
    r = _run("map", ref_path, skf, *flags, "-o", "map.out", cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert open(os.path.join(str(tmp_path), "map.out"), "rb").read() == want[options]
