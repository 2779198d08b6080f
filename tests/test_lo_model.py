"""tests/lo_model.py (the test-only restatement of `ska lo` with the engine's fixed orders) against the reference's own goldens
(tests/skalo.rs), byte for byte -- on the CPU oracle's reader, before anything on the device is compared with it."""
import os
import random

import pytest

import lo_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
IN = os.path.join(HERE, "golden", "input")
OK = os.path.join(HERE, "golden", "correct")


def _golden(name):
    with open(os.path.join(OK, name)) as f:
        return f.read()


def test_model_reproduces_snp_golden_with_reference():
    out, counts = M.run_skf(os.path.join(IN, "test_skalo.skf"), reference=os.path.join(IN, "test_skalo_reference.fas"))
    assert out["_snps.fas"] == _golden("test_skalo_snps.fas")
    assert set(out) == {"_snps.fas", "_pseudo_genomes.fas", "_snps.vcf", "_indels.vcf"}
    assert counts["snps"] == 3 and counts["unpositioned"] == 0


def test_model_reproduces_indel_golden():
    out, counts = M.run_skf(os.path.join(IN, "test_skalo_indel.skf"))
    assert out["_indels.vcf"] == _golden("test_skalo_indels.vcf")
    assert set(out) == {"_snps.fas", "_indels.vcf"}
    assert counts["indels"] == 1


def test_encoding_matches_the_reference():
    # bit_encoding.rs:123-166: A=0, C=1, T=2, G=3, first base high; rev_comp complements by XOR 2
    assert M.encode("ACTG") == 0b00011011
    assert M.decode(M.encode("GATTACA"), 7) == "GATTACA"
    assert M.rc(M.encode("AACG"), 4) == M.encode("CGTT")


def test_windows_equals_encode_of_every_window():
    rnd = random.Random(3)
    # n = 32 and 62: the (k - 1)-windows of k = 33 and k = 63; 'N' and '-' encode like the reference's (c >> 1) & 3
    for n in (1, 2, 4, 30, 31, 32, 40, 62, 63):
        for length in (0, n - 1, n, n + 1, 3 * n + 7):
            s = "".join(rnd.choice("ACGTACGTN-") for _ in range(max(length, 0)))
            assert M.windows(s, n) == [M.encode(s[i:i + n]) for i in range(len(s) - n + 1)], (n, length)
    assert M.windows("ACG", 4) == [] and M.windows("", 3) == []
    assert M.windows("ACGT", 4) == [M.encode("ACGT")]
    assert M.windows("ACG", 0) == [0, 0, 0, 0]


def test_single_sample_has_no_entry_node():
    keys = [M.encode("ACGTAC")]            # one split k-mer, k = 7
    with pytest.raises(M.NoEntry):
        M.run(keys, [b"A"], 7, ["s"])
