"""The model of `ska align --groups` (tests/subset_model.py) against the oracle chain it restates: a fresh ora.Array.from_dicts,
delete_samples(everybody outside the group), apply_filters, fasta -- per case, group and sampled option combination: equal column
multisets, the row count after the delete, the return value of apply_filters.  Runs on the CPU.  Also what keeps the GPU test of the
feature from being vacuous: in each of the three large cases every verdict class occurs, and no group's alignment is empty at
min_freq = 0 with no-const."""
import pytest

import subset_model as M


def test_grid_covers_every_option_value():
    assert len(M.GRID) == 12 and len(set(M.GRID)) == 12
    assert {o.min_freq for o in M.GRID} == {0.0, 0.6, 1.0}
    assert {o.filter_type for o in M.GRID} == {0, 1, 2, 3}
    for flag in ("filter_ambig_as_missing", "mask_ambig", "ignore_const_gaps"):
        assert {getattr(o, flag) for o in M.GRID} == {False, True}, flag
    assert M.GRID[0] == (0.0, False, 1, False, False)


def test_shapes_sit_on_the_kernels_edges():
    for case in M.LARGE_CASES:
        U = M.oracle_export(case).shape[0]
        assert U > 2 * 4096 and U % 16 != 0, (case, U)               # more than two compaction blocks, a partial 16-column group
    U = M.oracle_export("tiny").shape[0]
    assert U < 256 and U % 16 != 0, U


@pytest.mark.parametrize("case", list(M.CASES))
def test_model_equals_the_oracle_chain(case):
    var = M.oracle_export(case)
    U = var.shape[0]
    seen = {c: 0 for c in ("absent", "silent", "removed_freq", "removed_type", "kept")}
    for group in M.CASES[case]["groups"]:
        for opts in M.GRID:
            cols, counts = M.model(var, group, opts)
            o_cols, o_nrows, o_removed = M.oracle_chain(case, tuple(group), opts)
            where = (case, group, opts.ident())
            assert o_nrows == U - counts["absent"] == counts["rows_present"], where
            assert o_removed == counts["removed"], where
            assert len(o_cols) == counts["kept"] and o_cols == cols, where
            for c in seen:
                seen[c] += counts[c]
        # min_freq = 0 with no-const (GRID[0]): a group of two or more has sites.  One sample alone has one variant type per row, so
        # no-const keeps nothing of it (merge_ska_array.rs:322-334): its rows show without a filter
        cols, counts = M.model(var, group, M.GRID[0] if len(group) > 1 else M.Opts((0.0, False, 0, False, False)))
        assert counts["kept"] > 0, (case, group)
        if len(group) == 1:
            assert M.model(var, group, M.GRID[0])[1]["kept"] == 0
    if case in M.LARGE_CASES:
        assert all(seen.values()), (case, seen)
    print(case, "rows", U, seen)
