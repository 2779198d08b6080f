"""ctypes binding of the MI355X split-k-mer engine (libskx.so: include/skx.h + include/skx_host.h).

The product path.  It never imports anything from oracle/ and has no CPU
fallback: if libskx.so is missing or no gfx950 device is usable, every call
raises.  The Python surface mirrors the reference's Rust API for the hot path
(SkaDict / build_and_merge / MergeSkaArray / generic_modes), so tests read like
the reference's own.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libskx.so")

QUAL_NOFILTER, QUAL_MIDDLE, QUAL_STRICT = 0, 1, 2
FILTER_NONE, FILTER_NO_CONST, FILTER_NO_AMBIG, FILTER_NO_AMBIG_OR_CONST = 0, 1, 2, 3
OK, EINVAL, EIO, ENODEV, ENOMEM, EEMPTY, EUNSUP, EFORMAT = range(8)

KEY_DT = np.dtype([("lo", "<u8"), ("hi", "<u8")])
DIST_DT = np.dtype([("distance", "<f8"), ("mismatch_prop", "<f8"), ("match_count", "<u8"), ("mismatch_count", "<u8")])
PAIR_DT = np.dtype([("i", "<u4"), ("j", "<u4"), ("d", DIST_DT)])      # skx_dist_pair
NJ_DT = np.dtype([("a", "<u4"), ("b", "<u4"), ("len_a", "<f8"), ("len_b", "<f8")])      # skx_nj_join
MARKER_DT = np.dtype([("row", "<u8"), ("group", "<u4"), ("n_in", "<u4"), ("n_out", "<u4"), ("kind", "u1"), ("bases_in", "u1"), ("bases_out", "u1"),
                      ("reserved", "u1")])                                               # skx_marker
MARKER_INFO_DT = np.dtype([("presence", "<u8"), ("allele", "<u8")])                      # skx_marker_info
MARKER_PRESENCE, MARKER_ALLELE = 1, 2
CURVE_TILE_ROWS, CURVE_LDS_STEPS, CURVE_BATCH_ORDERS = 4096, 1024, 1024      # SKX_CURVE_* (include/skx.h): the shape of skx_array_curve's kernel
SCREEN_TILE, SCREEN_SAMPLES = 1024, 256                                     # SKX_SCREEN_* (include/skx.h): the shape of skx_array_screen's kernel
QC_TILE_ROWS, QC_SAMPLES = 4096, 64                                          # SKX_QC_* (include/skx.h): the shape of skx_array_sample_qc's second kernel
QC_SAMPLE_DT = np.dtype([(f, "<u8") for f in ("kmers", "ambiguous", "singletons", "core_present", "private_alleles", "minor_alleles")])      # skx_qc_sample
QC_INFO_DT = np.dtype([(f, "<u8") for f in ("rows", "rows_present", "core_rows", "core_variant_rows", "threshold")])                           # skx_qc_info
QC_SAMPLES_TEXT, QC_SUMMARY_TEXT, QC_FLAGGED_TEXT = 0, 1, 2                     # SKH_QC_* (include/skx_host.h)
SCREEN_RECORD_DT = np.dtype([("length", "<u8"), ("windows", "<u8"), ("rows_hit", "<u8")])      # skx_screen_record
SCREEN_CELL_DT = np.dtype([("found", "<u4"), ("match", "<u4"), ("ambig", "<u4")])              # skx_screen_cell
SCREEN_PAIRS, SCREEN_SUMMARY, SCREEN_MATRIX = 0, 1, 2                       # SKH_SCREEN_* (include/skx_host.h)
DENSITY_TILE_ROWS, DENSITY_SAMPLES, DENSITY_SCAN_BLOCK = 4096, 64, 4096      # SKX_DENSITY_* (include/skx.h): the shapes of skx_array_snp_density's kernels
DENSITY_WANT_SNPS, DENSITY_DENSE_BIT = 1, 62
DENSITY_REGION_DT = np.dtype([(f, "<u4") for f in ("sample", "chrom", "start", "end", "snps")])                                                 # skx_density_region
DENSITY_SAMPLE_DT = np.dtype([(f, "<u8") for f in ("sites", "callable", "ambiguous", "missing", "snps", "dense_snps", "regions", "region_bases")])   # skx_density_sample
DENSITY_BIN_DT = np.dtype([("snps", "<u4"), ("dense_snps", "<u4")])                                                                             # skx_density_bin
DENSITY_INFO_DT = np.dtype([(f, "<u8") for f in ("windows", "repeat_windows", "sites", "n_chrom", "n_bins", "n_snps", "n_regions")])             # skx_density_info
DENSITY_REGIONS, DENSITY_SUMMARY, DENSITY_BINS, DENSITY_SNPS = 0, 1, 2, 3   # SKH_DENSITY_* (include/skx_host.h)
MASK_CHUNK, MASK_ALL_SAMPLES = 1024, 0xFFFFFFFF                             # SKX_MASK_* (include/skx.h): the items a workgroup of skx_array_mask_regions' kernel takes
MASK_INTERVAL_DT = np.dtype([(f, "<u4") for f in ("sample", "chrom", "start", "end")])                                                          # skx_mask_interval
MASK_SAMPLE_DT = np.dtype([("sites_in_regions", "<u8"), ("cells_masked", "<u8")])                                                              # skx_mask_sample
MASK_INFO_DT = np.dtype([(f, "<u8") for f in ("sites", "rows_in", "rows_all_samples", "rows_emptied", "rows_out", "n_intervals_merged")])       # skx_mask_info
PAIR_SITE_DT = np.dtype([("row", "<u8"), ("pair", "<u4"), ("base_i", "u1"), ("base_j", "u1"), ("reserved", "u1", (2,))])      # skx_pair_site
TREE_JOIN_DT = np.dtype([("a", "<u4"), ("b", "<u4")])                                                                        # skx_tree_join


class Qual(C.Structure):
    _fields_ = [("min_count", C.c_uint16), ("min_qual", C.c_uint8), ("qual_filter", C.c_int32)]


class Stream(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("qual", C.c_void_p), ("len", C.c_uint64)]


class FilterSpec(C.Structure):
    _fields_ = [("min_freq", C.c_double), ("filter_ambig_as_missing", C.c_int32), ("filter_type", C.c_int32), ("mask_ambig", C.c_int32),
                ("ignore_const_gaps", C.c_int32), ("two_stage", C.c_int32)]


class ArrayInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("rc", C.c_int32), ("k_bits", C.c_int32), ("n_kmers", C.c_uint64),
                ("n_rows", C.c_uint64), ("n_samples", C.c_uint64), ("total_samples", C.c_uint64)]


class Timings(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("hist", "scatter", "dedupe", "key_union", "assemble", "filter", "compact", "distance",
                                                 "append_probe", "append", "pieces_stats", "pieces_rows")]


class Job(C.Structure):
    """skh_job (include/skx_host.h): one build | align | distance job over the GPUs of a node"""
    _fields_ = [("names", C.POINTER(C.c_char_p)), ("file1", C.POINTER(C.c_char_p)), ("file2", C.POINTER(C.c_char_p)), ("n_samples", C.c_int),
                ("k", C.c_int), ("rc", C.c_int), ("qual", Qual), ("threads", C.c_int), ("proportion_reads", C.c_double),
                ("output", C.c_char_p), ("merge_parts", C.c_int), ("min_freq", C.c_double),
                ("filter_type", C.c_int), ("mask_ambig", C.c_int), ("ignore_const_gaps", C.c_int), ("filter_ambig_as_missing", C.c_int),
                ("filt_ambig", C.c_int), ("extras", C.c_void_p)]


class DistExtras(C.Structure):
    """skh_dist_extras (include/skx_host.h): what `ska distance` writes besides its table"""
    _fields_ = [("tree", C.c_char_p), ("clusters", C.c_char_p), ("cluster_snps", C.c_double), ("cluster_mismatches", C.c_double)]


class SelectSpec(C.Structure):
    """skx_select_spec (include/skx.h): the criteria of `ska distance --max-snps / --max-mismatches / --closest`; a negative threshold / 0 = not given"""
    _fields_ = [("max_snps", C.c_double), ("max_mismatches", C.c_double), ("closest", C.c_int32), ("band_rows", C.c_int32)]

    @classmethod
    def of(cls, max_snps=None, max_mismatches=None, closest=0, band_rows=0):
        return cls(-1.0 if max_snps is None else float(max_snps), -1.0 if max_mismatches is None else float(max_mismatches), int(closest), int(band_rows))


class SelectInfo(C.Structure):
    """skx_select_info (include/skx.h)"""
    _fields_ = [("bands", C.c_uint64), ("band_rows", C.c_uint64), ("count_buffer_bytes", C.c_uint64), ("candidates", C.c_uint64)]


class MstSpec(C.Structure):
    """skx_mst_spec (include/skx.h): the thresholds of `ska distance --mst` (a negative one = not given) and the band of its sweep"""
    _fields_ = [("max_snps", C.c_double), ("max_mismatches", C.c_double), ("band_rows", C.c_int32)]

    @classmethod
    def of(cls, max_snps=None, max_mismatches=None, band_rows=0):
        return cls(-1.0 if max_snps is None else float(max_snps), -1.0 if max_mismatches is None else float(max_mismatches), int(band_rows))


class MstInfo(C.Structure):
    """skx_mst_info (include/skx.h)"""
    _fields_ = [(f, C.c_uint64) for f in ("bands", "band_rows", "count_buffer_bytes", "candidates", "edges", "components", "rounds")]


class BandedSpec(C.Structure):
    """skx_banded_spec (include/skx.h): the cluster thresholds of `ska distance --no-table --clusters` and the band of its sweep"""
    _fields_ = [("cluster_snps", C.c_double), ("cluster_mismatches", C.c_double), ("band_rows", C.c_int32)]


class BandedInfo(C.Structure):
    """skx_banded_info (include/skx.h)"""
    _fields_ = [("bands", C.c_uint64), ("band_rows", C.c_uint64), ("count_buffer_bytes", C.c_uint64), ("edges", C.c_uint64), ("clusters", C.c_uint64)]


class SubsetInfo(C.Structure):
    """skx_subset_info (include/skx.h): what Array.subset_filtered did"""
    _fields_ = [("rows_present", C.c_uint64), ("removed", C.c_uint64), ("silent", C.c_uint64), ("sites", C.c_uint64)]


class DensityResult(C.Structure):
    """skx_density_result (include/skx.h)"""
    _fields_ = [("info", C.c_uint64 * 7), ("samples", C.c_void_p), ("regions", C.c_void_p), ("bins", C.c_void_p), ("chrom_ids", C.c_void_p),
                ("chrom_lens", C.c_void_p), ("snps", C.c_void_p), ("snp_ref", C.c_void_p)]


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[skx {code}] {msg}")
        self.code = code


# every symbol include/skx.h and include/skx_host.h declare
SYMBOLS = """skx_last_error skx_version skx_ctx_create skx_ctx_destroy skx_ctx_sync skx_ctx_stream skx_dictset_build
skx_dictset_build_files skx_read_records skx_dictset_free skx_dictset_nsamples skx_dictset_key_bits skx_dictset_size skx_dictset_export
skx_keyset_union skx_keyset_union_notes skx_keyset_size skx_keyset_device skx_keyset_from_device skx_keyset_merge skx_keyset_free
skx_array_assemble skx_array_assemble_lazy skx_merge skx_build_and_merge skx_array_free skx_array_save skx_array_load skx_array_from_host
skx_array_info skx_array_name skx_array_version skx_array_export skx_array_sample_kmers skx_array_pieces_info skx_array_filter
skx_array_write_fasta skx_array_fasta skx_array_device_matrix skx_array_device_stats skx_array_set_total_samples skx_array_distance skx_free skx_ctx_timings skx_ctx_merge_path
skx_array_merge skx_array_delete_samples skx_array_weed skx_keyset_from_fasta skx_array_ctx skx_set_last_error skx_array_map skx_cov_histogram skx_phases_json skx_phase_add skx_skf_peek_k skx_array_load_filtered skx_ctx_expect_output skx_array_distance_planes skx_planes_distance skx_array_distance_filtered
skx_comm_unique_id skx_comm_create skx_comm_create_local skx_comm_destroy skx_comm_rank skx_comm_world skx_comm_bytes_received skx_comm_transport skx_comm_barrier
skx_comm_allgather skx_comm_allreduce_u32 skx_comm_gather_root skx_shard_range skx_pair_bands skx_keyset_allgather skx_array_reduce_stats skx_array_distance_sharded
skh_build_sharded skh_align_sharded skh_distance_sharded
skh_apply_filters skh_align skh_align_fd skh_distance_tsv skh_nk skh_save_skf skh_load_array skh_sample_name skh_main skh_merge skh_delete skh_weed skh_cov skh_cov_fit skh_align_inputs_fd skh_distance_skf_tsv skh_help skh_log
skx_array_lo_graph skx_lo_graph_info skx_lo_graph_export skx_lo_gather skx_lo_graph_free skh_lo
skx_dist_nj skx_matrix_nj skh_nj_newick skh_distance_clusters skh_distance_skf_tsv_extras
skx_array_distance_query skx_array_distance_query_filtered skh_distance_query_tsv
skx_array_distance_select skx_array_distance_select_prefiltered skh_distance_select_tsv
skx_array_distance_banded skx_array_distance_banded_prefiltered skh_clusters_csv skh_cluster_cutoffs skh_distance_banded_files
skx_array_subset_filtered skh_read_groups skh_align_groups skh_align_samples_fd
skx_array_distance_mst skx_array_distance_mst_prefiltered skh_distance_mst_tsv skh_mst_levels_csv
skx_ctx_filter_cut
skx_array_group_markers skh_markers skh_key_arms
skx_array_pair_sites skh_distance_sites
skx_array_curve skh_curve skh_curve_orders skh_curve_tsv
skx_array_screen skh_screen skh_screen_text
skx_array_sample_qc skh_qc skh_qc_text
skx_array_snp_density skh_density skh_density_text skh_density_mask_alignment
skx_array_mask_regions skx_reference_records skh_mask skh_mask_text skh_mask_read_regions skh_mask_read_bed
skh_newick_joins skh_parsimony_newick skh_parsimony_branches""".split()

_lib = None


def load_library():
    """Load libskx.so (no GPU needed for loading); fails loudly when the extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"(make -C ska.rust_amd). There is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    vp, cp, i, d, u64 = C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_uint64
    pp = C.POINTER(vp)
    lib.skx_last_error.restype = cp
    lib.skx_version.restype = cp
    lib.skx_ctx_create.argtypes = [i, pp]
    lib.skx_array_lo_graph.argtypes = [vp, pp]
    lib.skx_lo_graph_info.argtypes = [vp, C.POINTER(LoInfo)]
    lib.skx_lo_graph_export.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.skx_lo_gather.argtypes = [vp, vp, u64, vp, vp]
    lib.skx_lo_graph_free.argtypes = [vp]
    lib.skh_lo.argtypes = [vp, cp, cp, cp, C.c_float, C.c_size_t, C.c_size_t, i]
    lib.skx_dist_nj.argtypes = [vp, vp, i, vp]
    lib.skx_matrix_nj.argtypes = [vp, vp, i, vp]
    lib.skh_nj_newick.argtypes = [C.POINTER(cp), vp, i, pp, C.POINTER(u64)]
    lib.skh_distance_clusters.argtypes = [C.POINTER(cp), vp, i, d, d, pp, C.POINTER(u64), pp, C.POINTER(u64)]
    lib.skh_distance_skf_tsv_extras.argtypes = [vp, cp, d, i, C.POINTER(DistExtras), pp, C.POINTER(u64)]
    lib.skx_array_distance_query.argtypes = [vp, d, i, vp, i, vp]
    lib.skx_array_distance_query_filtered.argtypes = [vp, d, i, vp, i, vp, C.POINTER(C.c_int64), C.POINTER(u64)]
    lib.skh_distance_query_tsv.argtypes = [vp, cp, cp, C.POINTER(cp), i, d, i, pp, C.POINTER(u64)]
    lib.skx_array_distance_select.argtypes = [vp, d, i, C.POINTER(SelectSpec), pp, C.POINTER(u64), C.POINTER(C.c_int64), C.POINTER(u64), C.POINTER(SelectInfo)]
    lib.skx_array_distance_select_prefiltered.argtypes = [vp, C.c_int64, i, C.POINTER(SelectSpec), pp, C.POINTER(u64), C.POINTER(SelectInfo)]
    lib.skh_distance_select_tsv.argtypes = [vp, cp, d, i, C.POINTER(SelectSpec), pp, C.POINTER(u64)]
    lib.skx_array_distance_banded.argtypes = [vp, d, i, C.POINTER(BandedSpec), vp, vp, C.POINTER(C.c_int64), C.POINTER(u64), C.POINTER(BandedInfo)]
    lib.skx_array_distance_banded_prefiltered.argtypes = [vp, C.c_int64, i, C.POINTER(BandedSpec), vp, vp, C.POINTER(BandedInfo)]
    lib.skh_clusters_csv.argtypes = [C.POINTER(cp), vp, i, pp, C.POINTER(u64)]
    lib.skh_cluster_cutoffs.argtypes = [d, d, i, C.POINTER(u64), C.POINTER(d)]
    lib.skh_distance_banded_files.argtypes = [vp, cp, d, i, C.POINTER(DistExtras)]
    lib.skx_array_distance_mst.argtypes = [vp, d, i, C.POINTER(MstSpec), pp, C.POINTER(u64), C.POINTER(C.c_int64), C.POINTER(u64), C.POINTER(MstInfo)]
    lib.skx_array_distance_mst_prefiltered.argtypes = [vp, C.c_int64, i, C.POINTER(MstSpec), pp, C.POINTER(u64), C.POINTER(MstInfo)]
    lib.skh_distance_mst_tsv.argtypes = [vp, cp, d, i, C.POINTER(MstSpec), pp, C.POINTER(u64)]
    lib.skh_mst_levels_csv.argtypes = [C.POINTER(cp), vp, u64, i, vp, i, pp, C.POINTER(u64)]
    lib.skx_array_subset_filtered.argtypes = [vp, vp, i, C.POINTER(FilterSpec), pp, C.POINTER(SubsetInfo)]
    lib.skh_read_groups.argtypes = [cp, pp, C.POINTER(u64), C.POINTER(u64)]
    lib.skh_align_groups.argtypes = [vp, C.POINTER(cp), i, i, i, i, i, d, i, cp, i, cp]
    lib.skh_align_samples_fd.argtypes = [vp, C.POINTER(cp), i, i, i, i, i, d, i, C.POINTER(cp), i, i]
    lib.skx_array_group_markers.argtypes = [vp, vp, i, vp, d, d, i, pp, pp, C.POINTER(u64), vp]
    lib.skh_markers.argtypes = [vp, cp, cp, cp, d, d, i, i, i]
    lib.skh_key_arms.argtypes = [vp, i, cp, cp]
    lib.skh_key_arms.restype = None
    lib.skx_array_pair_sites.argtypes = [vp, d, vp, u64, u64, pp, pp, vp, C.POINTER(u64)]
    lib.skh_distance_sites.argtypes = [vp, cp, d, C.POINTER(SelectSpec), C.POINTER(MstSpec), cp, u64, pp, C.POINTER(u64)]
    lib.skx_array_curve.argtypes = [vp, vp, C.c_uint32, d, vp]
    lib.skh_curve_orders.argtypes = [u64, C.c_uint32, C.c_uint32, vp]
    lib.skh_curve_tsv.argtypes = [vp, C.c_uint32, C.c_uint32, pp, C.POINTER(u64)]
    lib.skh_curve.argtypes = [vp, cp, cp, C.c_uint32, u64, d, cp, i]
    lib.skx_array_screen.argtypes = [vp, cp, C.POINTER(u64), pp, pp, pp]
    lib.skh_screen_text.argtypes = [i, u64, vp, vp, vp, C.POINTER(cp), u64, d, d, pp, C.POINTER(u64)]
    lib.skh_screen.argtypes = [vp, cp, cp, cp, d, d, i]
    lib.skx_array_sample_qc.argtypes = [vp, d, vp, vp]
    lib.skh_qc_text.argtypes = [i, vp, C.POINTER(cp), u64, vp, d, pp, C.POINTER(u64)]
    lib.skh_qc.argtypes = [vp, cp, cp, d, d]
    lib.skx_array_snp_density.argtypes = [vp, cp, u64, C.c_uint32, i, C.POINTER(DensityResult)]
    lib.skh_density_text.argtypes = [i, C.POINTER(DensityResult), C.POINTER(cp), u64, u64, pp, C.POINTER(u64)]
    lib.skh_density_mask_alignment.argtypes = [vp, u64, C.POINTER(DensityResult), C.POINTER(cp), u64]
    lib.skh_density.argtypes = [vp, cp, cp, cp, u64, C.c_uint32, i, cp]
    lib.skx_array_mask_regions.argtypes = [vp, cp, vp, u64, vp, vp]
    lib.skx_reference_records.argtypes = [cp, pp, pp, C.POINTER(u64)]
    lib.skh_mask_read_regions.argtypes = [cp, u64, C.POINTER(cp), u64, C.POINTER(cp), vp, u64, pp, C.POINTER(u64)]
    lib.skh_mask_read_bed.argtypes = [cp, u64, C.POINTER(cp), vp, u64, pp, C.POINTER(u64)]
    lib.skh_mask_text.argtypes = [vp, vp, vp, u64, C.POINTER(cp), u64, pp, C.POINTER(u64)]
    lib.skh_mask.argtypes = [vp, cp, cp, cp, cp, i, u64, C.c_uint32, cp, cp]
    lib.skh_newick_joins.argtypes = [cp, C.POINTER(cp), i, vp, C.POINTER(i)]
    lib.skh_parsimony_newick.argtypes = [C.POINTER(cp), vp, i, i, vp, pp, C.POINTER(u64)]
    lib.skh_parsimony_branches.argtypes = [C.POINTER(cp), vp, i, i, vp, pp, C.POINTER(u64)]
    lib.skx_ctx_destroy.argtypes = [vp]
    lib.skx_ctx_sync.argtypes = [vp]
    lib.skx_ctx_stream.argtypes = [vp]
    lib.skx_ctx_stream.restype = vp
    lib.skx_ctx_timings.argtypes = [vp, C.POINTER(Timings), i]
    lib.skx_ctx_merge_path.argtypes = [vp]
    lib.skx_ctx_merge_path.restype = C.c_char_p
    lib.skx_ctx_filter_cut.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.skx_dictset_build.argtypes = [vp, C.POINTER(Stream), i, i, i, i, C.POINTER(Qual), pp]
    lib.skx_dictset_build_files.argtypes = [vp, C.POINTER(cp), C.POINTER(cp), i, i, i, C.POINTER(Qual), i, d, pp]
    lib.skx_dictset_free.argtypes = [vp]
    lib.skx_dictset_nsamples.argtypes = [vp]
    lib.skx_dictset_key_bits.argtypes = [vp]
    lib.skx_dictset_size.argtypes = [vp, i, C.POINTER(u64)]
    lib.skx_dictset_export.argtypes = [vp, i, vp, vp, u64]
    lib.skx_keyset_union.argtypes = [vp, vp, pp]
    lib.skx_keyset_union_notes.argtypes = [vp, vp, pp]
    lib.skx_keyset_size.argtypes = [vp, C.POINTER(u64)]
    lib.skx_keyset_device.argtypes = [vp, pp, C.POINTER(u64), C.POINTER(i)]
    lib.skx_keyset_from_device.argtypes = [vp, vp, u64, i, i, pp]
    lib.skx_keyset_merge.argtypes = [vp, pp, i, pp]
    lib.skx_keyset_free.argtypes = [vp]
    lib.skx_array_assemble.argtypes = [vp, vp, vp, C.POINTER(cp), pp]
    lib.skx_array_assemble_lazy.argtypes = [vp, vp, vp, C.POINTER(cp), pp]
    lib.skx_merge.argtypes = [vp, vp, C.POINTER(cp), pp]
    lib.skx_build_and_merge.argtypes = [vp, C.POINTER(cp), C.POINTER(cp), C.POINTER(cp), i, i, i, C.POINTER(Qual), i, d, pp]
    lib.skx_array_free.argtypes = [vp]
    lib.skx_array_save.argtypes = [vp, cp]
    lib.skx_array_load.argtypes = [vp, cp, i, pp]
    lib.skx_array_from_host.argtypes = [vp, i, i, C.POINTER(cp), i, vp, vp, vp, u64, cp, pp]
    lib.skx_array_info.argtypes = [vp, C.POINTER(ArrayInfo)]
    lib.skx_array_name.argtypes = [vp, u64]
    lib.skx_array_name.restype = cp
    lib.skx_array_version.argtypes = [vp]
    lib.skx_array_version.restype = cp
    lib.skx_array_export.argtypes = [vp, vp, vp, vp]
    lib.skx_array_sample_kmers.argtypes = [vp, vp]
    lib.skx_array_pieces_info.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_uint32)]
    lib.skx_array_filter.argtypes = [vp, u64, i, i, i, i, i, C.POINTER(C.c_int32)]
    lib.skx_array_write_fasta.argtypes = [vp, i]
    lib.skx_array_fasta.argtypes = [vp, pp, C.POINTER(u64)]
    lib.skx_array_device_matrix.argtypes = [vp, pp, C.POINTER(u64), C.POINTER(u64)]
    lib.skx_array_device_stats.argtypes = [vp, pp, pp, pp, pp]
    lib.skx_array_set_total_samples.argtypes = [vp, u64]
    lib.skx_array_distance.argtypes = [vp, d, i, vp]
    lib.skx_free.argtypes = [vp]
    lib.skh_apply_filters.argtypes = [vp, d, i, i, i, i, C.POINTER(C.c_int32)]
    lib.skh_align.argtypes = [vp, i, i, i, d, i, pp, C.POINTER(u64)]
    lib.skh_distance_tsv.argtypes = [vp, d, i, pp, C.POINTER(u64)]
    lib.skh_nk.argtypes = [vp, i, pp, C.POINTER(u64)]
    lib.skh_save_skf.argtypes = [vp, cp]
    lib.skh_load_array.argtypes = [vp, C.POINTER(cp), i, i, pp]
    lib.skx_array_merge.argtypes = [vp, pp, i, pp]
    lib.skx_array_delete_samples.argtypes = [vp, C.POINTER(cp), i]
    lib.skx_array_weed.argtypes = [vp, vp, i, C.POINTER(u64)]
    lib.skx_keyset_from_fasta.argtypes = [vp, cp, i, i, pp]
    lib.skx_array_map.argtypes = [vp, cp, i, i, i, i, pp, C.POINTER(u64)]
    lib.skx_cov_histogram.argtypes = [vp, cp, cp, i, i, vp]
    lib.skh_cov.argtypes = [vp, cp, cp, i, i, pp, C.POINTER(u64), C.POINTER(u64)]
    lib.skh_cov_fit.argtypes = [vp, u64, C.POINTER(d), C.POINTER(d), C.POINTER(u64)]
    lib.skx_array_ctx.argtypes = [vp]
    lib.skx_array_ctx.restype = vp
    lib.skx_set_last_error.argtypes = [cp]
    lib.skh_merge.argtypes = [vp, C.POINTER(cp), i, cp]
    lib.skh_delete.argtypes = [vp, C.POINTER(cp), i, cp]
    lib.skh_weed.argtypes = [vp, cp, i, d, i, i, i, i, cp]
    lib.skx_read_records.argtypes = [cp, cp, d, i, pp, pp, C.POINTER(u64)]
    lib.skh_sample_name.argtypes = [cp]
    lib.skh_sample_name.restype = vp
    lib.skx_ctx_expect_output.argtypes = [vp, i]
    lib.skx_array_distance_planes.argtypes = [vp, i, pp, C.POINTER(u64), C.POINTER(i)]
    lib.skx_planes_distance.argtypes = [vp, vp, i, u64, i, d, i, i, vp]
    lib.skx_array_distance_filtered.argtypes = [vp, d, i, vp, C.POINTER(C.c_int64), C.POINTER(u64)]
    lib.skx_array_load_filtered.argtypes = [vp, cp, C.POINTER(FilterSpec), pp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.skh_align_inputs_fd.argtypes = [vp, C.POINTER(cp), i, i, i, i, i, d, i, i]
    lib.skh_distance_skf_tsv.argtypes = [vp, cp, d, i, pp, C.POINTER(u64)]
    lib.skx_phases_json.argtypes = [pp, C.POINTER(u64), i]
    lib.skx_phase_add.argtypes = [cp, d]
    lib.skx_phase_add.restype = None
    lib.skx_comm_unique_id.argtypes = [vp]
    lib.skx_comm_create.argtypes = [vp, i, i, vp, pp]
    lib.skx_comm_create_local.argtypes = [vp, i, i, cp, pp]
    lib.skx_comm_destroy.argtypes = [vp]
    lib.skx_comm_destroy.restype = None
    lib.skx_comm_rank.argtypes = [vp]
    lib.skx_comm_world.argtypes = [vp]
    lib.skx_comm_bytes_received.argtypes = [vp]
    lib.skx_comm_bytes_received.restype = u64
    lib.skx_comm_transport.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    lib.skx_comm_barrier.argtypes = [vp]
    lib.skx_comm_allgather.argtypes = [vp, vp, vp, u64, i]
    lib.skx_comm_allreduce_u32.argtypes = [vp, vp, u64, i]
    lib.skx_comm_gather_root.argtypes = [vp, vp, vp, vp]
    lib.skx_shard_range.argtypes = [u64, i, i, C.POINTER(u64), C.POINTER(u64)]
    lib.skx_pair_bands.argtypes = [i, i, i, vp]
    lib.skx_keyset_allgather.argtypes = [vp, vp, pp]
    lib.skx_array_reduce_stats.argtypes = [vp, vp, u64]
    lib.skx_array_distance_sharded.argtypes = [vp, vp, i, d, vp, u64]
    lib.skh_build_sharded.argtypes = [vp, vp, C.POINTER(Job)]
    lib.skh_align_sharded.argtypes = [vp, vp, C.POINTER(Job)]
    lib.skh_distance_sharded.argtypes = [vp, vp, C.POINTER(Job)]
    _lib = lib
    return lib


def _check(rc):
    if rc != OK:
        raise EngineError(rc, _lib.skx_last_error().decode())


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _take(ptr, n):
    s = C.string_at(ptr, n.value)
    _lib.skx_free(ptr)
    return s


def qual(min_count=5, min_qual=20, qual_filter=QUAL_STRICT):
    return Qual(min_count, min_qual, qual_filter)


def curve_orders(seed, n_samples, n_orders):
    """skh_curve_orders: the seeded orders of `ska curve` (host only) -> int32 [n_orders, n_samples]"""
    load_library()
    o = np.zeros((n_orders, n_samples), np.int32)
    _check(_lib.skh_curve_orders(int(seed), int(n_samples), int(n_orders), _np_ptr(o)))
    return o


def curve_tsv(counts):
    """skh_curve_tsv: the text of <PREFIX>.curve.tsv from counts [P, S, 4] (host only)"""
    load_library()
    c = np.ascontiguousarray(counts, np.uint64)
    p, n = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_curve_tsv(_np_ptr(c), c.shape[0], c.shape[1], C.byref(p), C.byref(n)))
    return _take(p, n).decode()


def screen_text(which, ids, records, cells, names, min_cover=0.9, min_identity=0.0):
    """skh_screen_text: one of the three texts of `ska screen` (SCREEN_PAIRS, SCREEN_SUMMARY, SCREEN_MATRIX) from what Array.screen returns
    (host only)"""
    load_library()
    rec = np.ascontiguousarray(records, SCREEN_RECORD_DT)
    cel = np.ascontiguousarray(cells, SCREEN_CELL_DT).reshape(len(rec), len(names))
    blob = b"".join(x.encode() + b"\0" for x in ids)
    nm = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    p, n = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_screen_text(int(which), len(rec), _np_ptr(rec), blob, _np_ptr(cel), nm, len(names), float(min_cover), float(min_identity),
                                C.byref(p), C.byref(n)))
    return _take(p, n).decode()


def qc_text(which, samples, names, info, mad=5.0):
    """skh_qc_text: one of the three texts of `ska qc` (QC_SAMPLES_TEXT, QC_SUMMARY_TEXT, QC_FLAGGED_TEXT) from what Array.sample_qc returns
    (host only)"""
    load_library()
    rec = np.ascontiguousarray(samples, QC_SAMPLE_DT).reshape(len(names))
    inf = np.ascontiguousarray(info, QC_INFO_DT).reshape(1)
    nm = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    p, n = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_qc_text(int(which), _np_ptr(rec), nm, len(names), _np_ptr(inf), float(mad), C.byref(p), C.byref(n)))
    return _take(p, n).decode()


def _density_struct(res):
    """a skx_density_result over the arrays of what Array.snp_density returns -> (struct, what must stay alive while it is used)"""
    info = np.ascontiguousarray(res["info"], DENSITY_INFO_DT).reshape(1)
    keep = [np.ascontiguousarray(res["samples"], DENSITY_SAMPLE_DT), np.ascontiguousarray(res["regions"], DENSITY_REGION_DT),
            np.ascontiguousarray(res["bins"], DENSITY_BIN_DT), C.create_string_buffer(b"".join(x.encode() + b"\0" for x in res["chrom_ids"]) + b"\0"),
            np.ascontiguousarray(res["chrom_lens"], np.uint64)]
    r = DensityResult()
    for j, f in enumerate(DENSITY_INFO_DT.names):
        r.info[j] = int(info[0][f])
    r.samples, r.regions, r.bins, r.chrom_lens = _np_ptr(keep[0]), _np_ptr(keep[1]), _np_ptr(keep[2]), _np_ptr(keep[4])
    r.chrom_ids = C.cast(keep[3], C.c_void_p)
    if res.get("snps") is not None:
        keep += [np.ascontiguousarray(res["snps"], np.uint64), np.ascontiguousarray(res["snp_ref"], np.uint8)]
        r.snps, r.snp_ref = _np_ptr(keep[5]), _np_ptr(keep[6])
    return r, keep


def density_text(which, res, names, window=1000):
    """skh_density_text: one of the four texts of `ska density` (DENSITY_REGIONS, DENSITY_SUMMARY, DENSITY_BINS, DENSITY_SNPS) from what
    Array.snp_density returns (host only)"""
    load_library()
    r, keep = _density_struct(res)
    nm = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    p, n = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_density_text(int(which), C.byref(r), nm, len(names), int(window), C.byref(p), C.byref(n)))
    return _take(p, n).decode()


def _mask_intervals(intervals):
    """[(sample | MASK_ALL_SAMPLES, chrom, start, end)] or a MASK_INTERVAL_DT array -> a contiguous MASK_INTERVAL_DT array"""
    if isinstance(intervals, np.ndarray) and intervals.dtype == MASK_INTERVAL_DT:
        return np.ascontiguousarray(intervals)
    return np.array([tuple(int(x) for x in q) for q in intervals], MASK_INTERVAL_DT)


def _take_intervals(p, n):
    out = np.frombuffer(C.string_at(p, n.value * MASK_INTERVAL_DT.itemsize), MASK_INTERVAL_DT).copy() if n.value else np.zeros(0, MASK_INTERVAL_DT)
    _lib.skx_free(p)
    return out


def mask_read_regions(text, names, chrom_ids, chrom_lens):
    """skh_mask_read_regions: the text (bytes) of a regions file -> MASK_INTERVAL_DT array, 0-based inclusive (host only)"""
    load_library()
    nm = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    ids = (C.c_char_p * max(len(chrom_ids), 1))(*[x.encode() for x in chrom_ids])
    lens = np.ascontiguousarray(chrom_lens, np.uint64)
    buf = C.create_string_buffer(bytes(text), len(text)) if len(text) else None           # (exactly len bytes: no terminator is promised)
    p, n = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_mask_read_regions(C.cast(buf, C.c_char_p), len(text), nm, len(names), ids, _np_ptr(lens), len(chrom_ids), C.byref(p), C.byref(n)))
    return _take_intervals(p, n)


def mask_read_bed(text, chrom_ids, chrom_lens):
    """skh_mask_read_bed: the text (bytes) of a BED file -> MASK_INTERVAL_DT array of ALL intervals, 0-based inclusive (host only)"""
    load_library()
    ids = (C.c_char_p * max(len(chrom_ids), 1))(*[x.encode() for x in chrom_ids])
    lens = np.ascontiguousarray(chrom_lens, np.uint64)
    buf = C.create_string_buffer(bytes(text), len(text)) if len(text) else None
    p, n = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_mask_read_bed(C.cast(buf, C.c_char_p), len(text), ids, _np_ptr(lens), len(chrom_ids), C.byref(p), C.byref(n)))
    return _take_intervals(p, n)


def mask_text(samples, info, intervals, names):
    """skh_mask_text: PREFIX.mask.summary.tsv from what Array.mask_regions returned for `intervals` (host only)"""
    load_library()
    sm = np.ascontiguousarray(samples, MASK_SAMPLE_DT)
    inf = np.ascontiguousarray(info, MASK_INFO_DT).reshape(1)
    iv = _mask_intervals(intervals)
    nm = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    p, n = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_mask_text(_np_ptr(sm) if len(sm) else None, _np_ptr(inf), _np_ptr(iv) if len(iv) else None, len(iv), nm, len(names), C.byref(p), C.byref(n)))
    out = C.string_at(p, n.value).decode()
    _lib.skx_free(p)
    return out


def reference_records(path):
    """skx_reference_records: (ids, lengths as uint64) of a FASTA reference's records (host only)"""
    load_library()
    pi, pl, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    _check(_lib.skx_reference_records(os.fsencode(path), C.byref(pi), C.byref(pl), C.byref(n)))
    lens = np.frombuffer(C.string_at(pl, n.value * 8), np.uint64).copy() if n.value else np.zeros(0, np.uint64)
    ids, at = [], pi.value
    for _ in range(n.value):
        s = C.string_at(at)
        ids.append(s.decode())
        at += len(s) + 1
    _lib.skx_free(pi)
    _lib.skx_free(pl)
    return ids, lens


def density_mask_alignment(aln, res, names):
    """skh_density_mask_alignment: `ska map`'s alignment (bytes, format aln) with every sample's regions overwritten by 'N' (host only)"""
    load_library()
    r, keep = _density_struct(res)
    nm = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    buf = C.create_string_buffer(bytes(aln), len(aln))
    _check(_lib.skh_density_mask_alignment(C.cast(buf, C.c_void_p), len(aln), C.byref(r), nm, len(names)))
    return buf.raw


def cov_histogram(fq1, fq2, k=31, rc=True, ctx=None):
    """CoverageHistogram::new + histogram (coverage.rs:70-148,158-163) on the device."""
    ctx = ctx or default_context()
    h = np.zeros(1000, np.uint32)
    _check(_lib.skx_cov_histogram(ctx.h, fq1.encode(), fq2.encode(), k, int(rc), _np_ptr(h)))
    return h


def cov_fit(counts):
    c = np.ascontiguousarray(counts, np.float64)
    w0, cc, cut = C.c_double(), C.c_double(), C.c_uint64()
    load_library()
    _check(_lib.skh_cov_fit(_np_ptr(c), len(c), C.byref(w0), C.byref(cc), C.byref(cut)))
    return w0.value, cc.value, cut.value


def cov(fq1, fq2, k=31, rc=True, ctx=None):
    """`ska cov`: (plot_hist text, cutoff)"""
    ctx = ctx or default_context()
    p, n, cut = C.c_void_p(), C.c_uint64(), C.c_uint64()
    _check(_lib.skh_cov(ctx.h, fq1.encode(), fq2.encode(), k, int(rc), C.byref(p), C.byref(n), C.byref(cut)))
    return _take(p, n), cut.value


def phases(reset=False):
    """Wall-clock phases of the host path recorded since the last reset: {name: seconds} in first-use order."""
    import json
    buf, n = C.c_void_p(), C.c_uint64()
    _check(_lib.skx_phases_json(C.byref(buf), C.byref(n), int(reset)))
    return json.loads(_take(buf, n))


def planes_distance(planes_ptr, n_samples, words_per_row, filt_ambig, constant, i_lo, i_hi, ctx=None):
    """VariantDist of the pairs (i in [i_lo, i_hi), j > i) from gathered bit planes (skx_planes_distance)"""
    ctx = ctx or default_context()
    n = sum(n_samples - 1 - i for i in range(i_lo, i_hi))
    out = np.zeros(n, DIST_DT)
    if n == 0:
        return out
    _check(_lib.skx_planes_distance(ctx.h, planes_ptr, n_samples, words_per_row, int(filt_ambig), float(constant), i_lo, i_hi, _np_ptr(out)))
    return out


def read_records(file1, file2=None, proportion_reads=0.0, streaming=False):
    """One sample's files as the record stream the device takes (host only): (seq bytes, qual bytes or None)."""
    lib = load_library()
    ps, pq, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    _check(lib.skx_read_records(file1.encode(), file2.encode() if file2 else None, float(proportion_reads), int(bool(streaming)), C.byref(ps), C.byref(pq), C.byref(n)))
    seq = C.string_at(ps, n.value)
    q = C.string_at(pq, n.value) if pq.value else None
    lib.skx_free(ps)
    if pq.value:
        lib.skx_free(pq)
    return seq, q


def sample_name(path):
    lib = load_library()
    p = lib.skh_sample_name(path.encode())
    s = C.string_at(p).decode()
    lib.skx_free(p)
    return s


class LoInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("words_per_node", C.c_int32), ("n_samples", C.c_uint64), ("colour_words", C.c_uint64),
                ("n_nodes", C.c_uint64), ("n_edges", C.c_uint64), ("n_entries", C.c_uint64), ("n_colours", C.c_uint64), ("n_kmers", C.c_uint64)]


def _to_ints(words, wpn):
    """[n * wpn] little-endian 64-bit words -> list of Python ints"""
    if wpn == 1:
        return [int(x) for x in words]
    return [int(words[2 * i]) | (int(words[2 * i + 1]) << 64) for i in range(len(words) // 2)]


class LoGraph:
    """`ska lo`'s device graph (skx_array_lo_graph): CSR arrays as numpy (wpn 64-bit words per node), colours on demand"""

    def __init__(self, h):
        self.h = h
        inf = LoInfo()
        _check(_lib.skx_lo_graph_info(h, C.byref(inf)))
        self.info = {n: getattr(inf, n) for n, _ in LoInfo._fields_}
        w, N, E, X = inf.words_per_node, inf.n_nodes, inf.n_edges, inf.n_entries
        self.wpn = w
        self.nodes = np.zeros(N * w, np.uint64)
        self.offsets = np.zeros(N + 1, np.uint64)
        self.neighbours = np.zeros(E * w, np.uint64)
        self.entries = np.zeros(X * w, np.uint64)
        self.exits = np.zeros(X * w, np.uint64)
        _check(_lib.skx_lo_graph_export(h, self.nodes.ctypes.data, self.offsets.ctypes.data, self.neighbours.ctypes.data,
                                        self.entries.ctypes.data, self.exits.ctypes.data))

    def adjacency(self):
        """{node: [neighbours]} as Python ints"""
        nodes, nb = _to_ints(self.nodes, self.wpn), _to_ints(self.neighbours, self.wpn)
        off = [int(x) for x in self.offsets]
        return {n: nb[off[i]:off[i + 1]] for i, n in enumerate(nodes)}

    def gather(self, kmers):
        """full k-mers (Python ints) -> (colours as Python int bitsets, found flags)"""
        n, w = len(kmers), self.wpn
        q = np.zeros(max(1, n * w), np.uint64)
        for i, x in enumerate(kmers):
            for j in range(w):
                q[i * w + j] = (x >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
        W = self.info["colour_words"]
        out = np.zeros(max(1, n * W), np.uint64)
        found = np.zeros(max(1, n), np.uint8)
        _check(_lib.skx_lo_gather(self.h, q.ctypes.data, n, out.ctypes.data, found.ctypes.data))
        cols = [sum(int(out[i * W + t]) << (64 * t) for t in range(W)) for i in range(n)]
        return cols, [bool(found[i]) for i in range(n)]

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.skx_lo_graph_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


class Context:
    def __init__(self, device=0):
        lib = load_library()
        h = C.c_void_p()
        _check(lib.skx_ctx_create(device, C.byref(h)))
        self.h = h

    def sync(self):
        _check(_lib.skx_ctx_sync(self.h))

    @property
    def stream(self):
        return _lib.skx_ctx_stream(self.h)

    def timings(self, reset=False):
        t = Timings()
        _lib.skx_ctx_timings(self.h, C.byref(t), int(reset))
        return {n: getattr(t, n) for n, _ in Timings._fields_}

    def merge_path(self):
        """'append64' / 'append128' / 'sorted: <why>': the kernels the last merge on this context went through"""
        return _lib.skx_ctx_merge_path(self.h).decode()

    def filter_cut(self):
        """(ranks, row blocks): what the statistics pass of the last filter on this context left unread under its rank bound -- (0, 0): the full pass"""
        r, b = C.c_uint64(0), C.c_uint64(0)
        _check(_lib.skx_ctx_filter_cut(self.h, C.byref(r), C.byref(b)))
        return int(r.value), int(b.value)

    def lo_graph(self, array):
        """skx_array_lo_graph: `ska lo`'s coloured de Bruijn graph of `array` (a device Array on this context)"""
        h = C.c_void_p()
        _check(_lib.skx_array_lo_graph(array.h, C.byref(h)))
        return LoGraph(h)

    def dist_nj(self, dist, n_samples):
        """skx_dist_nj: neighbour joining on the `distance` field of a pair table (DIST_DT, n(n-1)/2 pairs) -> n - 1 join records (NJ_DT)"""
        dist = np.ascontiguousarray(dist, DIST_DT)
        if n_samples >= 2 and dist.size != n_samples * (n_samples - 1) // 2:
            raise ValueError("the table does not hold n(n-1)/2 pairs")
        joins = np.zeros(max(n_samples - 1, 1), NJ_DT)
        _check(_lib.skx_dist_nj(self.h, _np_ptr(dist), n_samples, _np_ptr(joins)))
        return joins[: n_samples - 1]

    def matrix_nj(self, matrix):
        """skx_matrix_nj: the same on a full symmetric n x n float64 matrix with a zero diagonal"""
        m = np.ascontiguousarray(matrix, np.float64)
        if m.ndim != 2 or m.shape[0] != m.shape[1]:
            raise ValueError("a square matrix is required")
        n = m.shape[0]
        joins = np.zeros(max(n - 1, 1), NJ_DT)
        _check(_lib.skx_matrix_nj(self.h, _np_ptr(m), n, _np_ptr(joins)))
        return joins[: n - 1]

    def distance_skf_tsv(self, skf_file, min_freq=0.0, filt_ambig=True, tree=None, clusters=None, cluster_snps=10.0, cluster_mismatches=1.0):
        """`ska distance <skf> [--tree FILE] [--clusters PREFIX ...]` (skh_distance_skf_tsv_extras) -> the table's text"""
        x = DistExtras(tree.encode() if tree else None, clusters.encode() if clusters else None, cluster_snps, cluster_mismatches)
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.skh_distance_skf_tsv_extras(self.h, skf_file.encode(), min_freq, int(filt_ambig), C.byref(x) if tree or clusters else None,
                                                C.byref(p), C.byref(n)))
        return _take(p, n)

    def distance_query_tsv(self, skf_file, names=(), query_skf=None, min_freq=0.0, filt_ambig=True):
        """`ska distance <skf> --query NAMES [--query-skf FILE]` (skh_distance_query_tsv) -> the header and the table's lines that name a query"""
        names = list(names)
        arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.skh_distance_query_tsv(self.h, skf_file.encode(), query_skf.encode() if query_skf else None, arr, len(names), float(min_freq),
                                           int(filt_ambig), C.byref(p), C.byref(n)))
        return _take(p, n)

    def distance_select_tsv(self, skf_file, min_freq=0.0, filt_ambig=True, max_snps=None, max_mismatches=None, closest=0, band_rows=0):
        """`ska distance <skf> --max-snps N --max-mismatches P --closest K` (skh_distance_select_tsv) -> the header and the table's lines the criteria keep"""
        spec = SelectSpec.of(max_snps, max_mismatches, closest, band_rows)
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.skh_distance_select_tsv(self.h, skf_file.encode(), float(min_freq), int(filt_ambig), C.byref(spec), C.byref(p), C.byref(n)))
        return _take(p, n)

    def distance_mst_tsv(self, skf_file, min_freq=0.0, filt_ambig=True, max_snps=None, max_mismatches=None, band_rows=0):
        """`ska distance <skf> --mst [--max-snps N] [--max-mismatches P]` (skh_distance_mst_tsv) -> the header and the lines of the table's minimum spanning forest"""
        spec = MstSpec.of(max_snps, max_mismatches, band_rows)
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.skh_distance_mst_tsv(self.h, skf_file.encode(), float(min_freq), int(filt_ambig), C.byref(spec), C.byref(p), C.byref(n)))
        return _take(p, n)

    def distance_sites(self, skf_file, prefix, min_freq=0.0, max_snps=None, max_mismatches=None, closest=0, mst=False, max_records=0):
        """`ska distance <skf> (--max-snps N | --max-mismatches P | --closest K | --mst) --sites PREFIX` (skh_distance_sites) -> the header and
        the selected lines; PREFIX.sites.tsv lists the rows behind each line's Distance.  Above max_records (0: no limit) the call raises and
        the error carries the table as its `table` attribute"""
        sel, forest = SelectSpec.of(max_snps, max_mismatches, closest), MstSpec.of(max_snps, max_mismatches)
        p, n = C.c_void_p(), C.c_uint64()
        rc = _lib.skh_distance_sites(self.h, os.fsencode(skf_file), float(min_freq), None if mst else C.byref(sel), C.byref(forest) if mst else None,
                                     os.fsencode(prefix), int(max_records), C.byref(p), C.byref(n))
        table = _take(p, n) if p.value else None
        if rc != OK:
            err = EngineError(rc, _lib.skx_last_error().decode())
            err.table = table
            raise err
        return table

    def distance_banded_files(self, skf_file, min_freq=0.0, filt_ambig=True, tree=None, clusters=None, cluster_snps=10.0, cluster_mismatches=1.0):
        """`ska distance <skf> --no-table [--tree FILE] [--clusters PREFIX ...]` (skh_distance_banded_files): the files, no table"""
        x = DistExtras(tree.encode() if tree else None, clusters.encode() if clusters else None, cluster_snps, cluster_mismatches)
        _check(_lib.skh_distance_banded_files(self.h, skf_file.encode(), float(min_freq), int(filt_ambig), C.byref(x)))

    def align_groups(self, inputs, groups_file, out_prefix, min_group_size=2, threads=1, min_freq=0.9, filter_ambig_as_missing=False,
                     filter_type=FILTER_NO_CONST, mask_ambig=False, ignore_const_gaps=False):
        """`ska align <inputs> --groups FILE -o PREFIX` (skh_align_groups): PREFIX.<label>.aln per group and PREFIX.groups.tsv from one load"""
        inputs = [inputs] if isinstance(inputs, str) else list(inputs)
        arr = (C.c_char_p * len(inputs))(*[x.encode() for x in inputs])
        _check(_lib.skh_align_groups(self.h, arr, len(inputs), int(threads), int(filter_type), int(mask_ambig), int(ignore_const_gaps), float(min_freq),
                                     int(filter_ambig_as_missing), groups_file.encode(), int(min_group_size), out_prefix.encode()))

    def markers(self, skf_file, groups_file, out_prefix, min_in=1.0, max_out=0.0, min_group_size=1, kinds=MARKER_PRESENCE | MARKER_ALLELE, fasta=False):
        """`ska markers <skf> --groups FILE -o PREFIX` (skh_markers): PREFIX.markers.tsv, PREFIX.markers.summary.tsv and, with fasta,
        PREFIX.<label>.markers.fa per group, from one load"""
        _check(_lib.skh_markers(self.h, os.fsencode(skf_file), os.fsencode(groups_file), os.fsencode(out_prefix), float(min_in), float(max_out),
                                int(min_group_size), int(kinds), int(fasta)))

    def curve(self, skf_file, out_prefix, permutations=20, seed=1, min_freq=0.9, order_file=None, all_permutations=False):
        """`ska curve <skf> -o PREFIX` (skh_curve): PREFIX.curve.tsv and, with all_permutations or an order file, PREFIX.curve.permutations.tsv"""
        _check(_lib.skh_curve(self.h, os.fsencode(skf_file), os.fsencode(out_prefix), int(permutations), int(seed), float(min_freq),
                              None if order_file is None else os.fsencode(order_file), int(all_permutations)))

    def qc(self, skf_file, out_prefix, min_freq=0.9, mad=5.0):
        """`ska qc <skf> -o PREFIX` (skh_qc): PREFIX.qc.tsv, PREFIX.qc.summary.tsv and PREFIX.qc.flagged.txt"""
        _check(_lib.skh_qc(self.h, os.fsencode(skf_file), os.fsencode(out_prefix), float(min_freq), float(mad)))

    def mask(self, reference, skf_file, out_file, regions=None, dense=False, window=1000, min_snps=5, bed=None, summary=None):
        """`ska mask <reference> <skf> -o OUT.skf` (skh_mask): the intervals of a regions file or of `ska density` on the loaded array (dense), and of
        a BED file, taken out of the array, which is saved as out_file; with summary, <summary>.mask.summary.tsv"""
        enc = lambda x: None if x is None else os.fsencode(x)
        _check(_lib.skh_mask(self.h, os.fsencode(reference), os.fsencode(skf_file), os.fsencode(out_file), enc(regions), int(dense), int(window), int(min_snps),
                             enc(bed), enc(summary)))

    def density(self, reference, skf_file, out_prefix, window=1000, min_snps=5, snps=False, masked_aln=None):
        """`ska density <reference> <skf> -o PREFIX` (skh_density): PREFIX.density.regions.tsv, .summary.tsv, .bins.tsv and, with snps, .snps.tsv;
        masked_aln: also `ska map --repeat-mask`'s alignment with the regions overwritten by 'N' into that file"""
        _check(_lib.skh_density(self.h, os.fsencode(reference), os.fsencode(skf_file), os.fsencode(out_prefix), int(window), int(min_snps), int(snps),
                                os.fsencode(masked_aln) if masked_aln is not None else None))

    def screen(self, skf_file, panel, out_prefix, min_cover=0.9, min_identity=0.0, matrix=False):
        """`ska screen <skf> <panel> -o PREFIX` (skh_screen): PREFIX.screen.tsv, PREFIX.screen.summary.tsv and, with matrix, PREFIX.screen.matrix.tsv"""
        _check(_lib.skh_screen(self.h, os.fsencode(skf_file), os.fsencode(panel), os.fsencode(out_prefix), float(min_cover), float(min_identity), int(matrix)))

    def align_samples(self, inputs, names, fd, threads=1, min_freq=0.9, filter_ambig_as_missing=False, filter_type=FILTER_NO_CONST, mask_ambig=False,
                      ignore_const_gaps=False):
        """`ska align <inputs> --samples NAMES` (skh_align_samples_fd): the alignment of that subset streamed to a file descriptor"""
        inputs = [inputs] if isinstance(inputs, str) else list(inputs)
        names = list(names)
        arr = (C.c_char_p * len(inputs))(*[x.encode() for x in inputs])
        nm = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
        _check(_lib.skh_align_samples_fd(self.h, arr, len(inputs), int(threads), int(filter_type), int(mask_ambig), int(ignore_const_gaps), float(min_freq),
                                         int(filter_ambig_as_missing), nm, len(names), int(fd)))

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.skx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("LOCAL_RANK", "0")) if os.environ.get("SKX_USE_LOCAL_RANK") else 0)
    return _default_ctx



def _join_table(joins):
    """joins as TREE_JOIN_DT records or as pairs -> [n - 1, 2] uint32"""
    j = np.asarray(joins)
    if j.dtype.names:
        j = np.stack([j["a"], j["b"]], axis=1) if len(j) else np.zeros((0, 2), np.uint32)
    return np.ascontiguousarray(j, np.uint32).reshape(-1, 2)


def newick_joins(text, names):
    """skh_newick_joins: Newick text over the samples `names` -> (joins as TREE_JOIN_DT, root_three) (host only)"""
    load_library()
    n = len(names)
    arr = (C.c_char_p * max(n, 1))(*[x.encode() for x in names])
    joins, three = np.zeros(max(n - 1, 1), TREE_JOIN_DT), C.c_int()
    _check(_lib.skh_newick_joins(text.encode(), arr, n, _np_ptr(joins), C.byref(three)))
    return joins[:n - 1], bool(three.value)


def _parsimony_text(fn, names, joins, root_three, branch_changes):
    load_library()
    n = len(names)
    arr = (C.c_char_p * n)(*[x.encode() for x in names])
    j = _join_table(joins)
    b = np.ascontiguousarray(branch_changes, np.uint64)
    if len(j) != n - 1 or len(b) != 2 * n - 2:
        raise ValueError("n - 1 joins and 2 n - 2 branches are required")
    p, ln = C.c_void_p(), C.c_uint64()
    _check(fn(arr, _np_ptr(j), n, int(root_three), _np_ptr(b), C.byref(p), C.byref(ln)))
    return _take(p, ln).decode()


def parsimony_newick(names, joins, root_three, branch_changes):
    """skh_parsimony_newick: the tree of skh_newick_joins again, the changes as branch lengths (host only)"""
    load_library()
    return _parsimony_text(_lib.skh_parsimony_newick, names, joins, root_three, branch_changes)


def parsimony_branches(names, joins, root_three, branch_changes):
    """skh_parsimony_branches: the same tree as PREFIX.branches.tsv (host only)"""
    load_library()
    return _parsimony_text(_lib.skh_parsimony_branches, names, joins, root_three, branch_changes)


def nj_newick(names, joins):
    """skh_nj_newick: the joins of Context.dist_nj / matrix_nj as one line of midpoint-rooted Newick (host only)"""
    load_library()
    n = len(names)
    j = np.ascontiguousarray(joins, NJ_DT)
    if j.size != n - 1:
        raise ValueError("n - 1 join records are required")
    arr = (C.c_char_p * n)(*[x.encode() for x in names])
    p, ln = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_nj_newick(arr, _np_ptr(j), n, C.byref(p), C.byref(ln)))
    return _take(p, ln).decode()


def distance_clusters(names, dist, max_snps=10.0, max_mismatches=1.0):
    """skh_distance_clusters: single-linkage clusters of a pair table -> (clusters.csv text, graph.dot text) (host only)"""
    load_library()
    n = len(names)
    d = np.ascontiguousarray(dist, DIST_DT)
    if d.size != n * (n - 1) // 2:
        raise ValueError("the table does not hold n(n-1)/2 pairs")
    arr = (C.c_char_p * n)(*[x.encode() for x in names])
    pc, nc, pd, nd = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    _check(_lib.skh_distance_clusters(arr, _np_ptr(d) if d.size else None, n, max_snps, max_mismatches, C.byref(pc), C.byref(nc), C.byref(pd), C.byref(nd)))
    return _take(pc, nc).decode(), _take(pd, nd).decode()


def clusters_csv(names, labels):
    """skh_clusters_csv: clusters.csv text of labels[i] = the lowest sample of i's cluster (host only)"""
    load_library()
    n = len(names)
    lab = np.ascontiguousarray(labels, np.uint32)
    if lab.size != n:
        raise ValueError("one label per name is required")
    arr = (C.c_char_p * n)(*[x.encode() for x in names])
    p, ln = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_clusters_csv(arr, _np_ptr(lab), n, C.byref(p), C.byref(ln)))
    return _take(p, ln).decode()


def mst_levels_csv(names, pairs, levels):
    """skh_mst_levels_csv: levels.csv text -- every sample's cluster at each level (the forest's lines whose printed distance is <= the level) and its
    address; pairs as Array.distance_mst returns them (host only)"""
    load_library()
    n = len(names)
    pr = np.ascontiguousarray(pairs, PAIR_DT)
    lv = np.ascontiguousarray(levels, np.float64)
    arr = (C.c_char_p * max(n, 1))(*[x.encode() for x in names])
    p, ln = C.c_void_p(), C.c_uint64()
    _check(_lib.skh_mst_levels_csv(arr, _np_ptr(pr) if pr.size else None, pr.size, n, _np_ptr(lv) if lv.size else None, lv.size, C.byref(p), C.byref(ln)))
    return _take(p, ln).decode()


def read_groups(path):
    """skh_read_groups: the groups file of `ska align --groups` -> [(label, [sample names])] in the order the labels first appear (host only)"""
    load_library()
    p, ln, n = C.c_void_p(), C.c_uint64(), C.c_uint64()
    _check(_lib.skh_read_groups(os.fsencode(path), C.byref(p), C.byref(ln), C.byref(n)))
    parts = _take(p, ln).split(b"\0")[:-1]
    groups = []
    for name, label in zip(parts[0::2], parts[1::2]):
        label = label.decode()
        if not groups or groups[-1][0] != label:
            groups.append((label, []))
        groups[-1][1].append(name.decode())
    return groups


def cluster_cutoffs(max_snps, max_mismatches, filt_ambig=True):
    """skh_cluster_cutoffs: the printed-value rules of skh_distance_clusters as (largest key, largest float64 proportion) that pass (host only)"""
    load_library()
    kmax, pmax = C.c_uint64(), C.c_double()
    _check(_lib.skh_cluster_cutoffs(float(max_snps), float(max_mismatches), int(filt_ambig), C.byref(kmax), C.byref(pmax)))
    return kmax.value, pmax.value


def record_stream(records):
    """records: iterable of bytes -> the device record stream (each record + b'\\n')."""
    return b"".join(bytes(r) + b"\n" for r in records)


COMM_ID_BYTES = 128


def comm_unique_id():
    """ncclGetUniqueId through the ABI: rank 0 makes it, the host carries the 128 bytes to the other ranks"""
    load_library()
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(_lib.skx_comm_unique_id(buf))
    return bytes(buf)


def shard_range(n_items, rank, world):
    """Contiguous shard [lo, hi) of rank (skx_shard_range; input order kept, cf. merge_ska_dict.rs:243-253,277-291)"""
    load_library()
    lo, hi = C.c_uint64(), C.c_uint64()
    _check(_lib.skx_shard_range(n_items, rank, world, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def pair_bands(n_samples, world, align=8):
    """Bands [i_lo, i_hi) of first samples of the pair matrix, one per rank (skx_pair_bands)"""
    load_library()
    out = np.zeros(2 * world, np.int32)
    _check(_lib.skx_pair_bands(n_samples, world, align, _np_ptr(out)))
    return [(int(out[2 * r]), int(out[2 * r + 1])) for r in range(world)]


class Comm:
    """The exchanges of a multi-GPU job behind the C ABI (include/skx.h "Collectives"): RCCL (Comm.rccl) or, for ranks that share
    one device, host-staged through a directory (Comm.local).  Every method is collective."""

    def __init__(self, handle, ctx):
        self.h, self.ctx = handle, ctx

    @classmethod
    def rccl(cls, rank, world, unique_id, ctx=None):
        ctx = ctx or default_context()
        h = C.c_void_p()
        idb = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(_lib.skx_comm_create(ctx.h, rank, world, idb, C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def local(cls, rank, world, directory, ctx=None):
        """ctx may be None: host buffers only (no GPU needed)"""
        load_library()
        h = C.c_void_p()
        _check(_lib.skx_comm_create_local(ctx.h if ctx is not None else None, rank, world, directory.encode(), C.byref(h)))
        return cls(h, ctx)

    rank = property(lambda self: _lib.skx_comm_rank(self.h))
    world = property(lambda self: _lib.skx_comm_world(self.h))
    bytes_received = property(lambda self: int(_lib.skx_comm_bytes_received(self.h)))

    def transport(self):
        """(ranks of the RCCL communicator -- 0 for the host-staged transport --, the device RCCL bound it to, the context's device)"""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(_lib.skx_comm_transport(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def barrier(self):
        _check(_lib.skx_comm_barrier(self.h))

    def allgather_host(self, arr):
        """numpy array (same shape on every rank) -> [world, ...]"""
        a = np.ascontiguousarray(arr)
        out = np.empty((self.world,) + a.shape, a.dtype)
        _check(_lib.skx_comm_allgather(self.h, _np_ptr(a), _np_ptr(out), a.nbytes, 0))
        return out

    def allgather_device(self, send_ptr, recv_ptr, nbytes):
        _check(_lib.skx_comm_allgather(self.h, send_ptr, recv_ptr, nbytes, 1))

    def allreduce_u32_host(self, arr):
        a = np.ascontiguousarray(arr, np.uint32).copy()
        _check(_lib.skx_comm_allreduce_u32(self.h, _np_ptr(a), a.size, 0))
        return a

    def gather_root_host(self, arr, sizes):
        """byte blocks of different sizes (sizes known everywhere) -> rank 0: one uint8 array there, None elsewhere"""
        a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        sz = np.ascontiguousarray(sizes, np.uint64)
        out = np.empty(int(sz.sum()) if self.rank == 0 else 0, np.uint8)
        _check(_lib.skx_comm_gather_root(self.h, _np_ptr(a), _np_ptr(sz), _np_ptr(out)))
        return out if self.rank == 0 else None

    def allreduce_u32_device(self, ptr, n):
        _check(_lib.skx_comm_allreduce_u32(self.h, ptr, n, 1))

    def keyset_allgather(self, local):
        """exchange 1: the global row set from every rank's key table (skx_keyset_allgather)"""
        h = C.c_void_p()
        _check(_lib.skx_keyset_allgather(self.h, local.h, C.byref(h)))
        return KeySet(h, self.ctx)

    def reduce_stats(self, array, total_samples):
        """exchange 2: per-row filter statistics over all ranks (skx_array_reduce_stats)"""
        _check(_lib.skx_array_reduce_stats(self.h, array.h, total_samples))

    def distance_sharded(self, array, total_samples, filt_ambig=True, constant=0.0):
        """exchange 3 + the pair sweep by bands (skx_array_distance_sharded): the whole table on rank 0, None elsewhere"""
        n = total_samples * (total_samples - 1) // 2
        out = np.zeros(n + 1 if self.rank == 0 else 1, DIST_DT)
        _check(_lib.skx_array_distance_sharded(self.h, array.h, int(filt_ambig), float(constant), _np_ptr(out), out.size))
        return out[:n] if self.rank == 0 else None

    def _job(self, names, inputs, k, rc, q, threads, proportion_reads, output):
        n = len(names)
        keep = [(C.c_char_p * n)(*[x.encode() for x in names]), (C.c_char_p * n)(*[a.encode() for a, _ in inputs]),
                (C.c_char_p * n)(*[(b.encode() if b else None) for _, b in inputs]), output.encode() if output else None]
        j = Job()
        j.names, j.file1, j.file2, j.n_samples = keep[0], keep[1], keep[2], n
        j.k, j.rc, j.qual, j.threads, j.proportion_reads, j.output = k, int(rc), q or qual(), threads, proportion_reads, keep[3]
        return j, keep

    def build(self, names, inputs, output, k=31, rc=True, q=None, threads=1, proportion_reads=0.0, merge_parts=False):
        """one rank of `ska build` over several GPUs (skh_build_sharded); inputs = [(file1, file2 | None)] of the WHOLE job"""
        j, keep = self._job(names, inputs, k, rc, q, threads, proportion_reads, output)
        j.merge_parts = int(merge_parts)
        _check(_lib.skh_build_sharded(self.ctx.h, self.h, C.byref(j)))

    def align(self, names, inputs, output, k=31, rc=True, q=None, threads=1, proportion_reads=0.0, min_freq=0.9, filter_type=FILTER_NO_CONST,
              mask_ambig=False, ignore_const_gaps=False, filter_ambig_as_missing=False):
        j, keep = self._job(names, inputs, k, rc, q, threads, proportion_reads, output)
        j.min_freq, j.filter_type, j.mask_ambig, j.ignore_const_gaps, j.filter_ambig_as_missing = min_freq, filter_type, int(mask_ambig), int(ignore_const_gaps), int(filter_ambig_as_missing)
        _check(_lib.skh_align_sharded(self.ctx.h, self.h, C.byref(j)))

    def distance(self, names, inputs, output, k=31, rc=True, q=None, threads=1, proportion_reads=0.0, min_freq=0.0, filt_ambig=True,
                 tree=None, clusters=None, cluster_snps=10.0, cluster_mismatches=1.0):
        j, keep = self._job(names, inputs, k, rc, q, threads, proportion_reads, output)
        j.min_freq, j.filt_ambig = min_freq, int(filt_ambig)
        if tree or clusters:                             # rank 0, which holds the table, writes them
            x = DistExtras(tree.encode() if tree else None, clusters.encode() if clusters else None, cluster_snps, cluster_mismatches)
            j.extras = C.cast(C.pointer(x), C.c_void_p)
        _check(_lib.skh_distance_sharded(self.ctx.h, self.h, C.byref(j)))

    def free(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.skx_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        self.free()


class DictSet:
    """A batch of per-sample SkaDicts (ska_dict.rs:56-69), device resident."""

    def __init__(self, handle, ctx):
        self.h, self.ctx = handle, ctx

    @classmethod
    def build(cls, streams, k, rc=True, q=None, ctx=None, quals=None):
        """streams: list of record-stream bytes (host); quals: optional list of quality streams."""
        ctx = ctx or default_context()
        q = q or qual()
        n = len(streams)
        bufs = [np.frombuffer(s, dtype=np.uint8) for s in streams]
        qbufs = [np.frombuffer(s, dtype=np.uint8) if s is not None else None for s in (quals or [None] * n)]
        arr = (Stream * n)()
        for i in range(n):
            arr[i].seq = bufs[i].ctypes.data if len(bufs[i]) else None
            arr[i].qual = qbufs[i].ctypes.data if qbufs[i] is not None else None
            arr[i].len = len(bufs[i])
        h = C.c_void_p()
        _check(_lib.skx_dictset_build(ctx.h, arr, n, 0, k, int(rc), C.byref(q), C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def build_device(cls, ptrs, lens, k, rc=True, q=None, ctx=None):
        """ptrs: device pointers (ints) of 16-B aligned record streams already in HBM."""
        ctx = ctx or default_context()
        q = q or qual()
        n = len(ptrs)
        arr = (Stream * n)()
        for i in range(n):
            arr[i].seq, arr[i].qual, arr[i].len = ptrs[i], None, lens[i]
        h = C.c_void_p()
        _check(_lib.skx_dictset_build(ctx.h, arr, n, 1, k, int(rc), C.byref(q), C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def from_files(cls, inputs, k, rc=True, q=None, threads=1, proportion_reads=0.0, ctx=None):
        ctx = ctx or default_context()
        q = q or qual()
        n = len(inputs)
        f1 = (C.c_char_p * n)(*[x[0].encode() for x in inputs])
        f2 = (C.c_char_p * n)(*[(x[1].encode() if x[1] else None) for x in inputs])
        h = C.c_void_p()
        _check(_lib.skx_dictset_build_files(ctx.h, f1, f2, n, k, int(rc), C.byref(q), threads, proportion_reads, C.byref(h)))
        return cls(h, ctx)

    @property
    def nsamples(self):
        return _lib.skx_dictset_nsamples(self.h)

    @property
    def key_bits(self):
        return _lib.skx_dictset_key_bits(self.h)

    def size(self, sample):
        n = C.c_uint64()
        _check(_lib.skx_dictset_size(self.h, sample, C.byref(n)))
        return n.value

    def export(self, sample):
        n = self.size(sample)
        keys = np.zeros(n, KEY_DT)
        bases = np.zeros(n, np.uint8)
        _check(_lib.skx_dictset_export(self.h, sample, _np_ptr(keys), _np_ptr(bases), n))
        return keys, bases

    def union_keys(self, notes=False):
        """notes: keep the pass's notes for the eager assemble that follows (directly or after KeySet all-gather): skx_keyset_union_notes"""
        h = C.c_void_p()
        _check((_lib.skx_keyset_union_notes if notes else _lib.skx_keyset_union)(self.ctx.h, self.h, C.byref(h)))
        return KeySet(h, self.ctx)

    def merge(self, names):
        n = len(names)
        nm = (C.c_char_p * n)(*[x.encode() for x in names])
        h = C.c_void_p()
        _check(_lib.skx_merge(self.ctx.h, self.h, nm, C.byref(h)))
        return Array(h, self.ctx)

    def assemble(self, rows, names):
        n = len(names)
        nm = (C.c_char_p * n)(*[x.encode() for x in names])
        h = C.c_void_p()
        _check(_lib.skx_array_assemble(self.ctx.h, self.h, rows.h, nm, C.byref(h)))
        return Array(h, self.ctx)

    def assemble_lazy(self, rows, names):
        """rows + these dictionaries as an array without a matrix; the dictset and the row set pass into the array (both handles end here)"""
        n = len(names)
        nm = (C.c_char_p * n)(*[x.encode() for x in names])
        h = C.c_void_p()
        dh, rh = self.h, rows.h
        self.h = None; rows.h = None
        _check(_lib.skx_array_assemble_lazy(self.ctx.h, dh, rh, nm, C.byref(h)))
        return Array(h, self.ctx)

    def free(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.skx_dictset_free(self.h)
            self.h = None

    def __del__(self):
        self.free()


class KeySet:
    def __init__(self, handle, ctx):
        self.h, self.ctx = handle, ctx

    def __len__(self):
        n = C.c_uint64()
        _check(_lib.skx_keyset_size(self.h, C.byref(n)))
        return n.value

    def device(self):
        p, n, w = C.c_void_p(), C.c_uint64(), C.c_int()
        _check(_lib.skx_keyset_device(self.h, C.byref(p), C.byref(n), C.byref(w)))
        return p.value, n.value, w.value

    @classmethod
    def from_device(cls, ptr, n_keys, k, rc=True, ctx=None):
        ctx = ctx or default_context()
        h = C.c_void_p()
        _check(_lib.skx_keyset_from_device(ctx.h, ptr, n_keys, k, int(rc), C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def from_fasta(cls, path, k, rc=True, ctx=None):
        """RefSka::new + kmer_iter (ska_ref.rs:189-262,541): the split k-mers of a FASTA file (what `ska weed` removes)."""
        ctx = ctx or default_context()
        h = C.c_void_p()
        _check(_lib.skx_keyset_from_fasta(ctx.h, path.encode(), k, int(rc), C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def merge(cls, sets, ctx=None):
        ctx = ctx or sets[0].ctx
        hs = (C.c_void_p * len(sets))(*[s.h for s in sets])
        h = C.c_void_p()
        _check(_lib.skx_keyset_merge(ctx.h, hs, len(sets), C.byref(h)))
        return cls(h, ctx)

    def free(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.skx_keyset_free(self.h)
            self.h = None

    def __del__(self):
        self.free()


class Array:
    """MergeSkaArray (merge_ska_array.rs:109-126) on the device."""

    def __init__(self, handle, ctx):
        self.h, self.ctx = handle, ctx

    @classmethod
    def build(cls, inputs, k=31, rc=True, q=None, threads=1, proportion_reads=0.0, ctx=None):
        """inputs: list of (name, file1, file2|None): build_and_merge + MergeSkaArray::new."""
        ctx = ctx or default_context()
        q = q or qual()
        n = len(inputs)
        names = (C.c_char_p * n)(*[x[0].encode() for x in inputs])
        f1 = (C.c_char_p * n)(*[x[1].encode() for x in inputs])
        f2 = (C.c_char_p * n)(*[(x[2].encode() if x[2] else None) for x in inputs])
        h = C.c_void_p()
        _check(_lib.skx_build_and_merge(ctx.h, names, f1, f2, n, k, int(rc), C.byref(q), threads, proportion_reads, C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def load(cls, path, want_bits=0, ctx=None):
        ctx = ctx or default_context()
        h = C.c_void_p()
        if want_bits:
            _check(_lib.skx_array_load(ctx.h, path.encode(), want_bits, C.byref(h)))
        else:
            p = (C.c_char_p * 1)(path.encode())
            _check(_lib.skh_load_array(ctx.h, p, 1, 1, C.byref(h)))
        return cls(h, ctx)

    # ---- .skf life-cycle: ska merge / delete / weed (generic_modes.rs:90-106,192-267) ----
    @classmethod
    def load_filtered(cls, path, min_freq=0.9, filter_ambig_as_missing=False, filter_type=FILTER_NO_CONST, mask_ambig=False, ignore_const_gaps=False,
                      two_stage=False, ctx=None):
        """skx_array_load_filtered: load + apply_filters (or distance's two filters) in one pass -> (array, removed, constant)"""
        ctx = ctx or default_context()
        fs = FilterSpec(min_freq, int(filter_ambig_as_missing), filter_type, int(mask_ambig), int(ignore_const_gaps), int(two_stage))
        h, rem, cst = C.c_void_p(), C.c_int64(), C.c_int64()
        _check(_lib.skx_array_load_filtered(ctx.h, path.encode(), C.byref(fs), C.byref(h), C.byref(rem), C.byref(cst)))
        return cls(h, ctx), rem.value, cst.value

    @classmethod
    def merge(cls, arrays, ctx=None):
        ctx = ctx or arrays[0].ctx
        hs = (C.c_void_p * len(arrays))(*[a.h for a in arrays])
        h = C.c_void_p()
        _check(_lib.skx_array_merge(ctx.h, hs, len(arrays), C.byref(h)))
        return cls(h, ctx)

    def delete_samples(self, names):
        nm = (C.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
        _check(_lib.skx_array_delete_samples(self.h, nm, len(names)))

    def subset_filtered(self, samples, min_freq=0.9, filter_ambig_as_missing=False, filter_type=FILTER_NO_CONST, mask_ambig=False, ignore_const_gaps=False,
                        two_stage=False, counts_only=False):
        """skx_array_subset_filtered: delete_samples(everybody else) + apply_filters as a new array, this one left as it is
        -> (Array | None with counts_only, {"rows_present", "removed", "silent", "sites"}); samples = distinct column indices in any order"""
        idx = np.ascontiguousarray(samples, np.int32)
        fs = FilterSpec(min_freq, int(filter_ambig_as_missing), filter_type, int(mask_ambig), int(ignore_const_gaps), int(two_stage))
        h, info = C.c_void_p(), SubsetInfo()
        _check(_lib.skx_array_subset_filtered(self.h, _np_ptr(idx), len(idx), C.byref(fs), None if counts_only else C.byref(h), C.byref(info)))
        return (None if counts_only else Array(h, self.ctx)), {n: getattr(info, n) for n, _ in SubsetInfo._fields_}

    def group_markers(self, segment_of, n_groups, reported=None, min_in=1.0, max_out=0.0, kinds=MARKER_PRESENCE | MARKER_ALLELE):
        """skx_array_group_markers: the presence and allele markers of every reported group of a partition, this array left as it is.
        segment_of[s] = the group of sample s (n_groups: listed by no group); reported[g] (default: every group)
        -> (records as MARKER_DT sorted by (group, row), their split k-mers as KEY_DT, per-group counts as MARKER_INFO_DT)"""
        seg = np.ascontiguousarray(segment_of, np.int32)
        if seg.size != self.nsamples:
            raise ValueError("one segment per sample is required")
        rep = np.ones(max(n_groups, 1), np.uint8) if reported is None else np.ascontiguousarray(reported, np.uint8)
        if rep.size < n_groups:
            raise ValueError("one flag per group is required")
        info = np.zeros(max(n_groups, 1), MARKER_INFO_DT)
        pr, pk, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(_lib.skx_array_group_markers(self.h, _np_ptr(seg), int(n_groups), _np_ptr(rep), float(min_in), float(max_out), int(kinds),
                                            C.byref(pr), C.byref(pk), C.byref(n), _np_ptr(info)))
        rec = np.frombuffer(C.string_at(pr, n.value * MARKER_DT.itemsize), MARKER_DT).copy() if n.value else np.zeros(0, MARKER_DT)
        keys = np.frombuffer(C.string_at(pk, n.value * KEY_DT.itemsize), KEY_DT).copy() if n.value else np.zeros(0, KEY_DT)
        _lib.skx_free(pr)
        _lib.skx_free(pk)
        return rec, keys, info[:n_groups]

    def curve(self, orders, min_freq=0.9):
        """skx_array_curve: pan, core, variant and core_variant rows after each sample of every order has been added, this array left as it is.
        orders: [P, S] (or [S]) sample indices, every row a permutation -> uint64 [P, S, 4]"""
        o = np.ascontiguousarray(orders, np.int32)
        o = o.reshape(1, -1) if o.ndim == 1 else o
        if o.ndim != 2 or o.shape[1] != self.nsamples:
            raise ValueError("every order names each of the array's samples")
        counts = np.zeros((o.shape[0], o.shape[1], 4), np.uint64)
        _check(_lib.skx_array_curve(self.h, _np_ptr(o), o.shape[0], float(min_freq), _np_ptr(counts)))
        return counts

    def sample_qc(self, min_freq=0.9):
        """skx_array_sample_qc: six counts per sample that depend on their rows' statistics, this array left as it is
        -> (QC_SAMPLE_DT [S], the array's totals as a QC_INFO_DT record)"""
        rec = np.zeros(max(self.nsamples, 1), QC_SAMPLE_DT)
        info = np.zeros(1, QC_INFO_DT)
        _check(_lib.skx_array_sample_qc(self.h, float(min_freq), _np_ptr(rec), _np_ptr(info)))
        return rec[:self.nsamples], info[0]

    def screen(self, path):
        """skx_array_screen: per (record, sample) of the FASTA panel at `path` the hit windows' cells that are present, equal the record's base
        and are ambiguous, this array left as it is -> (ids, records as SCREEN_RECORD_DT [R], cells as SCREEN_CELL_DT [R, S])"""
        n, pr, pi, pc = C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(_lib.skx_array_screen(self.h, os.fsencode(path), C.byref(n), C.byref(pr), C.byref(pi), C.byref(pc)))
        R, S = n.value, self.nsamples
        rec = np.frombuffer(C.string_at(pr, R * SCREEN_RECORD_DT.itemsize), SCREEN_RECORD_DT).copy()
        cells = np.frombuffer(C.string_at(pc, R * S * SCREEN_CELL_DT.itemsize), SCREEN_CELL_DT).copy().reshape(R, S)
        ids, at = [], pi.value
        for _ in range(R):
            s = C.string_at(at)
            ids.append(s.decode())
            at += len(s) + 1
        for p in (pr, pi, pc):
            _lib.skx_free(p)
        return ids, rec, cells

    def snp_density(self, reference, window=1000, min_snps=5, snps=False):
        """skx_array_snp_density: per sample the dense-SNP regions along the FASTA reference at `reference`, this array left as it is -> a dict:
        info (DENSITY_INFO_DT record), samples (DENSITY_SAMPLE_DT [S]), regions (DENSITY_REGION_DT, 0-based), bins (DENSITY_BIN_DT), chrom_ids,
        chrom_lens (uint64 [C]) and, with snps, snps (uint64: sample << 34 | x << 2 | base, bit DENSITY_DENSE_BIT = dense) and snp_ref (uint8)"""
        r = DensityResult()
        _check(_lib.skx_array_snp_density(self.h, os.fsencode(reference), int(window), int(min_snps), DENSITY_WANT_SNPS if snps else 0, C.byref(r)))
        info = np.array([tuple(int(x) for x in r.info)], DENSITY_INFO_DT)[0]

        def take(p, n, dt):
            return np.frombuffer(C.string_at(p, n * np.dtype(dt).itemsize), dt).copy() if p and n else np.zeros(0, dt)
        nC = int(info["n_chrom"])
        out = {"info": info, "samples": take(r.samples, self.nsamples, DENSITY_SAMPLE_DT), "regions": take(r.regions, int(info["n_regions"]), DENSITY_REGION_DT),
               "bins": take(r.bins, int(info["n_bins"]), DENSITY_BIN_DT), "chrom_lens": take(r.chrom_lens, nC, np.uint64), "chrom_ids": [],
               "snps": take(r.snps, int(info["n_snps"]), np.uint64) if snps else None, "snp_ref": take(r.snp_ref, int(info["n_snps"]), np.uint8) if snps else None}
        at = r.chrom_ids
        for _ in range(nC):
            s = C.string_at(at)
            out["chrom_ids"].append(s.decode())
            at += len(s) + 1
        for p in (r.samples, r.regions, r.bins, r.chrom_ids, r.chrom_lens, r.snps, r.snp_ref):
            _lib.skx_free(p)
        return out

    def mask_regions(self, reference, intervals, want_samples=True):
        """skx_array_mask_regions, in place: intervals = [(sample | MASK_ALL_SAMPLES, chrom, start, end)], 0-based inclusive, or a MASK_INTERVAL_DT
        array -> (per-sample counts as MASK_SAMPLE_DT [S] or None, the call's counts as a MASK_INFO_DT record)"""
        iv = _mask_intervals(intervals)
        sm = np.zeros(max(self.nsamples, 1), MASK_SAMPLE_DT)
        info = np.zeros(1, MASK_INFO_DT)
        _check(_lib.skx_array_mask_regions(self.h, os.fsencode(reference), _np_ptr(iv) if len(iv) else None, len(iv), _np_ptr(sm) if want_samples else None, _np_ptr(info)))
        return (sm[:self.nsamples] if want_samples else None), info[0]

    def pair_sites(self, ij, min_freq=0.0, max_records=0, keys=True):
        """skx_array_pair_sites: the rows that make up the filter-ambiguous distance of each pair of ij ([n_pairs, 2], i < j), this array left as
        it is -> (records as PAIR_SITE_DT sorted by (pair, row), their split k-mers as KEY_DT or None, the sites per pair).  Above max_records
        (0: no limit) the call raises ENOMEM and the error carries the counts as its `counts` attribute"""
        ij = np.ascontiguousarray(ij, np.uint32).reshape(-1, 2)
        counts = np.zeros(max(len(ij), 1), np.uint64)
        pr, pk, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        rc = _lib.skx_array_pair_sites(self.h, float(min_freq), _np_ptr(ij), len(ij), int(max_records), C.byref(pr), C.byref(pk) if keys else None,
                                       _np_ptr(counts), C.byref(n))
        if rc != OK:
            err = EngineError(rc, _lib.skx_last_error().decode())
            err.counts, err.records = counts[:len(ij)], pr.value
            raise err
        rec = np.frombuffer(C.string_at(pr, n.value * PAIR_SITE_DT.itemsize), PAIR_SITE_DT).copy() if n.value else np.zeros(0, PAIR_SITE_DT)
        k = None
        if keys:
            k = np.frombuffer(C.string_at(pk, n.value * KEY_DT.itemsize), KEY_DT).copy() if n.value else np.zeros(0, KEY_DT)
            _lib.skx_free(pk)
        _lib.skx_free(pr)
        return rec, k, counts[:len(ij)]

    def map(self, reference, fmt="aln", ambig_mask=False, repeat_mask=False, threads=0):
        """generic_modes::map: RefSka::new + map + write_aln | write_vcf -> text (generic_modes.rs:56-84)."""
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.skx_array_map(self.h, reference.encode(), int(ambig_mask), int(repeat_mask), 1 if fmt == "vcf" else 0, threads, C.byref(p), C.byref(n)))
        return _take(p, n)

    def weed_keys(self, keyset, reverse=False):
        r = C.c_uint64()
        _check(_lib.skx_array_weed(self.h, keyset.h, int(reverse), C.byref(r)))
        return r.value

    def weed(self, weed_fasta=None, reverse=False, min_freq=0.9, filter_ambig_as_missing=False, filter_type=FILTER_NONE,
             ambig_mask=False, ignore_const_gaps=False):
        _check(_lib.skh_weed(self.h, weed_fasta.encode() if weed_fasta else None, int(reverse), min_freq, int(filter_ambig_as_missing),
                             filter_type, int(ambig_mask), int(ignore_const_gaps), None))

    @classmethod
    def from_host(cls, k, rc, names, keys, variants, counts=None, version=None, ctx=None):
        ctx = ctx or default_context()
        keys = np.ascontiguousarray(keys, dtype=KEY_DT)
        variants = np.ascontiguousarray(variants, dtype=np.uint8)
        n = len(names)
        nm = (C.c_char_p * n)(*[x.encode() for x in names])
        h = C.c_void_p()
        counts = np.ascontiguousarray(counts, dtype=np.uint64) if counts is not None else None
        _check(_lib.skx_array_from_host(ctx.h, k, int(rc), nm, n, _np_ptr(keys), _np_ptr(variants), _np_ptr(counts), len(keys),
                                        version.encode() if version else None, C.byref(h)))
        return cls(h, ctx)

    def save(self, path):
        _check(_lib.skx_array_save(self.h, path.encode()))

    def save_skf(self, prefix):
        _check(_lib.skh_save_skf(self.h, prefix.encode()))

    def _info(self):
        info = ArrayInfo()
        _check(_lib.skx_array_info(self.h, C.byref(info)))
        return info

    k = property(lambda s: s._info().k)
    rc = property(lambda s: bool(s._info().rc))
    k_bits = property(lambda s: s._info().k_bits)
    nrows = property(lambda s: s._info().n_rows)
    nkmers = property(lambda s: s._info().n_kmers)
    nsamples = property(lambda s: s._info().n_samples)
    version = property(lambda s: _lib.skx_array_version(s.h).decode())

    @property
    def names(self):
        return [_lib.skx_array_name(self.h, i).decode() for i in range(self.nsamples)]

    def export(self):
        info = self._info()
        keys = np.zeros(info.n_kmers, KEY_DT)
        var = np.zeros((info.n_rows, info.n_samples), np.uint8)
        counts = np.zeros(info.n_rows, np.uint64)
        _check(_lib.skx_array_export(self.h, _np_ptr(keys), _np_ptr(var), _np_ptr(counts)))
        return keys, var, counts

    def export_keys(self):
        """split k-mers (sorted) and their counts without moving the matrix"""
        info = self._info()
        keys = np.zeros(info.n_kmers, KEY_DT)
        counts = np.zeros(info.n_rows, np.uint64)
        _check(_lib.skx_array_export(self.h, _np_ptr(keys), None, _np_ptr(counts)))
        return keys, counts

    def sample_kmers(self):
        out = np.zeros(self.nsamples, np.int64)
        _check(_lib.skx_array_sample_kmers(self.h, _np_ptr(out)))
        return out

    def pieces_info(self):
        """(bytes of pieces, row blocks, ranks per block) of an array still held as the append pass left it; (0, 0, 0) otherwise"""
        b, j, c = C.c_uint64(), C.c_uint64(), C.c_uint32()
        _check(_lib.skx_array_pieces_info(self.h, C.byref(b), C.byref(j), C.byref(c)))
        return b.value, j.value, c.value

    def filter(self, min_count, filter_ambig_as_missing=False, filter_type=FILTER_NO_CONST, mask_ambig=False,
               ignore_const_gaps=False, update_kmers=True):
        r = C.c_int32()
        _check(_lib.skx_array_filter(self.h, min_count, int(filter_ambig_as_missing), filter_type, int(mask_ambig),
                                     int(ignore_const_gaps), int(update_kmers), C.byref(r)))
        return r.value

    def apply_filters(self, min_freq, filter_ambig_as_missing=False, filter_type=FILTER_NO_CONST, ambig_mask=False,
                      ignore_const_gaps=False):
        r = C.c_int32()
        _check(_lib.skh_apply_filters(self.h, min_freq, int(filter_ambig_as_missing), filter_type, int(ambig_mask),
                                      int(ignore_const_gaps), C.byref(r)))
        return r.value

    def fasta(self):
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.skx_array_fasta(self.h, C.byref(p), C.byref(n)))
        return _take(p, n)

    def write_fasta(self, fd):
        """write_fasta streamed to a file descriptor (merge_ska_array.rs:507-520)."""
        _check(_lib.skx_array_write_fasta(self.h, int(fd)))

    def device_matrix(self):
        p, pitch, rows = C.c_void_p(), C.c_uint64(), C.c_uint64()
        _check(_lib.skx_array_device_matrix(self.h, C.byref(p), C.byref(pitch), C.byref(rows)))
        return p.value, pitch.value, rows.value

    def device_stats(self):
        p = [C.c_void_p() for _ in range(4)]
        _check(_lib.skx_array_device_stats(self.h, *[C.byref(x) for x in p]))
        return [x.value for x in p]

    def set_total_samples(self, total):
        _check(_lib.skx_array_set_total_samples(self.h, total))

    def nk(self, full_info=False):
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.skh_nk(self.h, int(full_info), C.byref(p), C.byref(n)))
        return _take(p, n)

    def distance(self, constant=0.0, filt_ambig=True):
        s = self.nsamples
        out = np.zeros(s * (s - 1) // 2, DIST_DT)
        _check(_lib.skx_array_distance(self.h, constant, int(filt_ambig), _np_ptr(out)))
        return out

    def distance_filtered(self, min_freq=0.0, filt_ambig=True):
        """generic_modes::distance without filtering the array itself -> (pairs, constant sites, rows used)"""
        s = self.nsamples
        out = np.zeros(max(s * (s - 1) // 2, 1), DIST_DT)
        cst, rows = C.c_int64(), C.c_uint64()
        _check(_lib.skx_array_distance_filtered(self.h, float(min_freq), int(filt_ambig), _np_ptr(out), C.byref(cst), C.byref(rows)))
        return out[: s * (s - 1) // 2], cst.value, rows.value

    def distance_query(self, query, constant=0.0, filt_ambig=True):
        """skx_array_distance_query: out[q][j] = the pair (query[q], j) as `distance` gives it, the entry j == query[q] zeroed"""
        q = np.ascontiguousarray(query, np.int32)
        out = np.zeros((max(len(q), 1), self.nsamples), DIST_DT)
        _check(_lib.skx_array_distance_query(self.h, float(constant), int(filt_ambig), _np_ptr(q), len(q), _np_ptr(out)))
        return out[: len(q)]

    def distance_query_filtered(self, query, min_freq=0.0, filt_ambig=True):
        """skx_array_distance_query_filtered -> (out[q][j] as `distance_filtered` gives the pair, constant sites, rows used)"""
        q = np.ascontiguousarray(query, np.int32)
        out = np.zeros((max(len(q), 1), self.nsamples), DIST_DT)
        cst, rows = C.c_int64(), C.c_uint64()
        _check(_lib.skx_array_distance_query_filtered(self.h, float(min_freq), int(filt_ambig), _np_ptr(q), len(q), _np_ptr(out), C.byref(cst), C.byref(rows)))
        return out[: len(q)], cst.value, rows.value

    def distance_select(self, min_freq=0.0, filt_ambig=True, max_snps=None, max_mismatches=None, closest=0, band_rows=0):
        """skx_array_distance_select: the pairs of `distance_filtered`'s table the criteria keep, picked on the device band by band ->
        (pairs (PAIR_DT, ascending (i, j)), constant sites, rows used, info dict)"""
        spec = SelectSpec.of(max_snps, max_mismatches, closest, band_rows)
        p, n, cst, rows, info = C.c_void_p(), C.c_uint64(), C.c_int64(), C.c_uint64(), SelectInfo()
        _check(_lib.skx_array_distance_select(self.h, float(min_freq), int(filt_ambig), C.byref(spec), C.byref(p), C.byref(n), C.byref(cst), C.byref(rows), C.byref(info)))
        pairs = np.frombuffer(C.string_at(p, n.value * PAIR_DT.itemsize), PAIR_DT).copy() if n.value else np.zeros(0, PAIR_DT)
        if p:
            _lib.skx_free(p)
        return pairs, cst.value, rows.value, {f: getattr(info, f) for f, _ in SelectInfo._fields_}

    def distance_select_prefiltered(self, constant=0, filt_ambig=True, max_snps=None, max_mismatches=None, closest=0, band_rows=0):
        """skx_array_distance_select_prefiltered: the pairs of `distance`'s table (every row, `constant` added) the criteria keep -> (pairs, info dict)"""
        spec = SelectSpec.of(max_snps, max_mismatches, closest, band_rows)
        p, n, info = C.c_void_p(), C.c_uint64(), SelectInfo()
        _check(_lib.skx_array_distance_select_prefiltered(self.h, int(constant), int(filt_ambig), C.byref(spec), C.byref(p), C.byref(n), C.byref(info)))
        pairs = np.frombuffer(C.string_at(p, n.value * PAIR_DT.itemsize), PAIR_DT).copy() if n.value else np.zeros(0, PAIR_DT)
        if p:
            _lib.skx_free(p)
        return pairs, {f: getattr(info, f) for f, _ in SelectInfo._fields_}

    def distance_mst(self, min_freq=0.0, filt_ambig=True, max_snps=None, max_mismatches=None, band_rows=0):
        """skx_array_distance_mst: the lines of `distance_filtered`'s table that form its minimum spanning forest under the order (distance, i, j),
        among the lines the thresholds keep, held on the device band by band -> (pairs (PAIR_DT, ascending (i, j)), constant sites, rows used, info dict)"""
        spec = MstSpec.of(max_snps, max_mismatches, band_rows)
        p, n, cst, rows, info = C.c_void_p(), C.c_uint64(), C.c_int64(), C.c_uint64(), MstInfo()
        _check(_lib.skx_array_distance_mst(self.h, float(min_freq), int(filt_ambig), C.byref(spec), C.byref(p), C.byref(n), C.byref(cst), C.byref(rows), C.byref(info)))
        pairs = np.frombuffer(C.string_at(p, n.value * PAIR_DT.itemsize), PAIR_DT).copy() if n.value else np.zeros(0, PAIR_DT)
        if p:
            _lib.skx_free(p)
        return pairs, cst.value, rows.value, {f: getattr(info, f) for f, _ in MstInfo._fields_}

    def distance_mst_prefiltered(self, constant=0, filt_ambig=True, max_snps=None, max_mismatches=None, band_rows=0):
        """skx_array_distance_mst_prefiltered: the same of `distance`'s table (every row, `constant` added) -> (pairs, info dict)"""
        spec = MstSpec.of(max_snps, max_mismatches, band_rows)
        p, n, info = C.c_void_p(), C.c_uint64(), MstInfo()
        _check(_lib.skx_array_distance_mst_prefiltered(self.h, int(constant), int(filt_ambig), C.byref(spec), C.byref(p), C.byref(n), C.byref(info)))
        pairs = np.frombuffer(C.string_at(p, n.value * PAIR_DT.itemsize), PAIR_DT).copy() if n.value else np.zeros(0, PAIR_DT)
        if p:
            _lib.skx_free(p)
        return pairs, {f: getattr(info, f) for f, _ in MstInfo._fields_}

    def _banded_outputs(self, labels, tree):
        s = self.nsamples
        lab = np.zeros(max(s, 1), np.uint32) if labels else None
        joins = np.zeros(max(s - 1, 1), NJ_DT) if tree else None
        return s, lab, joins

    def distance_banded(self, min_freq=0.0, filt_ambig=True, labels=True, tree=False, cluster_snps=10.0, cluster_mismatches=1.0, band_rows=0):
        """skx_array_distance_banded: the clusters and / or the neighbour-joining joins of `distance_filtered`'s table from the banded sweep,
        the table never formed -> (labels (uint32: the lowest sample of each sample's cluster) or None, joins (NJ_DT) or None, constant sites,
        rows used, info dict)"""
        s, lab, joins = self._banded_outputs(labels, tree)
        spec, cst, rows, info = BandedSpec(float(cluster_snps), float(cluster_mismatches), int(band_rows)), C.c_int64(), C.c_uint64(), BandedInfo()
        _check(_lib.skx_array_distance_banded(self.h, float(min_freq), int(filt_ambig), C.byref(spec), _np_ptr(lab) if labels else None,
                                              _np_ptr(joins) if tree else None, C.byref(cst), C.byref(rows), C.byref(info)))
        return (lab[:s] if labels else None, joins[: max(s - 1, 0)] if tree else None, cst.value, rows.value,
                {f: getattr(info, f) for f, _ in BandedInfo._fields_})

    def distance_banded_prefiltered(self, constant=0, filt_ambig=True, labels=True, tree=False, cluster_snps=10.0, cluster_mismatches=1.0, band_rows=0):
        """skx_array_distance_banded_prefiltered: the same of `distance`'s table (every row, `constant` added) -> (labels, joins, info dict)"""
        s, lab, joins = self._banded_outputs(labels, tree)
        spec, info = BandedSpec(float(cluster_snps), float(cluster_mismatches), int(band_rows)), BandedInfo()
        _check(_lib.skx_array_distance_banded_prefiltered(self.h, int(constant), int(filt_ambig), C.byref(spec), _np_ptr(lab) if labels else None,
                                                          _np_ptr(joins) if tree else None, C.byref(info)))
        return lab[:s] if labels else None, joins[: max(s - 1, 0)] if tree else None, {f: getattr(info, f) for f, _ in BandedInfo._fields_}

    def distance_planes(self, filt_ambig=True):
        """device pointer to this array's bit planes [n_planes][n_samples][words_per_row] -> (ptr, words_per_row, n_planes)"""
        p, w, n = C.c_void_p(), C.c_uint64(), C.c_int()
        _check(_lib.skx_array_distance_planes(self.h, int(filt_ambig), C.byref(p), C.byref(w), C.byref(n)))
        return p.value, w.value, n.value

    def distance_tsv(self, min_freq=0.0, filt_ambig=True):
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.skh_distance_tsv(self.h, min_freq, int(filt_ambig), C.byref(p), C.byref(n)))
        return _take(p, n)

    def align(self, filter_type=FILTER_NO_CONST, mask_ambig=False, ignore_const_gaps=False, min_freq=0.9,
              filter_ambig_as_missing=False):
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.skh_align(self.h, filter_type, int(mask_ambig), int(ignore_const_gaps), min_freq,
                              int(filter_ambig_as_missing), C.byref(p), C.byref(n)))
        return _take(p, n)

    def free(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.skx_array_free(self.h)
            self.h = None

    def __del__(self):
        self.free()
