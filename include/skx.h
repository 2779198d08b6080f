/*
 * skx.h -- C ABI of the MI355X-native split-k-mer engine (libskx.so).
 *
 * Drop-in boundary for the build -> merge -> align/distance path of
 * bacpop/ska.rust v0.5.2.  The reference has no FFI layer; the seam is the
 * generic Rust API that lib.rs::main calls.  Every entry
 * point below cites the reference interface it replaces.  Plain pointers and
 * sizes only; no C++/torch types.  All functions return 0 on success and a
 * non-zero SKX_E* code on failure (skx_last_error() gives the message, which
 * matches the reference's panic text where one exists); nothing throws or
 * longjmps across the boundary.  Handles own host + device memory and are
 * released by the caller.  There is NO CPU fallback: every compute entry
 * point fails with SKX_ENODEV when no gfx950 device is usable.
 */
#ifndef SKX_H
#define SKX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKX_OK        0
#define SKX_EINVAL    1   /* bad argument (bad k, mismatched k/rc, ...)          */
#define SKX_EIO       2   /* unreadable / malformed input file                   */
#define SKX_ENODEV    3   /* no usable HIP device / HIP runtime error            */
#define SKX_ENOMEM    4
#define SKX_EEMPTY    5   /* "<file> has no valid sequence" (ska_dict.rs:374)    */
#define SKX_EUNSUP    6   /* feature not available on the device path            */
#define SKX_EFORMAT   7   /* .skf decode error (lets a u64 load fall through to u128, lib.rs:635-661) */

/* src/lib.rs QualFilter; src/cli.rs:27-29 defaults (min_count 5, min_qual 20, strict) */
enum { SKX_QUAL_NOFILTER = 0, SKX_QUAL_MIDDLE = 1, SKX_QUAL_STRICT = 2 };
/* src/cli.rs FilterType */
enum { SKX_FILTER_NONE = 0, SKX_FILTER_NO_CONST = 1, SKX_FILTER_NO_AMBIG = 2, SKX_FILTER_NO_AMBIG_OR_CONST = 3 };

/* QualOpts (src/lib.rs; used by merge_ska_dict.rs:354-361, ska_dict.rs:333-341) */
typedef struct {
    uint16_t min_count;
    uint8_t  min_qual;
    int32_t  qual_filter;
} skx_qual;

typedef struct { uint64_t lo, hi; } skx_key;   /* split k-mer as the reference encodes it; hi == 0 for k <= 31 */

typedef struct skx_ctx     skx_ctx;      /* one per GPU / process                                   */
typedef struct skx_dictset skx_dictset;  /* a batch of per-sample SkaDicts, device resident         */
typedef struct skx_keyset  skx_keyset;   /* sorted unique split k-mers (rows of a merged array)     */
typedef struct skx_array   skx_array;    /* MergeSkaArray: keys + samples x k-mers middle bases     */

const char *skx_last_error(void);
const char *skx_version(void);            /* "0.5.2": the ska_version written into .skf files      */

int  skx_ctx_create(int device, skx_ctx **out);
void skx_ctx_destroy(skx_ctx *ctx);
int  skx_ctx_sync(skx_ctx *ctx);          /* drain the context's HIP stream                         */
void *skx_ctx_stream(skx_ctx *ctx);       /* the hipStream_t all kernels of this ctx are launched on */

/* ------------------------------------------------------------------------------------------
 * Record stream: what the host reader hands to the device in place of needletail's record
 * iterator (ska_dict.rs:131-153).  Each record's bases (line breaks removed) followed by one
 * '\n'; `qual` (FASTQ only) has the same layout.  Pointers are host memory unless on_device.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const uint8_t *seq;
    const uint8_t *qual;      /* NULL for FASTA input */
    uint64_t       len;       /* bytes in seq (and qual) */
} skx_stream;

/* SkaDict::new for a batch of samples (ska_dict.rs:333-378; one GPU unit of work per sample,
 * merge_ska_dict.rs:244,404).  k odd in 5..=63 else SKX_EINVAL "Invalid k-mer length".
 * A sample without any split k-mer -> SKX_EEMPTY.  FASTQ streams (qual != NULL) apply the
 * quality rules of split_kmer.rs:66-71,328-339 and the KmerFilter of bloom_filter.rs:116-148. */
int skx_dictset_build(skx_ctx *ctx, const skx_stream *samples, int n_samples, int on_device,
                      int k, int rc, const skx_qual *qual, skx_dictset **out);
/* same, reading FASTA/FASTQ(.gz) files with the library's own reader (needletail replacement).
 * file2[i] may be NULL.  proportion_reads 0 == None (ska_dict.rs:125-141). */
int skx_dictset_build_files(skx_ctx *ctx, const char *const *file1, const char *const *file2, int n_samples,
                            int k, int rc, const skx_qual *qual, int threads, double proportion_reads,
                            skx_dictset **out);
/* One sample's files as the record stream skx_dictset_build takes: what needletail's parse_fastx_file hands SkaDict::new record by
 * record (ska_dict.rs:131-153, 356-366) -- each record's bases (and qualities) followed by '\n'.  Host only, no device: plain, gzip
 * (the library's own inflater; members' CRC-32 and length checked: a damaged or truncated file is SKX_EIO), bzip2 / xz / zstd; FASTA or
 * FASTQ.  streaming != 0: through the line-by-line FASTQ reader of the read-set pipeline (SKX_EUNSUP: not FASTQ).  seq / qual:
 * malloc'd (skx_free); *qual = NULL for FASTA. */
int skx_read_records(const char *file1, const char *file2, double proportion_reads, int streaming, uint8_t **seq, uint8_t **qual, uint64_t *len);
void skx_dictset_free(skx_dictset *d);
int  skx_dictset_nsamples(const skx_dictset *d);
int  skx_dictset_key_bits(const skx_dictset *d);      /* 64 | 128 (lib.rs:592) */
/* SkaDict::ksize / kmers() (ska_dict.rs:499-512): entry count, then copy-out sorted by key */
int  skx_dictset_size(skx_dictset *d, int sample, uint64_t *n);
int  skx_dictset_export(skx_dictset *d, int sample, skx_key *keys, uint8_t *bases, uint64_t cap);

/* ------------------------------------------------------------------------------------------
 * MergeSkaDict::append/merge + MergeSkaArray::new (merge_ska_dict.rs:77-151,
 * merge_ska_array.rs:166-186), split so that a multi-GPU host can all-gather key tables
 * between the two halves:
 *   skx_keyset_union   : distinct split k-mers over all samples of the dictset
 *   skx_keyset_device / skx_keyset_from_device / skx_keyset_merge : exchange + combine tables
 *   skx_array_assemble : rows = keyset, columns = the dictset's samples ('-' where absent)
 * skx_merge() is the single-GPU composition of the three.
 * ------------------------------------------------------------------------------------------ */
int  skx_keyset_union(skx_ctx *ctx, skx_dictset *d, skx_keyset **out);
/* The same pass, which also keeps its notes (2 bytes per dictionary word: which row of its sub-bucket the word's key became, which bases)
 * for the skx_array_assemble over the same dictset that follows -- directly, or on the global rows skx_keyset_allgather returns for this
 * key set (the notes travel with it): the matrix is then filled without a second read of the dictionaries, as skx_merge does on one GPU
 * (merge_ska_dict.rs:77-109 appends a sample in one pass over its dictionary).  Costs the notes' memory until the key set / the rows are freed. */
int  skx_keyset_union_notes(skx_ctx *ctx, skx_dictset *d, skx_keyset **out);
int  skx_keyset_size(const skx_keyset *ks, uint64_t *n);
/* device pointer to n packed 64-bit words per key (1 for k<=31, 2 above), engine order */
int  skx_keyset_device(skx_keyset *ks, const void **dptr, uint64_t *n_keys, int *words_per_key);
int  skx_keyset_from_device(skx_ctx *ctx, const void *dptr, uint64_t n_keys, int k, int rc, skx_keyset **out);
int  skx_keyset_merge(skx_ctx *ctx, skx_keyset *const *sets, int n_sets, skx_keyset **out);
void skx_keyset_free(skx_keyset *ks);
int  skx_array_assemble(skx_ctx *ctx, skx_dictset *d, skx_keyset *rows, const char *const *names, skx_array **out);
/* The same array held as rows + dictionaries (no rows x samples matrix until an operation needs one: skx_array_device_stats gathers
 * the row statistics alone, skx_array_filter then writes only the kept rows, skx_array_save streams windows).  TAKES OWNERSHIP of d and
 * rows, also on failure: a multi-GPU rank's column slab over the global rows of 8 000 samples is 100+ GB it need not allocate. */
int  skx_array_assemble_lazy(skx_ctx *ctx, skx_dictset *d, skx_keyset *rows, const char *const *names, skx_array **out);
int  skx_merge(skx_ctx *ctx, skx_dictset *d, const char *const *names, skx_array **out);

/* build_and_merge (merge_ska_dict.rs:354-417) + MergeSkaArray::new: the `ska build` body.
 * When the samples' dictionaries do not fit in free device memory together (estimate from the file sizes, 60 % of free
 * HBM; SKX_BUILD_BATCH_MB overrides the budget), consecutive batches of samples are built and joined by the
 * skx_array_merge row-set path; a batch that still runs out of memory is halved and retried.  Same rows, columns and
 * sample order as a single batch. */
int skx_build_and_merge(skx_ctx *ctx, const char *const *names, const char *const *file1, const char *const *file2,
                        int n_samples, int k, int rc, const skx_qual *qual, int threads, double proportion_reads,
                        skx_array **out);

/* ------------------------------------------------------------------------------------------ MergeSkaArray */
void skx_array_free(skx_array *a);
/* save / load (merge_ska_array.rs:191-204): snappy-frame(CBOR), want_bits 64|128|0 */
int  skx_array_save(skx_array *a, const char *path);
int  skx_array_load(skx_ctx *ctx, const char *path, int want_bits, skx_array **out);
/* load + filter in one pass over the file (the body of `ska align x.skf` and `ska distance x.skf`): the same array as
 * skx_array_load followed by generic_modes::apply_filters (generic_modes.rs:112-131: threshold ceil(n_samples * min_freq),
 * update_kmers = false), or -- two_stage != 0 -- by the two filters of generic_modes::distance (generic_modes.rs:149-168: NoFilter
 * at ceil(n_samples * min_freq) when min_freq * n_samples >= 1, then NoConst at 0; *constant = rows the second one removed).
 * Rows are filtered as they come off the decoder, so the unfiltered rows x samples matrix never exists on the device and the
 * split k-mer list is not decoded (the resulting array has no keys: save / merge / weed / map on it fail with SKX_EINVAL).
 * Files the one-pass reader does not take (k > 31, unusual field order, stored counts that differ from the rows) go through
 * skx_array_load + skx_array_filter inside the call. */
typedef struct { double min_freq; int32_t filter_ambig_as_missing, filter_type, mask_ambig, ignore_const_gaps, two_stage; } skx_filter_spec;
int  skx_array_load_filtered(skx_ctx *ctx, const char *path, const skx_filter_spec *f, skx_array **out, int64_t *removed, int64_t *constant);
/* construct from host data (row-major [n_rows, n_samples] as in the .skf) */
int  skx_array_from_host(skx_ctx *ctx, int k, int rc, const char *const *names, int n_samples,
                         const skx_key *keys, const uint8_t *variants, const uint64_t *variant_count /* NULL: recount */,
                         uint64_t n_rows, const char *version, skx_array **out);
typedef struct {
    int32_t  k, rc, k_bits;
    uint64_t n_kmers;      /* split_kmers.len() */
    uint64_t n_rows;       /* variants.nrows()  */
    uint64_t n_samples;    /* columns held by this array                                  */
    uint64_t total_samples;/* samples over all ranks when this array is one column slab (== n_samples otherwise) */
} skx_array_info_t;
int  skx_array_info(const skx_array *a, skx_array_info_t *info);
const char *skx_array_name(const skx_array *a, uint64_t i);
const char *skx_array_version(const skx_array *a);
/* copy-out, rows sorted by key: keys[n_kmers], variants row-major [n_rows, n_samples], counts[n_rows] */
int  skx_array_export(skx_array *a, skx_key *keys, uint8_t *variants, uint64_t *counts);
/* n_sample_kmers (merge_ska_array.rs:554-559) */
int  skx_array_sample_kmers(skx_array *a, int64_t *out);
/* an array still held as the append pass left it (pieces of 4-bit base sets by first-seen rank: csrc/skx_append.hip): bytes of pieces written,
 * row blocks, ranks per block; *piece_bytes = 0 when the array holds a matrix instead.  No counterpart in the reference (its merged dictionary
 * holds a Vec<u8> per row, merge_ska_dict.rs:41-58); bench.py prices the append kernel's needed traffic with it. */
int  skx_array_pieces_info(skx_array *a, uint64_t *piece_bytes, uint64_t *row_blocks, uint32_t *ranks_per_block);
/* MergeSkaArray::filter (merge_ska_array.rs:289-402); *removed = its i32 return value */
int  skx_array_filter(skx_array *a, uint64_t min_count, int filter_ambig_as_missing, int filter_type,
                      int mask_ambig, int ignore_const_gaps, int update_kmers, int32_t *removed);
/* Optional hint before skx_array_load_filtered: the array about to be loaded will be written with skx_array_write_fasta to `fd` (a
 * regular file opened read-write, at its current offset).  The engine then allocates the file's pages while the rows are still
 * being read -- page allocation, not copying, is what bounds a 5 GB alignment on tmpfs.  No effect on the bytes written. */
int  skx_ctx_expect_output(skx_ctx *ctx, int fd);
/* write_fasta (merge_ska_array.rs:499-517): ">name\nSEQ\n" per sample to fd */
int  skx_array_write_fasta(skx_array *a, int fd);
/* same into a malloc'd buffer (free with skx_free) */
int  skx_array_fasta(skx_array *a, char **buf, uint64_t *len);
/* device view of the sample-major middle-base matrix: row s = sample s, pitch bytes apart */
int  skx_array_device_matrix(skx_array *a, const uint8_t **dptr, uint64_t *pitch, uint64_t *n_rows);

/* multi-GPU column slabs: device views of the per-row statistics the filter reads
 * (cells != '-', cells in ACGT, set of IUPAC codes present, stored variant_count; u32 each, n_rows long) so that
 * the host can reduce them across ranks, and the global sample count the gap test must use */
int  skx_array_device_stats(skx_array *a, uint32_t **present, uint32_t **unambig, uint32_t **mask, uint32_t **variant_count);
int  skx_array_set_total_samples(skx_array *a, uint64_t total_samples);

typedef struct { double distance, mismatch_prop; uint64_t match_count, mismatch_count; } skx_dist;
/* MergeSkaArray::distance (merge_ska_array.rs:416-438,587-632): upper triangle, pairs (i<j) row-major.  filt_ambig = 0 (--allow-ambiguous):
 * rows in which no cell is ambiguous -- the array's row statistics say which -- are counted by the 4-plane sweep, the others by the
 * twelve-class one; the sums are the reference's per-row sums either way.  SKX_EINVAL for a null array or table, like every form below */
int  skx_array_distance(skx_array *a, double constant, int filt_ambig, skx_dist *out);
/* generic_modes::distance (generic_modes.rs:136-189) in one call that leaves the array as it is: rows below ceil(n_samples *
 * min_freq) (when min_freq * n_samples >= 1) and constant rows are skipped while the bit planes are built (*constant = rows the
 * NoConst stage removes, added to every pair's matches), instead of being filtered out of the matrix first.  Same numbers as
 * skx_array_filter x 2 + skx_array_distance. */
int  skx_array_distance_filtered(skx_array *a, double min_freq, int filt_ambig, skx_dist *out, int64_t *constant, uint64_t *rows_used);
/* The rows of that table that hold a query sample (`ska distance --query`): query = n_query distinct sample indices in any order,
 * out = n_query x n_samples row-major, out[q * n_samples + j] = the pair (query[q], j) with the numbers skx_array_distance /
 * skx_array_distance_filtered give it (same planes, same counts, same arithmetic); the entry j == query[q] is zeroed.  The filters stay
 * those of the whole array: thresholds, *constant and the kept rows are the full table's.  The bit planes are built with the queries in
 * front and the pair sweep runs over the band of the queries, so the count buffers are n_query x n_samples pairs, not n_samples^2.
 * SKX_EINVAL with a message for an index out of range, a repeated index or n_query < 1.  The array is left as it is; both key widths
 * and arrays held as pieces are taken. */
int  skx_array_distance_query(skx_array *a, double constant, int filt_ambig, const int *query, int n_query, skx_dist *out);
int  skx_array_distance_query_filtered(skx_array *a, double min_freq, int filt_ambig, const int *query, int n_query,
                                       skx_dist *out, int64_t *constant, uint64_t *rows_used);
/* The lines of that table a user of a large collection asks for (`ska distance --max-snps / --max-mismatches / --closest`; the reference leaves
 * the selection to scripts/cluster_dists.py), picked on the device band by band over the pair matrix, so that device and host memory are
 * O(band x n_samples + selected pairs) instead of O(n_samples^2).  A pair's values are the skx_dist skx_array_distance_filtered gives it, compared
 * as those doubles: max_snps keeps distance <= max_snps, max_mismatches keeps mismatch_prop <= max_mismatches; a pair that passes every threshold
 * given is a candidate.  closest = K: for every sample its candidate partners ordered by (distance, partner index), the first min(K, how many)
 * of them its nearest; a pair is kept when either of its samples has the other among its nearest.  K >= n_samples - 1 is no constraint.
 * band_rows: first samples of the pair matrix swept at a time (any positive value is taken as given). */
typedef struct {
    double  max_snps;        /* < 0: none */
    double  max_mismatches;  /* < 0: none; at most 1 */
    int32_t closest;         /* 0: none; at most 1 024 unless >= n_samples - 1 */
    int32_t band_rows;       /* 0: the engine's choice -- the largest multiple of 64 whose count buffer stays within 1 GiB, at least 64 */
} skx_select_spec;
typedef struct { uint32_t i, j; skx_dist d; } skx_dist_pair;               /* i < j: sample indices; d: bit for bit the full table's entry */
/* what a call did: bands swept, first samples per band, bytes of the device count buffer, pairs that passed the thresholds */
typedef struct { uint64_t bands, band_rows, count_buffer_bytes, candidates; } skx_select_info;
/* pairs: malloc'd (skx_free), n_pairs of them ascending by (i, j), i.e. in the table's order; constant / rows_used as skx_array_distance_filtered
 * reports them; info may be NULL.  SKX_EINVAL with a message that begins "distance select:" for a NaN, max_mismatches > 1, closest < 0,
 * 1 024 < closest < n_samples - 1, band_rows < 0 or none of the three criteria given.  Fewer than two samples: zero pairs.  The array is left as
 * it is; both key widths and arrays held as pieces are taken. */
int  skx_array_distance_select(skx_array *a, double min_freq, int filt_ambig, const skx_select_spec *spec, skx_dist_pair **pairs, uint64_t *n_pairs,
                               int64_t *constant, uint64_t *rows_used, skx_select_info *info);
/* The same selection on an array the two filters have been applied to already (skx_array_load_filtered), as skx_array_distance_query is to
 * skx_array_distance_query_filtered: every row is swept and `constant` (>= 0, else SKX_EINVAL) is added to every pair's matches. */
int  skx_array_distance_select_prefiltered(skx_array *a, int64_t constant, int filt_ambig, const skx_select_spec *spec, skx_dist_pair **pairs,
                                           uint64_t *n_pairs, skx_select_info *info);
/* The minimum spanning forest of that table (`ska distance --mst`): the candidates are the lines that pass max_snps / max_mismatches as for
 * skx_array_distance_select (every line when neither is given); the lines are ordered by (distance, i, j) -- the distance, then the line's place
 * in the table -- which is strict, so the forest is unique: n_samples - (connected components of the candidates) lines.  Cut at L it gives the
 * single-linkage clusters of every threshold L at once.  Kept on the device across the bands of the same sweep (after a band: the forest of the
 * bands so far; the next band merges its candidates in by Boruvka rounds), in O(n_samples) memory beside the band's count buffer.  The device
 * orders by the exact integer numerator of the distance, which orders as the float64 value and as its two printed decimals do. */
typedef struct { double max_snps, max_mismatches; int32_t band_rows; } skx_mst_spec;   /* thresholds as skx_select_spec: < 0 = not set; band_rows as there */
/* what a call did: bands swept, first samples per band, bytes of the device count buffer, pairs that passed the thresholds, the forest's lines,
 * its trees (n_samples - edges), the most rounds a band took to merge */
typedef struct { uint64_t bands, band_rows, count_buffer_bytes, candidates, edges, components, rounds; } skx_mst_info;
/* pairs: malloc'd (skx_free), n_pairs of them ascending by (i, j), every d bit for bit the full table's entry; constant / rows_used as
 * skx_array_distance_filtered reports them; info may be NULL.  SKX_EINVAL with a message that begins "distance mst:" for a NaN threshold,
 * max_mismatches > 1 or band_rows < 0; SKX_EUNSUP with the same beginning above 65 536 samples, or at 2^32 / 36 swept rows and more (an edge is
 * one 64-bit word: the numerator, 16 bits a sample).  Fewer than two samples: zero pairs.  The array is left as it is; both key widths and arrays
 * held as pieces are taken. */
int  skx_array_distance_mst(skx_array *a, double min_freq, int filt_ambig, const skx_mst_spec *spec, skx_dist_pair **pairs, uint64_t *n_pairs,
                            int64_t *constant, uint64_t *rows_used, skx_mst_info *info);
/* The same on an array the two filters have been applied to already, as skx_array_distance_select_prefiltered is to skx_array_distance_select
 * (constant >= 0, else SKX_EINVAL) */
int  skx_array_distance_mst_prefiltered(skx_array *a, int64_t constant, int filt_ambig, const skx_mst_spec *spec, skx_dist_pair **pairs,
                                        uint64_t *n_pairs, skx_mst_info *info);
/* The two halves of skx_array_distance, so that a multi-GPU host can exchange the bit planes between them (SURVEY.md 8e:
 * "tile the pair matrix over ranks"): every rank builds the planes of its own samples over the (globally filtered) rows, the
 * planes are all-gathered (plane-major: planes[p][sample][word], 4 planes with filt_ambig, 8 without), and each rank
 * finishes a band of first samples [i_lo, i_hi) against every later sample -- `out` = those pairs, (i, j > i) row-major, in the
 * arithmetic of merge_ska_array.rs:596-631.  Any 0 <= i_lo < i_hi <= n_samples (pair tiles start at i_lo).  The planes pointer stays valid while the array lives. */
int  skx_array_distance_planes(skx_array *a, int filt_ambig, const void **planes, uint64_t *words_per_row, int *n_planes);
int  skx_planes_distance(skx_ctx *ctx, const void *planes, int n_samples, uint64_t words_per_row, int filt_ambig, double constant,
                         int i_lo, int i_hi, skx_dist *out);
void skx_free(void *p);

/* ------------------------------------------------------------------------------------------
 * Collectives: the exchanges of a job whose samples are sharded over the GPUs of a node, one process per
 * GPU.  They stand where the reference's build_and_merge joins the dictionaries of its worker threads (merge_ska_dict.rs:354-417:
 * samples dealt to threads in input order, per-thread dictionaries merged pairwise) -- here the "threads" are ranks, each rank keeps
 * the columns of its own samples, and what is exchanged is the row set (one all-gather of the per-rank key tables), the per-row
 * filter statistics, and for `ska distance` the bit planes.  Transport: RCCL over xGMI on the context's stream
 * (skx_comm_create; librccl is opened at run time), or a host-staged exchange through a directory on tmpfs for ranks that share one
 * device, which RCCL refuses (skx_comm_create_local; tests and single-GPU emulation of an N-rank job).  The host launches the
 * processes and carries the 128-byte id from rank 0 to the others (a file, an environment variable, MPI, a torch store ...).
 * Every call below is collective: all ranks of the communicator make it, in the same order.
 * ------------------------------------------------------------------------------------------ */
typedef struct skx_comm skx_comm;
#define SKX_COMM_ID_BYTES 128
int  skx_comm_unique_id(uint8_t id[SKX_COMM_ID_BYTES]);                        /* ncclGetUniqueId; rank 0 only */
int  skx_comm_create(skx_ctx *ctx, int rank, int world, const uint8_t id[SKX_COMM_ID_BYTES], skx_comm **out);   /* ncclCommInitRank on ctx's device */
/* host-staged transport: `dir` is a fresh directory every rank can reach (NULL at world 1: the library makes its own and removes it with the
 * communicator); ctx may be NULL when only host buffers are exchanged */
int  skx_comm_create_local(skx_ctx *ctx, int rank, int world, const char *dir, skx_comm **out);
void skx_comm_destroy(skx_comm *c);
int  skx_comm_rank(const skx_comm *c);
int  skx_comm_world(const skx_comm *c);
uint64_t skx_comm_bytes_received(const skx_comm *c);                           /* payload this rank has received so far (reports) */
/* what the communicator runs on: *rccl_ranks = ncclCommCount of the RCCL communicator (0: the host-staged transport), *rccl_device = the
 * device RCCL bound it to (ncclCommCuDevice; -1: none), *ctx_device = the engine context's device.  A report for a job's first contact with
 * a node (bench.py prints them per rank); stands where merge_ska_dict.rs:354-417 logs its thread count. */
int  skx_comm_transport(const skx_comm *c, int *rccl_ranks, int *rccl_device, int *ctx_device);
int  skx_comm_barrier(skx_comm *c);
/* the two primitives the exchanges are made of, for hosts with exchanges of their own: `bytes` from every rank, rank r's at
 * recv + r * bytes (recv must not overlap send); in-place sum of n 32-bit counters.  on_device: the pointers are device memory
 * (required by the RCCL transport). */
int  skx_comm_allgather(skx_comm *c, const void *send, void *recv, uint64_t bytes, int on_device);
int  skx_comm_allreduce_u32(skx_comm *c, uint32_t *buf, uint64_t n, int on_device);
/* host blocks of different sizes (sizes[world], known to every rank) to rank 0: recv there = the blocks in rank order */
int  skx_comm_gather_root(skx_comm *c, const void *send, const uint64_t *sizes, void *recv);
/* partitioning, pure arithmetic: the contiguous shard [lo, hi) of `rank` (input order kept, so names stay in CLI order, cf. the
 * offsets of merge_ska_dict.rs:243-253,277-291), and the bands of first samples of the pair matrix (lo_hi[2 r], lo_hi[2 r + 1];
 * starts on multiples of `align`, about the same number of pairs each, merge_ska_array.rs:416-438 order kept) */
int  skx_shard_range(uint64_t n_items, int rank, int world, uint64_t *lo, uint64_t *hi);
int  skx_pair_bands(int n_samples, int world, int align, int *lo_hi);
/* exchange 1: one all-gather of the per-rank key tables (padded to the longest) + their union: every rank gets the same global
 * row set, which skx_array_assemble / skx_array_assemble_lazy then fills with the rank's own columns.  SKX_EINVAL with the
 * reference's "K-mer lengths do not match" / "Strand use inconsistent" when ranks disagree. */
int  skx_keyset_allgather(skx_comm *c, skx_keyset *local, skx_keyset **rows);
/* exchange 2: the per-row statistics the filter reads, over all ranks (counts summed in one all-reduce, 16-bit code sets
 * all-gathered and OR-ed); variant_count becomes the global count, the array's total_samples the job's sample count */
int  skx_array_reduce_stats(skx_comm *c, skx_array *a, uint64_t total_samples);
/* exchange 3: MergeSkaArray::distance (merge_ska_array.rs:416-438,587-632) for a sharded job: `a` = this rank's samples over the
 * globally filtered rows; one all-gather of the bit planes (--allow-ambiguous: one all-reduce of a byte per row first, so that the ranks
 * agree on the rows without an ambiguous cell, which travel as 4 planes; the others as 8), each rank finishes a band of the pair
 * matrix, rank 0 receives all pairs: out[n_out], n_out >= S (S - 1) / 2 there (ignored elsewhere) */
int  skx_array_distance_sharded(skx_comm *c, skx_array *a, int filt_ambig, double constant, skx_dist *out, uint64_t n_out);


/* ---- .skf life-cycle: `ska merge`, `ska delete`, `ska weed` ---- */
/* generic_modes::merge (generic_modes.rs:90-106) = MergeSkaArray::to_dict (merge_ska_array.rs:208-222) +
 * MergeSkaDict::extend (merge_ska_dict.rs:160-193) folded over the inputs + MergeSkaArray::new (:166-186): rows = union of
 * the inputs' split k-mers, columns = their samples in order, absent cells '-'.  SKX_EINVAL with the reference's panic
 * texts "K-mer lengths do not match: a b" / "Strand use inconsistent". */
int  skx_array_merge(skx_ctx *ctx, skx_array *const *arrays, int n_arrays, skx_array **out);
/* MergeSkaArray::delete_samples (merge_ska_array.rs:231-271) incl. update_counts(false): rows no remaining sample has are
 * dropped.  SKX_EINVAL "Invalid number of samples to remove" / "Could not find sample(s): {..}" where it panics. */
int  skx_array_delete_samples(skx_array *a, const char *const *names, int n_names);
/* `ska align --groups / --samples`: the alignment of a subset of the samples without the .skf in between -- MergeSkaArray::delete_samples of
 * everybody else (merge_ska_array.rs:231-271, with its update_counts(false), :139-163: rows no sample of the subset has are dropped and the
 * counts become the cells present) followed by generic_modes::apply_filters (generic_modes.rs:112-131: threshold ceil(n_samples * min_freq)
 * over the subset, update_kmers = false) = MergeSkaArray::filter (merge_ska_array.rs:289-402), decided per row in one pass over the subset's
 * cells.  samples = n_samples distinct indices into `a` in any order; *out = a new array on a's context holding the kept rows in a's row
 * order and the subset's samples in ascending index (as the delete leaves them), mask_ambig applied.  Like the result of
 * skx_array_load_filtered it has no split k-mers: save / merge / weed / map on it fail with SKX_EINVAL; write_fasta / fasta / info / name work.
 * info (may be NULL): rows_present = rows left by the delete (what `ska nk` would print), removed = the filter's return value, silent = rows
 * update_counts(true) drops uncounted (filter_ambig_as_missing: no unambiguous cell), sites = rows of *out.  out may be NULL: the counts alone.
 * `a` keeps its content (an array held as pieces or lazily is materialised first); both key widths are taken; a subset of all samples is
 * allowed.  The n_samples x rows matrix of the unfiltered subset is never allocated.  SKX_EINVAL with a message that begins "subset:" for
 * n_samples < 1, an index out of range, a repeated index, two_stage != 0, min_freq outside [0, 1] or NaN. */
typedef struct { uint64_t rows_present, removed, silent, sites; } skx_subset_info;
int  skx_array_subset_filtered(skx_array *a, const int *samples, int n_samples, const skx_filter_spec *f,
                               skx_array **out, skx_subset_info *info);
/* `ska markers`: which split k-mers, and which middle-base alleles, tell one group of samples from everybody else -- for every group of a
 * partition from a number of passes over the matrix that does not depend on how many groups there are.  The reference has no counterpart: its
 * users chain delete_samples of a group (merge_ska_array.rs:231-271) and the Debug output of `ska nk --full-info` (:649-698) once per group and
 * compare the text (SKA 1 had `ska unique`).
 * Inputs.  The array holds S samples and U rows.  Cells are bytes; code(cell) is the 4-bit IUPAC set (A 1, C 2, T 4, G 8; '-' and the 0 byte
 * are 0).  A partition assigns every sample to exactly one segment: segments 0..G-1 are the groups (of the file, in the order their labels first
 * appear); samples no group lists form one further, unnamed segment, which is never reported -- its samples still count as "others".
 * Per-row quantities for a reported group g (n = its size): in = cells of g with code != 0; out = cells of all other samples with code != 0;
 * bases_in / bases_out = OR of the codes on each side.
 * Thresholds, computed in doubles exactly like this: t_in = max(1, (uint64)ceil(n * P)), t_out = (uint64)floor((S - n) * Q).
 * Kinds.  presence marker of g: in >= t_in and out <= t_out.  allele marker of g: in >= t_in, not a presence marker, and
 * bases_in & bases_out == 0.  An ambiguous cell stands for all its bases, which is conservative.  A row can be a marker of several groups; it is
 * a marker of one group at most once.
 * segment_of[S]: the segment of every sample, n_groups for the unnamed one; reported[n_groups]: non-zero = this group's markers are wanted (a
 * group that is not reported still counts as others); P = min_in, Q = max_out; kinds: SKX_MARKER_PRESENCE | SKX_MARKER_ALLELE (which of the two
 * are returned; an allele marker is never a presence marker, whichever are asked for).  records / keys: malloc'd (skx_free), n of each, sorted by
 * (group, row index in the array's current order); keys[i] = the record's split k-mer as skx_array_export gives keys; info (n_groups, may be
 * NULL): the records of each kind per group.  The records are counted before their buffer is allocated: when they do not fit, SKX_ENOMEM with
 * a message.  SKX_EINVAL with a message that begins "markers:" for P or Q outside [0, 1] or NaN, a segment index out of range, a reported group
 * without samples, kinds == 0 or unknown bits, an array without split k-mers (skx_array_load_filtered, skx_array_subset_filtered); SKX_EUNSUP with
 * the same beginning above 65 535 samples or segments.  `a` keeps its content (an array held as pieces or lazily is materialised first); both
 * key widths are taken.  Device memory beside the array: 12 bytes a row, 16 a group, 68 a record while they are sorted. */
enum { SKX_MARKER_PRESENCE = 1, SKX_MARKER_ALLELE = 2 };
typedef struct {
    uint64_t row;                      /* row index in the array's current order */
    uint32_t group, n_in, n_out;       /* in, out */
    uint8_t  kind;                     /* SKX_MARKER_PRESENCE or SKX_MARKER_ALLELE */
    uint8_t  bases_in, bases_out, reserved;
} skx_marker;
typedef struct { uint64_t presence, allele; } skx_marker_info;
int  skx_array_group_markers(skx_array *a, const int32_t *segment_of, int n_groups, const uint8_t *reported, double min_in, double max_out, int kinds,
                             skx_marker **records, skx_key **keys, uint64_t *n, skx_marker_info *info);
/* `ska distance --sites`: which rows make up the distance of a pair, and which base each of the two samples carries there.  The reference has no
 * counterpart: its users run `ska delete` down to the pair (merge_ska_array.rs:231-271), `ska align` and `ska nk --full-info` and compare columns.
 * Definition.  The array holds S samples and U rows, in its current order.  Cells are bytes; code(cell) is the 4-bit IUPAC set as above
 * (skx_array_group_markers); a cell is unambiguous when popcount(code) == 1.  A row is swept when it passes the two filters of
 * generic_modes::distance for min_freq -- the rows the distance entry points build their planes over: the threshold ceil(S * min_freq) when
 * min_freq * S >= 1, then NoConst.
 *     sites(i, j) = { r swept : M[i][r] and M[j][r] unambiguous and M[i][r] != M[j][r] },  r ascending        (i < j)
 * |sites(i, j)| is the `distance` skx_array_distance_filtered gives the pair with filt_ambig, exactly; without filt_ambig distances are fractional
 * sums over base-set overlaps and sites are not defined.  (The NoConst stage never removes a site row: two different unambiguous bases make the
 * row non-constant.  Only the frequency threshold can.)
 * ij = n_pairs x (i, j) with i < j < S, in any order; a pair given twice gets two runs of records.  records: malloc'd (skx_free), n of them,
 * sorted by (pair, row) -- the order of ij, then ascending rows; pair = the index into ij, row = the index in the array's current order, the bases
 * as ASCII.  keys may be NULL; otherwise keys[n] (malloc'd) = the record's split k-mer as skx_array_group_markers returns keys; both key widths
 * are taken.  counts (n_pairs entries, the caller's memory) may be NULL; otherwise counts[p] = |sites| of pair p.
 * The records are counted exactly before anything is allocated for them: max_records > 0 and a larger total is SKX_ENOMEM with a message naming
 * both numbers, and so are records that do not fit the device or the host; counts is filled even then, so that a caller can size a second call.
 * SKX_EINVAL with a message that begins "pair sites:" for i >= j, an index outside the array, NaN or min_freq outside [0, 1], keys != NULL on an
 * array without split k-mers (skx_array_load_filtered, skx_array_subset_filtered).  n_pairs == 0 or U == 0: SKX_OK with *n = 0.  `a` keeps its
 * content (an array held as pieces or lazily is materialised first).  Device memory beside the array: a byte a row, 8 bytes per pair and 4 096
 * rows, 16 bytes a record (32 with keys). */
typedef struct { uint64_t row; uint32_t pair; uint8_t base_i, base_j, reserved[2]; } skx_pair_site;
int  skx_array_pair_sites(skx_array *a, double min_freq, const uint32_t *ij, uint64_t n_pairs, uint64_t max_records,
                          skx_pair_site **records, skx_key **keys, uint64_t *counts, uint64_t *n);
/* `ska curve`: how the collection behaves as it grows -- the rows present, the rows that pass a frequency threshold and the variant sites after
 * each sample of an order has been added, for any number of orders from one load.  The reference has no counterpart: `ska nk` prints one number
 * for the whole file, and its users chain `ska delete` down to a prefix (merge_ska_array.rs:231-271) and `ska align` once per prefix and shuffle.
 * Definition.  The array holds S samples and U rows, in its current order.  code(cell) is the 4-bit IUPAC set as above (skx_array_group_markers:
 * A 1, C 2, T 4, G 8; '-' and the 0 byte are 0); a cell is unambiguous when popcount(code) == 1.  An order is a permutation o[0..S) of the sample
 * indices.  For t = 1..S the prefix is o[0..t); per row n = cells of the prefix with code != 0 and B = OR of the codes of its unambiguous cells.
 * The threshold, computed in doubles exactly like this: thr(t) = max(1, (uint64)ceil(t * min_freq)).  Four counts over the rows per (order, t):
 *     pan           n >= 1                           the rows `ska delete` of everybody outside the prefix leaves
 *     core          n >= thr(t)                      the rows --min-freq f --filter no-filter keeps on the prefix
 *     variant       popcount(B) >= 2
 *     core_variant  n >= thr(t) and popcount(B) >= 2   the columns of `ska align --min-freq f --filter no-ambig-or-const --no-gap-only-sites`
 * core is not monotone in t when min_freq < 1: it is counted at every step.
 * orders: n_orders x S sample indices, every run of S a permutation; counts: the caller's memory, n_orders x S x 4 in the order pan, core,
 * variant, core_variant (counts[(p * S + t - 1) * 4 + c]).  `a` keeps its content (an array held as pieces or lazily is materialised first);
 * both key widths are taken, and so is an array without split k-mers (skx_array_load_filtered, skx_array_subset_filtered): nothing here needs
 * keys.  SKX_EINVAL with a message that begins "curve:" for NULL arguments, n_orders == 0, NaN or min_freq outside [0, 1], a run that is not a
 * permutation (a repeat, an index out of range), a cell outside the alphabet; SKX_EUNSUP with the same beginning above 65 535 samples.  U == 0:
 * SKX_OK with zeros.  The results are sums of integers: the same bytes whatever the order of arrival.
 * One workgroup walks one order over SKX_CURVE_TILE_ROWS rows and keeps SKX_CURVE_LDS_STEPS steps of counters on chip at a time; a launch takes
 * at most SKX_CURVE_BATCH_ORDERS orders and 2^22 (order, step) pairs.  Device memory beside the array: 36 bytes per (order, step) of a launch
 * (at most 151 MB) and 4 S bytes of thresholds. */
enum { SKX_CURVE_TILE_ROWS = 4096, SKX_CURVE_LDS_STEPS = 1024, SKX_CURVE_BATCH_ORDERS = 1024 };
int  skx_array_curve(skx_array *a, const int32_t *orders, uint32_t n_orders, double min_freq, uint64_t *counts);
/* MergeSkaArray::weed (merge_ska_array.rs:452-487): rows whose split k-mer is (reverse: is not) in `weed` are removed;
 * `weed` = the split k-mers of the weed FASTA (RefSka::new + kmer_iter, ska_ref.rs:189-262,541), i.e. the key set of its
 * dictionary: skx_dictset_build_files (1 sample) -> skx_keyset_union. */
int  skx_array_weed(skx_array *a, skx_keyset *weed, int reverse, uint64_t *removed);
/* RefSka::new + kmer_iter (ska_ref.rs:189-262,541) for `ska weed`: the split k-mers of a FASTA file as a key set;
 * SKX_EINVAL "Cannot create reference from FASTQ files" (ska_ref.rs:206-208), SKX_EEMPTY "<file> has no valid sequence" */
int  skx_keyset_from_fasta(skx_ctx *ctx, const char *path, int k, int rc, skx_keyset **out);
/* ---- `ska cov` ----
 * CoverageHistogram::new (coverage.rs:70-148) + the histogram step of fit_histogram (:158-163): occurrence counts of the
 * split k-mers of a FASTQ pair (qualities ignored): hist[c - 1] = #split k-mers seen c times, c <= 1000 (hist has 1000 entries).
 * SKX_EINVAL "<file> appears to be FASTA.\nCoverage can only be used with FASTQ files, not FASTA." */
int  skx_cov_histogram(skx_ctx *ctx, const char *fastq_fwd, const char *fastq_rev, int k, int rc, uint32_t *hist);

/* ---- `ska map` ----
 * generic_modes::map (generic_modes.rs:56-84) = RefSka::new(k, reference, rc, ambig_mask, repeat_mask) (ska_ref.rs:189-311)
 * + RefSka::map (:508-533) + write_aln (format 0, :622-645, AlnWriter aln_writer.rs) | write_vcf (format 1, :648-765).
 * The text is malloc'd (skx_free).  Errors where the reference panics: "Cannot create reference from FASTQ files",
 * "<file> has no valid sequence" (SKX_EEMPTY), "No split k-mers mapped to reference". */
int  skx_array_map(skx_array *a, const char *reference_fasta, int ambig_mask, int repeat_mask, int format, int threads, char **buf, uint64_t *len);
/* `ska screen`: which samples carry which sequences of a panel, and how well they match -- three integers per (record, sample) of a multi-FASTA
 * panel (resistance genes, virulence factors, replicons, typing loci) from one pass, without the S x panel-length cells `ska map` writes.  The
 * reference has no counterpart: its users count columns of `ska map`'s alignment, or run `ska weed --reverse` and `ska nk` once per record.
 * Definition (tests/screen_model.py states the same).  A panel is a FASTA file of R records.  A record's windows are exactly those `ska map`
 * gives a chromosome: runs of ACGT in either case, N splitting runs, and the end-of-record quirk (a run that starts less than k + 1 letters
 * before the end of its record gives none); each window has the position of its middle base, its canonical split k-mer and its is_rc.  Every
 * window counts on its own: a split k-mer that occurs twice counts twice, within a record or across records.  A window hits when its split
 * k-mer is a row of the array.  For a hit window and sample s the cell is the array's byte for (row, s), passed through RC_IUPAC when is_rc
 * (ska_ref.rs:519-530); the 0 byte an array may hold for '-' is '-'.  Per (record r, sample s), over r's hit windows:
 *     found   the cells that are not '-'
 *     match   the cells equal to the record's own middle base, upper-cased
 *     ambig   the cells that are present and none of A, C, G, T
 *     snp     found - match - ambig                                       (derived, not stored)
 * Per record: length = its bytes of sequence, windows = its windows, rows_hit = its hit windows.  A pair (r, s) passes, for a cover C and an
 * identity I in [0, 1], when windows > 0 and found >= max(1, ceil(C * windows)) and match >= ceil(I * found), the products in doubles
 * (skh_screen: --min-cover, --min-identity).
 * records[r] = {length, windows, rows_hit}; ids = the R record ids (the header up to white space), each NUL-terminated, one after the other;
 * cells[r * S + s] = {found, match, ambig}.  All three are malloc'd (skx_free); on an error none is.  `a` keeps its content (an array held as
 * pieces or lazily is materialised first); both key widths, engine-ordered or not.  SKX_EINVAL "split k-mers and variants are out of step ..."
 * as skx_array_map; "Cannot create reference from FASTQ files" for a FASTQ panel; SKX_EEMPTY "<file> has no valid sequence" for a panel
 * without a window; SKX_EINVAL naming the id for a record id that occurs twice, and for a cell outside the alphabet; SKX_EUNSUP above 2^31
 * (record, sample) pairs.  A panel none of whose windows hit (or an array without rows) is no error: every count is 0.  The counts are sums of
 * integers: the same bytes whatever the order of arrival.
 * One workgroup walks SKX_SCREEN_TILE consecutive hit windows for SKX_SCREEN_SAMPLES samples, a lane a sample.  Device memory beside the array:
 * `ska map`'s window buffers (25 bytes a panel byte, 33 at k > 31), 9 bytes a hit window, 12 bytes a (record, sample) pair. */
enum { SKX_SCREEN_TILE = 1024, SKX_SCREEN_SAMPLES = 256 };
typedef struct { uint64_t length, windows, rows_hit; } skx_screen_record;
typedef struct { uint32_t found, match, ambig; } skx_screen_cell;
int  skx_array_screen(skx_array *a, const char *panel_fasta, uint64_t *n_records, skx_screen_record **records, char **ids, skx_screen_cell **cells);
/* `ska qc`: which samples should not be in this file -- six counts per sample that each depend on a statistic of the row a cell sits in, from
 * two passes over the matrix.  The reference has no counterpart: `ska nk` (lib.rs:808-827) prints one k-mer count per sample, and its users run
 * `ska delete` and `ska nk` once per sample and compare.
 * Definition (tests/qc_model.py states the same).  The array holds S samples and U rows in its current order.  code(cell) is the 4-bit IUPAC
 * set of skx_array_group_markers (A 1, C 2, T 4, G 8; '-' and the 0 byte are 0).  A cell is present when its code != 0 and unambiguous when
 * popcount(code) == 1.  Per row r:
 *     n       = its present cells
 *     c[b]    = its cells that are exactly the unambiguous base b (b in A, C, T, G)
 *     unamb   = c[A] + c[C] + c[T] + c[G]
 *     major   = the base with the largest c[b], ties going to the lowest code (A < C < T < G); undefined when unamb == 0
 *     core    when n >= thr, thr = max(1, (uint64)ceil(S * min_freq)) computed in doubles exactly so (skx_array_curve's rule at t = S)
 *     variant when at least two bases have c[b] > 0
 * Per sample s six counts over the rows; a cell of s counts into
 *     kmers            when it is present                                   (equals skx_array_sample_kmers)
 *     ambiguous        when it is present and popcount(code) >= 2
 *     singletons       when it is present and n == 1
 *     core_present     when it is present and the row is core
 *     private_alleles  when it is unambiguous with base b, c[b] == 1 and unamb >= 2   (another sample carries a different plain base there)
 *     minor_alleles    when it is unambiguous, the row is core and its base != major
 * For the whole array: rows = U, rows_present (n >= 1), core_rows, core_variant_rows (core and variant), threshold = thr; the last three counts
 * equal skx_array_curve's pan, core and core_variant at t = S for any order.
 * samples: the caller's S records; info may be NULL.  `a` keeps its content (an array held as pieces or lazily is materialised first); both key
 * widths are taken, and so is an array without split k-mers: nothing here needs keys.  SKX_EINVAL with a message that begins "qc:" for NULL
 * arguments, NaN or min_freq outside [0, 1], a cell outside the alphabet; SKX_EUNSUP with the same beginning above 65 535 samples (the per-row
 * counters are 16 bits), for 2^32 rows or more, and for an array that holds only a part of its samples (skx_array_set_total_samples: a rank's
 * share of a collection spread over several devices).  U == 0: SKX_OK, zeros, threshold still set.  All results are sums of integers: the same bytes whatever the order of
 * arrival.
 * Two launches.  The first reads the matrix once, a lane 16 rows, and leaves a 16-bit descriptor per row (present, singleton, core, variant, the
 * bases with c == 1 where unamb >= 2, the major base one-hot); the second runs over (SKX_QC_TILE_ROWS rows, SKX_QC_SAMPLES samples) units,
 * classifies each cell against its row's descriptor and adds each unit's sums to the samples' counters.  Device memory beside the array:
 * 2 bytes a row (rounded up to SKX_QC_TILE_ROWS), 48 bytes a sample, 28 bytes of totals. */
enum { SKX_QC_TILE_ROWS = 4096, SKX_QC_SAMPLES = 64 };   /* the shape of the second kernel as built */
typedef struct { uint64_t kmers, ambiguous, singletons, core_present, private_alleles, minor_alleles; } skx_qc_sample;
typedef struct { uint64_t rows, rows_present, core_rows, core_variant_rows, threshold; } skx_qc_info;
int  skx_array_sample_qc(skx_array *a, double min_freq, skx_qc_sample *samples, skx_qc_info *info);
/* `ska density`: the stretches of a reference in which one sample carries far more SNPs than descent alone explains (recombination, to be taken
 * out before a tree is built), from one streamed pass over the matrix instead of the S x L alignment `ska map` writes.  The reference has no
 * counterpart: its users write that alignment and run a separate tool over it.
 * Definition (tests/density_model.py states the same).
 * Reference and windows.  The reference is a FASTA file of C chromosomes.  Its windows are `ska map`'s: runs of ACGT in either case, N splitting
 *     runs, and the end-of-record quirk (a run that starts less than k + 1 letters before the end of its record gives none); each window has the
 *     position of its middle base, its canonical split k-mer and its is_rc.
 * Sites.  A window is a site when its split k-mer is a row of the array and that split k-mer occurs exactly once among all windows of the
 *     reference.  The repeated windows are the ones `ska map --repeat-mask` masks; they are never sites, so every row is the row of at most one site.
 * Cells.  For site x and sample s the cell is the array's byte for (row, s), passed through RC_IUPAC when is_rc; the 0 byte counts as '-'.
 * Classes.  With r = the reference's middle base, upper-cased, a cell is missing when it is '-'; ambiguous when it is present and none of A, C,
 *     G, T; snp when it is one of A, C, G, T and != r; otherwise it matches.  callable = matching + snp, so missing + ambiguous + callable = sites
 *     for every sample.
 * Dense SNPs.  Per (sample, chromosome) take the SNP positions p_0 < p_1 < ...; SNP i is dense when some j with j <= i <= j + T - 1 has
 *     p_{j+T-1} - p_j < W: i is one of T consecutive SNPs that lie inside W consecutive reference positions.
 * Regions.  A region is a maximal run of consecutive dense SNPs of one (sample, chromosome): sample, chromosome, start = first position, end =
 *     last position (0-based here), snps = their number.  Regions never span chromosomes.
 * Bins.  Chromosome c has ceil(len_c / W) bins of W positions; per bin, summed over samples, snps and dense_snps.
 * Per sample.  sites, callable, ambiguous, missing, snps, dense_snps, regions and region_bases (the sum of end - start + 1).
 * Whole call.  windows, repeat_windows (windows whose split k-mer occurs more than once) and sites.
 * Everything is an integer: the same bytes whatever the order of arrival.  1 <= W <= 2^31, 2 <= T <= 65 535.
 * Results (each malloc'd, skx_free; on an error none is returned and *out is zeroed): samples[S]; regions[info.n_regions] ascending by (sample,
 * chromosome, start); bins[info.n_bins], chromosome after chromosome; chrom_ids = the C ids (the header up to white space), each NUL-terminated,
 * one after the other; chrom_lens[C]; with SKX_DENSITY_WANT_SNPS snps[info.n_snps], ascending by (sample, x), = sample << 34 | x << 2 | base, x the position in
 * the concatenated reference, base the cell as read on the reference's strand (A 0, C 1, T 2, G 3), bit SKX_DENSITY_DENSE_BIT set when the SNP
 * is dense, and snp_ref[info.n_snps] = the reference's byte there, upper-cased.
 * `a` keeps its content (an array held as pieces or lazily is materialised first); both key widths, engine-ordered or not.  SKX_EINVAL with a
 * message that begins "density:" for NULL arguments, W or T out of range, a cell of a site outside the alphabet, a chromosome id that occurs twice;
 * "Cannot create reference from FASTQ files", SKX_EEMPTY "<file> has no valid sequence" and "split k-mers and variants are out of step ..." as
 * skx_array_map; SKX_EUNSUP with "density:" for an array that holds only a part of its samples, 2^28 samples or more, 2^32 - 2 SNP records or
 * more.  No site, or an array without rows, is no error: the counts are zeros.
 * Device side.  density_rows_kernel leaves per row the byte a matching cell holds (0: no site) and the site's position.  density_kernel runs over
 * units of (SKX_DENSITY_TILE_ROWS rows, SKX_DENSITY_SAMPLES samples), a lane 16 rows, twice: a count launch (four counts per sample, the unit's
 * SNPs) and, after a scan of the units, a write launch (one 64-bit record per SNP).  The records are sorted; the dense flags, regions, bins and
 * per-sample sums come from passes over the sorted list in blocks of SKX_DENSITY_SCAN_BLOCK.  Device memory beside the array: `ska map`'s window
 * buffers (25 bytes a reference byte at k <= 31, 33 above) and the repeat sort's (28 bytes a window), 5 bytes a row (rounded up to
 * SKX_DENSITY_TILE_ROWS), 8 bytes a unit, 64 bytes a sample, 8 bytes a bin, and per SNP record 16 bytes and the radix sort's own buffers while
 * the list is sorted, 27 bytes after it, 20 bytes a region. */
enum { SKX_DENSITY_TILE_ROWS = 4096, SKX_DENSITY_SAMPLES = 64, SKX_DENSITY_SCAN_BLOCK = 4096 };   /* the shapes of the kernels as built */
enum { SKX_DENSITY_WANT_SNPS = 1, SKX_DENSITY_DENSE_BIT = 62 };
typedef struct { uint32_t sample, chrom, start, end, snps; } skx_density_region;
typedef struct { uint64_t sites, callable, ambiguous, missing, snps, dense_snps, regions, region_bases; } skx_density_sample;
typedef struct { uint32_t snps, dense_snps; } skx_density_bin;
typedef struct { uint64_t windows, repeat_windows, sites, n_chrom, n_bins, n_snps, n_regions; } skx_density_info;
typedef struct {
    skx_density_info info;
    skx_density_sample *samples; skx_density_region *regions; skx_density_bin *bins;
    char *chrom_ids; uint64_t *chrom_lens;
    uint64_t *snps; uint8_t *snp_ref;
} skx_density_result;
int  skx_array_snp_density(skx_array *a, const char *reference_fasta, uint64_t window, uint32_t min_snps, int flags, skx_density_result *out);
/* `ska mask`: regions of a reference taken out of an array, per sample or for every sample, in place -- what makes the regions of `ska density`
 * (or a BED of phage, mobile-element or repeat coordinates) usable by every command that reads a .skf.  The reference has no counterpart: its
 * `ska weed` removes split k-mers by sequence, never by position and never per sample.
 * Definition (tests/mask_model.py states the same).
 * Sites.  Reference, windows and sites are `ska density`'s (above): `ska map`'s windows; a window is a site when its split k-mer is a row and
 *     occurs exactly once among the reference's windows.  Repeated windows are never sites, so a row is the row of at most one site.  is_rc plays
 *     no part: a cell is only ever made missing.
 * Intervals.  (sample or SKX_MASK_ALL_SAMPLES, chrom = the index of the FASTA record, start, end), 0-based and inclusive, in positions of a
 *     window's middle base.  Per (sample, chromosome), and per chromosome for ALL, intervals that overlap or touch (start <= the other's end + 1)
 *     are merged first: the result does not depend on how the caller cut them.  n_intervals_merged counts the merged ones.
 * Step 1.  Every row whose site lies in an ALL interval is removed (rows_all_samples).
 * Step 2.  For each remaining row whose site lies in an interval of sample s (sites_in_regions[s] counts it, present or not): if the cell
 *     (row, s) is present -- neither '-' nor the 0 byte -- it becomes '-', the row's stored count drops by one (never below 0) and
 *     cells_masked[s] counts it.
 * Step 3.  A row that lost a cell in step 2 and has no present cell left is removed (rows_emptied): delete_samples' update_counts(false) rule,
 *     applied to the rows the call touched.  Keys, variants and counts are compacted in the array's row order; names, k, rc and the sample count
 *     stay.  A row that is no site, or whose site lies in no interval, keeps every cell and its count -- also one that held no present cell before.
 * Whole call.  sites, rows_in, rows_all_samples, rows_emptied, rows_out = rows_in - rows_all_samples - rows_emptied.  Everything is an integer:
 *     the same bytes whatever the order of arrival.  Masking a second time with the same intervals changes nothing.
 * samples: S records of the caller's, or NULL.  The call works in place, as skx_array_weed does; an array held as pieces or lazily is
 * materialised first; both key widths, engine-ordered or not.  Every refusal comes before the first cell is changed: `a` keeps its content.
 * SKX_EINVAL with a message that begins "mask:" for NULL arguments, an interval with start > end, an end past its chromosome, a sample or
 * chromosome index out of range, a chromosome id that occurs twice; "Cannot create reference from FASTQ files", SKX_EEMPTY "<file> has no valid
 * sequence" and "split k-mers and variants are out of step ..." as skx_array_map; SKX_EUNSUP with "mask:" for an array that holds only a part
 * of its samples.  n == 0, no site, no rows, or every row removed (an array of 0 rows comes back and can be saved) is no error.
 * Device side (csrc/skx_mask.hip).  The sites are compacted in reference order to (position in the concatenated reference, row); every merged
 * interval finds its stretch of that list by binary search; the host scans the lengths in 64 bits; mask_items_kernel takes SKX_MASK_CHUNK
 * consecutive (interval, site) items a workgroup -- the ALL intervals first (keep[row] = 0, no cell read), then the per-sample ones (cell, count
 * by a 32-bit atomic, the sample's two sums per wave).  Intervals are merged per sample and a row has one site, so no cell is visited twice.
 * When a cell was masked the rows' statistics are counted again from the cells (one read of the matrix); rows go through skx_array_weed's
 * compaction.  Device memory beside the array: `ska map`'s window buffers and the repeat sort's, 9 bytes a hit window, 8 bytes a site, 24 bytes
 * a merged interval, 16 bytes a sample, a byte a row, and the compaction's second matrix when a row goes. */
enum { SKX_MASK_CHUNK = 1024 };                  /* items a workgroup of mask_items_kernel takes, as built */
#define SKX_MASK_ALL_SAMPLES 0xFFFFFFFFu
typedef struct { uint32_t sample; uint32_t chrom; uint32_t start, end; } skx_mask_interval;
typedef struct { uint64_t sites_in_regions, cells_masked; } skx_mask_sample;
typedef struct { uint64_t sites, rows_in, rows_all_samples, rows_emptied, rows_out, n_intervals_merged; } skx_mask_info;
int  skx_array_mask_regions(skx_array *a, const char *reference_fasta, const skx_mask_interval *iv, uint64_t n,
                            skx_mask_sample *samples, skx_mask_info *info);
/* the records of a FASTA reference as skx_array_map, skx_array_snp_density and skx_array_mask_regions number them (host only): *ids = the *n ids
 * (the header up to white space), each NUL-terminated, one after the other; *lens = their lengths in bases.  Both malloc'd (skx_free).  "Cannot
 * create reference from FASTQ files" and a reference longer than 4 G bases are refused as there. */
int  skx_reference_records(const char *reference_fasta, char **ids, uint64_t **lens, uint64_t *n);
/* the `k` a .skf file states in its first fields, without loading it (0: not found there, or the file cannot be read): lets a caller that
 * would try 64-bit keys first and 128-bit keys next (lib.rs:635-661) go to the right width at once */
int  skx_skf_peek_k(const char *path);
/* the context an array lives on; and a way for host glue above the ABI to leave its message in skx_last_error() */
skx_ctx *skx_array_ctx(const skx_array *a);
void skx_set_last_error(const char *msg);

/* ---- `ska lo` (generic_modes.rs:286-306, src/skalo) ----
 * read_graph.rs:build_graph + extremities.rs:identify_good_kmers on the device: the coloured de Bruijn graph of the array (every sample on
 * this device; at most 65 535 samples, the reference's u16 sample index), in CSR form with (k-1)-mer nodes in the reference's 2-bit code
 * (A=0, C=1, T=2, G=3, first base high; words_per_node 64-bit words each, little-endian: 1 for k <= 31, 2 above).  Nodes ascending,
 * each node's neighbours ascending with repeated edges kept, entry nodes ascending, exit nodes (their reverse complements) ascending.
 * The colours (sample bitsets, colour_words 64-bit words, bit s = sample s) of the full k-mers stay on the device: skx_lo_gather looks
 * up a batch of them (found[i] = 0: not a k-mer of the graph).  A k-mer two (row, base) pairs write keeps the colour of the lowest
 * (split k-mer, base code). */
typedef struct skx_lo_graph skx_lo_graph;
typedef struct {
    int32_t  k, words_per_node;
    uint64_t n_samples, colour_words;
    uint64_t n_nodes, n_edges, n_entries;   /* n_exits == n_entries */
    uint64_t n_colours;                     /* present (row, base) pairs */
    uint64_t n_kmers;                       /* distinct full k-mers */
} skx_lo_info;
int  skx_array_lo_graph(skx_array *a, skx_lo_graph **out);
int  skx_lo_graph_info(const skx_lo_graph *g, skx_lo_info *info);
/* copy-out; any pointer may be NULL: nodes[n_nodes * wpn], offsets[n_nodes + 1], neighbours[n_edges * wpn], entries / exits[n_entries * wpn] */
int  skx_lo_graph_export(const skx_lo_graph *g, uint64_t *nodes, uint64_t *offsets, uint64_t *neighbours, uint64_t *entries, uint64_t *exits);
/* kmers[n * wpn] full k-mers -> colours[n * colour_words], found[n] */
int  skx_lo_gather(skx_lo_graph *g, const uint64_t *kmers, uint64_t n, uint64_t *colours, uint8_t *found);
void skx_lo_graph_free(skx_lo_graph *g);

/* ---- `ska distance --tree` (the reference has no call site: replaces scripts/cluster_dists.py --rapidnj) ----
 * Neighbour joining (Saitou-Nei, Studier-Keppler Q) in float64 on the device.  Leaves are the nodes 0 .. n-1 in sample order, join t
 * (0-based) makes node n + t.  With n nodes active and r[x] the sum of D[x][y] over them, a step joins the active pair that minimises
 * Q(x, y) = (n-2) D[x][y] - r[x] - r[y], ties to the lowest (min id, max id); a < b by id, len_a = D[a][b]/2 + (r[a] - r[b]) / (2(n-2)),
 * len_b = D[a][b] - len_a (raw: they may be negative on non-additive data); the new node is (D[a][k] + D[b][k] - D[a][b]) / 2 from k.
 * The last record joins the two nodes left with len_a = D[a][b], len_b = 0; n = 2 has that record only.  The same input gives the same
 * records bit for bit.  SKX_EINVAL with a message for n < 2, SKX_ENOMEM with one when the 8 n^2 byte matrix does not fit the device. */
typedef struct { uint32_t a, b; double len_a, len_b; } skx_nj_join;
/* joins: n_samples - 1 records.  d: upper triangle, pairs (i<j) row-major, as skx_array_distance writes it (its `distance` field is used) */
int  skx_dist_nj(skx_ctx *ctx, const skx_dist *d, int n_samples, skx_nj_join *joins);
/* the same on a full row-major n x n host matrix of doubles (symmetric, zero diagonal, finite; refused otherwise) */
int  skx_matrix_nj(skx_ctx *ctx, const double *m, int n, skx_nj_join *joins);

/* ---- `ska distance --no-table`: the tree and the clusters without the table.  The pair matrix is swept band by band as for
 * skx_array_distance_select, and two consumers keep their result on the device: a union-find over the pairs that pass the cluster thresholds
 * (a link points the higher root at the lower, so a cluster's root is its lowest sample whatever the order of the bands), and the float64
 * matrix of the distances, which neighbour joining then runs on as it runs for skx_dist_nj.  Device memory: the band's count buffer, 8 n^2
 * bytes for the joins, O(n) besides; host memory O(n).  The thresholds are those of skh_distance_clusters, i.e. on the values as the table
 * prints them (skh_cluster_cutoffs). */
typedef struct {
    double  cluster_snps, cluster_mismatches;   /* as skh_distance_clusters takes them; used when labels != NULL */
    int32_t band_rows;                          /* 0: the engine's choice, as skx_select_spec.band_rows */
} skx_banded_spec;
/* what a call did: bands swept, first samples per band, bytes of the device count buffer, pairs within the thresholds, clusters */
typedef struct { uint64_t bands, band_rows, count_buffer_bytes, edges, clusters; } skx_banded_info;
/* labels (n_samples, or NULL): labels[i] = the lowest sample of i's cluster, the partition skh_distance_clusters makes of the full table.
 * joins (n_samples - 1, or NULL): the records skx_dist_nj gives on the full table's distances, bit for bit; n_samples as skx_dist_nj takes it
 * (2 .. 65 535).  constant / rows_used as skx_array_distance_filtered reports them; info may be NULL.  SKX_EINVAL with a message that begins
 * "distance banded:" when both outputs are NULL, a threshold is NaN or negative (with labels) or band_rows < 0.  Fewer than two samples and
 * labels only: every sample its own cluster.  The array is left as it is; both key widths and arrays held as pieces are taken. */
int  skx_array_distance_banded(skx_array *a, double min_freq, int filt_ambig, const skx_banded_spec *spec,
                               uint32_t *labels, skx_nj_join *joins, int64_t *constant, uint64_t *rows_used, skx_banded_info *info);
/* The same on an array the two filters have been applied to already, as skx_array_distance_select_prefiltered is to skx_array_distance_select */
int  skx_array_distance_banded_prefiltered(skx_array *a, int64_t constant, int filt_ambig, const skx_banded_spec *spec,
                                           uint32_t *labels, skx_nj_join *joins, skx_banded_info *info);

/* wall-clock phases of the host-side path (file reading + upload, .skf codec, FASTA writer ...), accumulated per name since the
 * last reset: a JSON object {"phase": seconds, ...} in first-use order (malloc'd, skx_free).  The reference has no counterpart;
 * bench.py's end_to_end leg and SKX_DEBUG read them.  skx_phase_add lets host glue above the ABI record its own phases. */
int  skx_phases_json(char **buf, uint64_t *len, int reset);
void skx_phase_add(const char *name, double seconds);

/* per-stage device timings of the last call on this ctx (ms; HIP events on the ctx stream).  The last four are single kernels of the
 * append pass, measured inside their stages (probe + append inside key_union, pieces_stats inside assemble, the kept rows' pieces_rows
 * inside compact): what bench.py's `roofline.dominant` is computed from. */
typedef struct { double hist, scatter, dedupe, key_union, assemble, filter, compact, distance, append_probe, append, pieces_stats, pieces_rows; } skx_timings;
int  skx_ctx_timings(skx_ctx *ctx, skx_timings *t, int reset);
/* which kernels the last merge on this context went through: "append64" / "append128" (MergeSkaDict::append in one pass over the
 * unsorted regions, merge_ska_dict.rs:77-109, for u64 / u128 keys) or "sorted: <why the pass was not taken>" (per-sample sort +
 * union + assemble); "" before the first merge.  The reference has no counterpart: its append is one code path. */
const char *skx_ctx_merge_path(skx_ctx *ctx);
/* what the statistics pass of the last skx_array_filter on this context left unread: a filter at min_count >= 2 over an array still
 * held as the merge's pieces counts only the first-seen ranks that enough samples reach (the rest cannot pass).  *ranks = ranks not
 * read, *blocks = row blocks that had such ranks; both 0 when the pass was the full one.  The reference has no counterpart. */
int  skx_ctx_filter_cut(skx_ctx *ctx, uint64_t *ranks, uint64_t *blocks);

#ifdef __cplusplus
}
#endif
#endif
