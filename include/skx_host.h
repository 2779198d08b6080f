/*
 * skx_host.h -- host-side mirror of the reference's mode glue for the hot path, above the skx.h C ABI.
 * Same names, argument meaning and error behaviour as the Rust functions they replace (the reference's
 * toolchain is absent from this image, so the host side is C++; a Rust host would call skx.h directly and
 * keep its own generic_modes.rs / io_utils.rs).  Text results are malloc'd; free with skx_free().
 */
#ifndef SKX_HOST_H
#define SKX_HOST_H
#include "skx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* generic_modes::apply_filters (generic_modes.rs:112-131): threshold = ceil(n_samples * min_freq), update_kmers = false */
int skh_apply_filters(skx_array *a, double min_freq, int filter_ambig_as_missing, int filter_type, int ambig_mask,
                      int ignore_const_gaps, int32_t *removed);
/* generic_modes::align (generic_modes.rs:22-50): filters then the FASTA alignment */
int skh_align(skx_array *a, int filter_type, int mask_ambig, int ignore_const_gaps, double min_freq,
              int filter_ambig_as_missing, char **buf, uint64_t *len);
int skh_align_fd(skx_array *a, int filter_type, int mask_ambig, int ignore_const_gaps, double min_freq,
                 int filter_ambig_as_missing, int fd);   /* the same, streamed to a file descriptor */
/* `ska align <inputs>` (lib.rs:617-662 = io_utils::load_array + generic_modes::align): one .skf input goes through the engine's
 * one-pass load + filter (skx_array_load_filtered), several sequence files through build_and_merge with the CLI defaults */
int skh_align_inputs_fd(skx_ctx *ctx, const char *const *inputs, int n_inputs, int threads, int filter_type, int mask_ambig, int ignore_const_gaps,
                        double min_freq, int filter_ambig_as_missing, int fd);
/* `ska align <inputs> --groups FILE -o PREFIX [--min-group-size N]` (no counterpart in the reference, whose users run `ska delete` of everybody
 * else, generic_modes.rs:192-210, and `ska align`, :22-50, once per group): the inputs are loaded once (skh_load_array: one .skf, or sequence
 * files built with the CLI defaults); every group of at least min_group_size (>= 1) samples goes through skx_array_subset_filtered and
 * skx_array_write_fasta into <PREFIX>.<label>.aln -- the bytes `ska delete` + `ska align` with the same options write.  Names are matched to
 * samples as skx_array_delete_samples matches them (first match wins; "Could not find sample(s): {..}"); samples the file does not list
 * belong to no group.  <PREFIX>.groups.tsv: header "Group\tSamples\tSplit k-mers\tRemoved\tSites\tFile", a line per group in file order
 * (Split k-mers = rows left by the delete, what `ska nk` prints), "-" in the last three columns of a group that was too small.
 * Phases: align.groups_load / groups_verdicts / groups_rows / groups_write. */
int skh_align_groups(skx_ctx *ctx, const char *const *inputs, int n_inputs, int threads, int filter_type, int mask_ambig, int ignore_const_gaps,
                     double min_freq, int filter_ambig_as_missing, const char *groups_file, int min_group_size, const char *out_prefix);
/* `ska align <inputs> --samples NAMES | --samples-file FILE`: the one subset `names` (repeats collapse), its alignment streamed to fd */
int skh_align_samples_fd(skx_ctx *ctx, const char *const *inputs, int n_inputs, int threads, int filter_type, int mask_ambig, int ignore_const_gaps,
                         double min_freq, int filter_ambig_as_missing, const char *const *names, int n_names, int fd);
/* the groups file of skh_align_groups (host only, no device): two columns, sample name and group label, separated by a tab (when the line
 * holds one outside quotes) or else by a comma; <prefix>.clusters.csv as skh_clusters_csv writes it is taken as it is -- its header line
 * "id,Cluster__autocolour" is skipped when it comes first, names in double quotes with inner quotes doubled may hold , " and line breaks.
 * Blank lines and a trailing carriage return are ignored.  *buf (malloc'd) = the pairs as "name\0label\0", group by group in the order
 * the labels first appear and in file order within a group; *n_pairs (may be NULL) = how many.  SKX_EINVAL with "groups file <path>: line
 * <n>: ..." for a line without exactly two fields, an empty name or label, a label holding '/' or a NUL or equal to "." or "..", a sample
 * name listed twice; SKX_EIO when the file cannot be read. */
int skh_read_groups(const char *path, char **buf, uint64_t *len, uint64_t *n_pairs);
/* `ska markers <SKF_FILE> --groups FILE -o PREFIX [--min-in P] [--max-out Q] [--min-group-size N] [--kind ...] [--fasta]` (no counterpart in the
 * reference, whose users run `ska delete` of a group, generic_modes.rs:192-210, and `ska nk --full-info`, lib.rs:808-827, once per group and
 * compare the text): the file is loaded once (skh_load_array), the groups file is read by skh_read_groups and its names matched as
 * skh_align_groups matches them; groups of fewer than min_group_size (>= 1) samples are not reported, their samples still count as others;
 * one call of skx_array_group_markers (its definition of a marker; kinds as it takes them) answers every group.
 * <PREFIX>.markers.tsv: header "Group\tUpper\tLower\tKind\tIn\tOut\tBases\tOther bases", one line per record, groups in file order, within a
 * group in the order `ska nk --full-info` prints the rows of the same file, Upper and Lower decoded as there; Kind = presence | allele,
 * In = in/n, Out = out/(S-n), Bases / Other bases = the IUPAC letter of the set ("-" for the empty one).
 * <PREFIX>.markers.summary.tsv: header "Group\tSamples\tPresence\tAllele", one line per group, "-" in the two counts of a group that was too small.
 * fasta != 0: <PREFIX>.<label>.markers.fa for every reported group with a marker, one record per marker in the TSV's order:
 * ">{label}_{i} kind=.. in=.. out=.. bases=.." (i from 1), sequence = Upper + the first of A, C, G, T in the group's set + Lower + one N --
 * `ska weed <skf> <that file> --reverse --min-freq 0` keeps exactly the marker rows (k bases alone give the reference's reader no split k-mer; the N adds none).
 * Phases: markers.load / markers.pass / markers.text. */
int skh_markers(skx_ctx *ctx, const char *skf_file, const char *groups_file, const char *out_prefix, double min_in, double max_out,
                int min_group_size, int kinds, int fasta);
/* the seeded orders of `ska curve`, from one stream: splitmix64 (state = seed; next: state += 0x9E3779B97F4A7C15, z = state,
 * z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB, z ^ z >> 31), order 0 drawn first; each order starts as
 * 0..S-1 and is shuffled by Fisher-Yates from i = S-1 down to 1, swapping o[i] and o[j] with j from [0, i] by rejection: draws x >= 2^64 -
 * 2^64 mod (i + 1) are thrown away, j = x mod (i + 1).  orders: the caller's n_orders x S.  Host only (tests/curve_model.py states the same). */
int skh_curve_orders(uint64_t seed, uint32_t n_samples, uint32_t n_orders, int32_t *orders);
/* <PREFIX>.curve.tsv from the counts of skx_array_curve (host only): header "t\tpan_min\tpan_median\tpan_max\tpan_mean\tcore_min\t...
 * \tcore_variant_mean", then one line per t = 1..S with, for each of pan, core, variant and core_variant, the minimum, the lower median (place
 * (P - 1) / 2 of the sorted values), the maximum and the mean over the P orders.  The mean has three decimals and is rounded half up in integers,
 * (sum * 1000 + P / 2) / P: no floating point reaches the text.  *buf is malloc'd (skx_free). */
int skh_curve_tsv(const uint64_t *counts, uint32_t n_orders, uint32_t n_samples, char **buf, uint64_t *len);
/* `ska curve <SKF_FILE> -o PREFIX [--permutations P] [--seed N] [--min-freq F] [--order-file FILE] [--all-permutations]` (no counterpart in the
 * reference): the file is loaded once (skh_load_array) and one call of skx_array_curve answers every order -- n_permutations (1..10 000) orders
 * of skh_curve_orders for `seed`, or, with order_file != NULL, the one order of that file: sample names, one a line (blank lines and a trailing
 * carriage return ignored), every sample of the array exactly once; a name that is unknown, given twice or missing is SKX_EINVAL with the name in
 * the message.  <PREFIX>.curve.tsv as skh_curve_tsv writes it; with all_permutations or an order file also <PREFIX>.curve.permutations.tsv:
 * header "permutation\tt\tsample\tpan\tcore\tvariant\tcore_variant\tnew", one line per order (from 0) and t, sample = the one added at t,
 * new = pan(t) - pan(t - 1) with pan(0) = 0.  Phases: curve.load / curve.orders / curve.kernel / curve.text. */
int skh_curve(skx_ctx *ctx, const char *skf_file, const char *out_prefix, uint32_t n_permutations, uint64_t seed, double min_freq,
              const char *order_file, int all_permutations);
/* the three texts of `ska screen` from what skx_array_screen returns (host only; definition of the counts and of "passes" in include/skx.h,
 * restated in tests/screen_model.py).  names: the array's n_samples sample names.
 * SKH_SCREEN_PAIRS   <PREFIX>.screen.tsv: header "record\tlength\twindows\tsample\tfound\tmatch\tambig\tsnp\tcover\tidentity", then one line
 *                    per passing (record, sample), in panel order and then array order; snp = found - match - ambig, cover = found / windows
 *                    and identity = match / found, each the double quotient printed as %.4f.
 * SKH_SCREEN_SUMMARY <PREFIX>.screen.summary.tsv: header "record\tlength\twindows\trows_hit\tsamples_passing", one line per record, those
 *                    without a window included.
 * SKH_SCREEN_MATRIX  <PREFIX>.screen.matrix.tsv: header "record" and the sample names, one line per record: its id, then 1 where the pair
 *                    passes and 0 where it does not.
 * SKX_EINVAL for NULL arguments, another `which`, NaN or a cover or identity outside [0, 1].  *buf is malloc'd (skx_free). */
enum { SKH_SCREEN_PAIRS = 0, SKH_SCREEN_SUMMARY = 1, SKH_SCREEN_MATRIX = 2 };
int skh_screen_text(int which, uint64_t n_records, const skx_screen_record *records, const char *ids, const skx_screen_cell *cells,
                    const char *const *names, uint64_t n_samples, double min_cover, double min_identity, char **buf, uint64_t *len);
/* `ska screen <SKF_FILE> <PANEL> -o PREFIX [--min-cover C] [--min-identity I] [--matrix]` (no counterpart in the reference): the file is loaded
 * once (skh_load_array), one call of skx_array_screen counts every (record, sample) pair, and <PREFIX>.screen.tsv, <PREFIX>.screen.summary.tsv
 * and, with matrix != 0, <PREFIX>.screen.matrix.tsv are written as skh_screen_text forms them.  The refusals are skx_array_screen's.
 * Phases: screen.load / screen.counts (inside it screen.read_panel, screen.windows, screen.lookup, screen.kernel) / screen.text. */
int skh_screen(skx_ctx *ctx, const char *skf_file, const char *panel_fasta, const char *out_prefix, double min_cover, double min_identity, int matrix);
/* the three texts of `ska qc` from what skx_array_sample_qc returns (host only; the counts are defined in include/skx.h, the rule and the texts
 * restated in tests/qc_model.py).  names: the array's n_samples sample names; mad: the M of the rule.
 * Six metrics per sample: kmers, ambiguous, singletons, core_missing = core_rows - core_present (0 where a made-up core_present is the larger),
 * private_alleles, minor_alleles.  The flag rule, in integers and one double product: for a metric with values x[0..S), med = place (S - 1) / 2
 * of the sorted values, mad = the same place of the sorted |x - med|, d = max(mad, 1); a sample is high when x > med and (double)(x - med) >
 * M * (double)d, and low symmetrically.  kmers is flagged on both sides (low_kmers, high_kmers), the other five on the high side under their
 * own names.  S = 1 has no flags (x = med); at S = 2 med is the smaller value and mad 0, so the larger one is high once it is more than M above.
 * SKH_QC_SAMPLES  <PREFIX>.qc.tsv: header "sample\tkmers\tambiguous\tsingletons\tcore_present\tcore_missing\tprivate_alleles\tminor_alleles\t
 *                 flags", then a line per sample in the array's order; flags in the order low_kmers, high_kmers, ambiguous, singletons,
 *                 core_missing, private_alleles, minor_alleles, comma separated, or "-".
 * SKH_QC_SUMMARY  <PREFIX>.qc.summary.tsv: the lines "samples", "rows", "rows_present", "core_rows", "core_variant_rows", "threshold", each
 *                 with its value behind a tab; the line "metric\tmin\tmedian\tmax\tmad\tflagged"; a line per metric in the order above
 *                 (flagged = the samples flagged through it; all zeros without samples).
 * SKH_QC_FLAGGED  <PREFIX>.qc.flagged.txt: the names with at least one flag, one per line, in the array's order: what `ska delete -f` reads.
 * SKX_EINVAL for NULL arguments, another `which`, a negative or NaN mad.  *buf is malloc'd (skx_free). */
enum { SKH_QC_SAMPLES = 0, SKH_QC_SUMMARY = 1, SKH_QC_FLAGGED = 2 };
int skh_qc_text(int which, const skx_qc_sample *samples, const char *const *names, uint64_t n_samples, const skx_qc_info *info, double mad,
                char **buf, uint64_t *len);
/* `ska qc <SKF_FILE> -o PREFIX [--min-freq F] [--mad M]` (no counterpart in the reference): the file is loaded once, unfiltered
 * (skh_load_array), one call of skx_array_sample_qc counts, and the three files are written as skh_qc_text forms them (the flagged list always,
 * empty when nobody is flagged).  SKX_EINVAL for NULL arguments, min_freq outside [0, 1] and a negative or NaN mad before anything is loaded;
 * otherwise the refusals are skx_array_sample_qc's.  Phases: qc.load / qc.kernels / qc.text. */
int skh_qc(skx_ctx *ctx, const char *skf_file, const char *out_prefix, double min_freq, double mad);
/* the four texts of `ska density` from what skx_array_snp_density returns (host only; the counts are defined in include/skx.h, the texts restated
 * in tests/density_model.py).  names: the array's n_samples sample names; window: the W of the call.  Positions are 1-based and inclusive.
 * SKH_DENSITY_REGIONS <PREFIX>.density.regions.tsv: header "sample\tchromosome\tstart\tend\tlength\tsnps", a line per region in the result's order.
 * SKH_DENSITY_SUMMARY <PREFIX>.density.summary.tsv: header "sample\tsites\tcallable\tambiguous\tmissing\tsnps\tdense_snps\tregions\tregion_bases\t
 *                     snps_outside", a line per sample in the array's order; snps_outside = snps - dense_snps.
 * SKH_DENSITY_BINS    <PREFIX>.density.bins.tsv: header "chromosome\tstart\tend\tsnps\tdense_snps", a line per bin, chromosome after chromosome;
 *                     the last bin of a chromosome ends at its length.
 * SKH_DENSITY_SNPS    <PREFIX>.density.snps.tsv: header "sample\tchromosome\tposition\tref\talt\tdense", a line per SNP in the list's order;
 *                     ref = the reference's base upper-cased, alt = the sample's base on the reference's strand, dense = 1 or 0.
 * SKX_EINVAL for NULL arguments, another `which`, window 0, a result that names a sample, chromosome or position that is not there, bins that are
 * not those of `window`, SKH_DENSITY_SNPS on a result without the list.  *buf is malloc'd (skx_free). */
enum { SKH_DENSITY_REGIONS = 0, SKH_DENSITY_SUMMARY = 1, SKH_DENSITY_BINS = 2, SKH_DENSITY_SNPS = 3 };
int skh_density_text(int which, const skx_density_result *r, const char *const *names, uint64_t n_samples, uint64_t window, char **buf, uint64_t *len);
/* what --masked-aln does to `ska map`'s alignment of the same array and reference (format aln: per sample '>' name '\n', the concatenated
 * chromosomes, '\n'), in place: in each sample's line every byte of a region [start, end] that is not '-' becomes 'N'.  SKX_EINVAL when the
 * text's length is not that of these samples on this reference, or a region lies outside it. */
int skh_density_mask_alignment(char *aln, uint64_t len, const skx_density_result *r, const char *const *names, uint64_t n_samples);
/* `ska density <REFERENCE> <SKF_FILE> -o PREFIX [--window W] [--min-snps T] [--snps] [--masked-aln FILE]` (no counterpart in the reference): the
 * file is loaded once, unfiltered (skh_load_array), one call of skx_array_snp_density counts, and <PREFIX>.density.regions.tsv, .summary.tsv,
 * .bins.tsv and, with snps != 0, .snps.tsv are written as skh_density_text forms them.  masked_aln != NULL: skx_array_map's alignment of the same
 * reference (format aln, no ambig mask, repeat mask on) through skh_density_mask_alignment into that file: what a tree builder takes.
 * SKX_EINVAL for NULL arguments and W or T out of range before anything is loaded; otherwise the refusals are skx_array_snp_density's (and
 * skx_array_map's).  Phases: density.load / density.kernels (inside it density.read_reference, .windows, .lookup, .rows, .count, .write, .sort,
 * .dense) / density.text / density.masked_aln. */
int skh_density(skx_ctx *ctx, const char *reference_fasta, const char *skf_file, const char *out_prefix, uint64_t window, uint32_t min_snps, int snps,
                const char *masked_aln);
/* ---- `ska mask` (no counterpart in the reference; the counts are defined in include/skx.h, the files and the text restated in
 * tests/mask_model.py).  The two readers take a file's text (host only) and hand over malloc'd intervals (skx_free; *n may be 0) in the file's
 * order, 0-based and inclusive as skx_array_mask_regions takes them.  Both accept CRLF, blank lines and lines that start with '#', and refuse
 * with SKX_EINVAL and a message "mask: regions line N: ..." / "mask: bed line N: ..." (N from 1): a line with too few fields, a sample or
 * chromosome that is not among names / chrom_ids (the first of two equal names wins), a start or an end that is not an unsigned decimal number
 * of 32 bits, an end past its chromosome, and
 * skh_mask_read_regions  `ska density`'s OUT.density.regions.tsv or any tab-separated file of its shape: the first line that is neither blank
 *                        nor a comment is the header and is skipped; then sample, chromosome, start, end, 1-based and inclusive; further
 *                        columns are ignored.  Refused too: start < 1, end < start.
 * skh_mask_read_bed      chromosome, start (0-based), end (exclusive), no header; every interval is an ALL interval.  Refused too: end <= start. */
int skh_mask_read_regions(const char *text, uint64_t len, const char *const *names, uint64_t n_samples, const char *const *chrom_ids, const uint64_t *chrom_lens,
                          uint64_t n_chrom, skx_mask_interval **out, uint64_t *n);
int skh_mask_read_bed(const char *text, uint64_t len, const char *const *chrom_ids, const uint64_t *chrom_lens, uint64_t n_chrom, skx_mask_interval **out, uint64_t *n);
/* <PREFIX>.mask.summary.tsv from what skx_array_mask_regions returned for the intervals iv[n] (host only): header "sample\tintervals\t
 * interval_bases\tsites_in_regions\tcells_masked", a line per sample in the array's order (its intervals and their bases after merging), then
 * the lines "all_samples_intervals", "all_samples_bases", "sites", "rows_in", "rows_all_samples", "rows_emptied", "rows_out", each with its
 * value behind a tab.  SKX_EINVAL for NULL arguments and an interval that names a sample that is not there or ends before it starts.  *buf is
 * malloc'd (skx_free). */
int skh_mask_text(const skx_mask_sample *samples, const skx_mask_info *info, const skx_mask_interval *iv, uint64_t n, const char *const *names, uint64_t n_samples,
                  char **buf, uint64_t *len);
/* `ska mask <REFERENCE> <SKF_FILE> -o OUT.skf (--regions FILE | --dense [--window W] [--min-snps T]) [--bed FILE] [--summary PREFIX]`: the file is
 * loaded once, unfiltered (skh_load_array); the intervals are those of regions_file (skh_mask_read_regions) or, with dense != 0, the regions of
 * skx_array_snp_density on the loaded array at window / min_snps -- the same file as `ska density` followed by `ska mask --regions` -- and those
 * of bed_file (skh_mask_read_bed); one call of skx_array_mask_regions; the array is saved as skh_save_skf saves it (".skf" appended unless
 * there) and, with summary_prefix, <PREFIX>.mask.summary.tsv written.  SKX_EINVAL before anything is loaded for NULL arguments, none of the
 * three sources, regions_file together with dense, W or T out of range (with dense), and an output that is the input file: the input is never
 * overwritten.  Otherwise the refusals are the readers' and the ABI's.  Phases: mask.load / mask.density / mask.read_intervals / mask.regions
 * (inside it mask.read_reference, .windows, .lookup, .kernels, .compact) / mask.save / mask.text. */
int skh_mask(skx_ctx *ctx, const char *reference_fasta, const char *skf_file, const char *out_file, const char *regions_file, int dense, uint64_t window,
             uint32_t min_snps, const char *bed_file, const char *summary_prefix);
/* `ska distance <skf>` (lib.rs:710-727 = load + generic_modes::distance), same one-pass load */
int skh_distance_skf_tsv(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, char **buf, uint64_t *len);
/* what `ska distance` writes besides its table (any of the two names may be NULL; NULL for the struct = nothing): `tree` = the file of
 * the midpoint-rooted neighbour-joining tree (skx_dist_nj + skh_nj_newick), `clusters` = the prefix of <prefix>.clusters.csv and
 * <prefix>.graph.dot (skh_distance_clusters at the two thresholds).  The reference leaves both to scripts/cluster_dists.py. */
typedef struct { const char *tree, *clusters; double cluster_snps, cluster_mismatches; } skh_dist_extras;
/* skh_distance_skf_tsv, and the extras from the same table */
int skh_distance_skf_tsv_extras(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, const skh_dist_extras *extras, char **buf, uint64_t *len);
/* `ska distance <skf> --query / --query-file / --query-skf`: the header and exactly those lines of skh_distance_skf_tsv's table in which Sample1
 * or Sample2 is a query sample, in the table's order and text.  names[n_names]: query samples by name (repeats collapse; one that is not in
 * the array: SKX_EINVAL "Could not find sample(s): {..}").  query_skf (NULL: none): a second file merged into the first in memory exactly as
 * skh_merge would (its refusals and messages), every sample of it a query; the table is then the merged array's.  The filters stay those of
 * the whole array.  One file: the one-pass filtered load, then skx_array_distance_query; two: skx_array_merge, then
 * skx_array_distance_query_filtered.  An empty query set is SKX_EINVAL. */
int skh_distance_query_tsv(skx_ctx *ctx, const char *skf_file, const char *query_skf, const char *const *names, int n_names, double min_freq,
                           int filt_ambig, char **buf, uint64_t *len);
/* `ska distance <skf> --max-snps / --max-mismatches / --closest`: the header and exactly those lines of skh_distance_skf_tsv's table that
 * skx_array_distance_select keeps under `spec`, in the table's order and text.  The same one-pass filtered load; the full table is never formed. */
int skh_distance_select_tsv(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, const skx_select_spec *spec, char **buf, uint64_t *len);
/* `ska distance <skf> --mst`: the header and the lines of skh_distance_skf_tsv's table that form its minimum spanning forest under `spec`
 * (skx_array_distance_mst), in the table's order and text.  The same one-pass filtered load; the full table is never formed. */
int skh_distance_mst_tsv(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, const skx_mst_spec *spec, char **buf, uint64_t *len);
/* `ska distance <skf> (--max-snps N | --max-mismatches P | --closest K | --mst ...) --sites PREFIX [--sites-max N]`: the table's selected lines as
 * skh_distance_select_tsv (spec) or skh_distance_mst_tsv (mst) give them -- exactly one of the two is not NULL -- and in <prefix>.sites.tsv the rows
 * that make up each line's Distance (skx_array_pair_sites; filter-ambiguous distances only).  The file is loaded with its split k-mers
 * (skh_load_array), the pairs come from skx_array_distance_select / skx_array_distance_mst with min_freq and the sites from skx_array_pair_sites
 * with the same min_freq and max_records (0: no limit).
 * <prefix>.sites.tsv: header "Sample1\tSample2\tUpper\tLower\tBase1\tBase2", one line per record, the pairs in the order of the table's lines,
 * rows ascending within a pair; Upper / Lower as <prefix>.markers.tsv spells them (skh_key_arms).
 * *buf is the table whenever the selection itself succeeded: when the sites are refused (SKX_ENOMEM above max_records, with the ABI's message)
 * the call returns the error and still hands the table back, and no sites file is written.
 * Phases: distance.pair_sweep / distance.table_text / distance.sites_count / distance.sites_write / distance.sites_text. */
int skh_distance_sites(skx_ctx *ctx, const char *skf_file, double min_freq, const skx_select_spec *spec, const skx_mst_spec *mst, const char *prefix,
                       uint64_t max_records, char **buf, uint64_t *len);
/* the two arms of a split k-mer of length k as `ska nk --full-info` spells them: upper and lower receive (k - 1) / 2 letters and a NUL each */
void skh_key_arms(const skx_key *key, int k, char *upper, char *lower);
/* the clusters of a forest at a ladder of SNP thresholds (host only): for each of the n_levels levels L, in the order given, the connected
 * components of the forest's lines whose distance as the table prints it ("%.2f") is <= L -- the single-linkage clusters of `--clusters
 * --cluster-snps L` when the forest is the whole table's -- numbered 1, 2, ... in ascending order of their lowest sample.  csv: the header
 * "id,snps_<L>,...,address" (every L printed "%g"), one line per sample in the array's order, names written as skh_clusters_csv writes them,
 * `address` the level columns joined by '.'.  pairs: i < j < n, as skx_array_distance_mst returns them. */
int skh_mst_levels_csv(const char *const *names, const skx_dist_pair *pairs, uint64_t n_pairs, int n, const double *levels, int n_levels, char **buf, uint64_t *len);
/* the joins of skx_dist_nj / skx_matrix_nj over n leaves as one line of Newick (host only).  A negative raw length is written as 0 and the
 * difference moved to the sibling branch of the same join, so the distance between the two joined nodes is kept (Kuhner-Felsenstein).
 * Midpoint root: the two leaves with the largest path distance in the corrected tree (ties to the lowest (id, id)), the root half way
 * along the path between them, on the first edge that reaches the half.  Children ordered by the lowest leaf id below them, lengths
 * %.5f, ";" and a newline at the end; a name holding any of ()[]':;, or white space in single quotes with inner quotes doubled. */
int skh_nj_newick(const char *const *names, const skx_nj_join *joins, int n, char **buf, uint64_t *len);
/* ---- a user's tree as joins (host only; no device is touched).  The reading half of a per-branch parsimony count on a tree; the device half
 * is not in the engine yet. ----
 * A rooted binary tree over n samples as n - 1 joins in the node numbering of skx_nj_join: nodes 0 .. n-1 are the samples, join t makes node
 * n + t from children (a, b), both < n + t; every node below the root 2n-2 is a child exactly once. */
typedef struct { uint32_t a, b; } skx_tree_join;
/* Newick text as such joins: the inverse of skh_nj_newick's spelling, and what IQ-TREE and rapidnj write.
 * names[n] are the samples, n >= 2; a leaf's label is matched to them exactly (the first of two equal names wins).  Inner nodes are numbered as
 * their ')' come, so join t is the t-th ')' of the text, children in the order of the text; joins receives n - 1 records.  Read: labels in single
 * quotes with '' for a quote inside, [comments], white space, branch lengths and inner labels (both read and dropped).  A root with three
 * children (a, b, c) becomes R = (a, Y), Y = (b, c) -- Y is node 2n-3 -- and *root_three (may be NULL) is set.  The nesting is kept on an
 * explicit stack: a caterpillar tree is as deep as it has leaves.  SKX_EINVAL with a message that begins "newick:" and names the position in the
 * text (a byte offset from 0) or the sample for: any other node with more than two children, a node with one child, a leaf that is not a sample,
 * a sample named twice or missing from the tree, text after the ';', a text that ends early, a comment or a quoted label without its end. */
int skh_newick_joins(const char *text, const char *const *names, int n, skx_tree_join *joins, int *root_three);
/* the tree of such joins as one line of Newick: topology, child order and root as the text skh_newick_joins read had them (root_three: its
 * root's three children again, the branch above the first with length[a] + length[Y]), length[2n-2] = an integer per node below the root (a count
 * of changes on the branch above it) as branch lengths, leaves spelled as skh_nj_newick spells them, inner nodes labelled n1, n2, ... in the
 * order of their ')' (n<t+1> is node n+t; the root has no label), ";" and a newline at the end. */
int skh_parsimony_newick(const char *const *names, const skx_tree_join *joins, int n, int root_three, const uint64_t *branch_changes, char **buf, uint64_t *len);
/* the same tree as a table: header "Node\tParent\tLeaves\tLowest leaf\tChanges", one line per node below the root in node order -- the samples,
 * then n1, n2, ... -- with its parent's label ("root" for the root), the leaves below it, the name of the lowest sample below it and the number
 * given for the branch above it.  The Y of a trifurcating root has no line: its children hang under "root", its number is added to the first child's. */
int skh_parsimony_branches(const char *const *names, const skx_tree_join *joins, int n, int root_three, const uint64_t *branch_changes, char **buf, uint64_t *len);
/* single-linkage clusters of a distance table (host only; names[n], d = the n(n-1)/2 pairs of skx_array_distance).  A pair is an edge when
 * its values as the TSV prints them (%.2f, %.5f, parsed back) satisfy snps <= max_snps && mismatches <= max_mismatches.  csv: header
 * "id,Cluster__autocolour", clusters numbered from 1 by size descending (ties: lowest sample index), rows by cluster then sample index,
 * names RFC 4180-quoted where they hold , " or a line break.  dot: "strict graph {", one node line per sample in sample order, one edge
 * line per edge in table order, "}"; " and \ in a name escaped with \.  Either output pointer pair may be NULL. */
int skh_distance_clusters(const char *const *names, const skx_dist *d, int n, double max_snps, double max_mismatches,
                          char **csv, uint64_t *csv_len, char **dot, uint64_t *dot_len);
/* the CSV half of skh_distance_clusters from the clusters themselves: labels[i] = the lowest sample of i's cluster (labels[labels[i]] ==
 * labels[i] <= i, refused otherwise), as skx_array_distance_banded returns them */
int skh_clusters_csv(const char *const *names, const uint32_t *labels, int n, char **csv, uint64_t *csv_len);
/* skh_distance_clusters' two rules as what a device compares (host only): a pair is an edge exactly when its key (the numerator of its distance:
 * over 1 with filt_ambig, over 36 without) is <= *kmax and its mismatch proportion, as a double, is <= *pmax.  Rounding to a fixed number of
 * decimals is monotone, so both exist; they are found by bisection against snprintf / strtod.  A max_snps no key exceeds gives *kmax = 2^62.
 * SKX_EINVAL for a NaN or a negative threshold. */
int skh_cluster_cutoffs(double max_snps, double max_mismatches, int filt_ambig, uint64_t *kmax, double *pmax);
/* `ska distance <skf> --no-table --tree / --clusters`: the files of skh_distance_skf_tsv_extras' extras, byte for byte, without the table and
 * without <prefix>.graph.dot (its edge list is the O(pairs) object this form avoids).  The same one-pass filtered load, then
 * skx_array_distance_banded_prefiltered: host memory is O(samples).  extras must name at least one of the two. */
int skh_distance_banded_files(skx_ctx *ctx, const char *skf_file, double min_freq, int filt_ambig, const skh_dist_extras *extras);
/* generic_modes::distance (generic_modes.rs:136-189): two-stage filter, then the long-form TSV with the
 * VariantDist Display format "{:.2}\t{:.5}\t{}\t{}" (merge_ska_array.rs:57-65) */
int skh_distance_tsv(skx_array *a, double min_freq, int filt_ambig, char **buf, uint64_t *len);
/* Display / Debug of MergeSkaArray as `ska nk [--full-info]` prints them (merge_ska_array.rs:649-698, lib.rs:808-827) */
int skh_nk(skx_array *a, int full_info, char **buf, uint64_t *len);
/* generic_modes::save_skf (generic_modes.rs:270-283): appends ".skf" unless already there */
int skh_save_skf(skx_array *a, const char *out_prefix);
/* io_utils::load_array (io_utils.rs:60-93) + the u64-then-u128 retry of lib.rs:635-661 */
int skh_load_array(skx_ctx *ctx, const char *const *inputs, int n_inputs, int threads, skx_array **out);
/* generic_modes::merge (generic_modes.rs:90-106): first file decides u64/u128 (lib.rs:728-741), the others must load as the
 * same type ("Failed to load input file (inconsistent k-mer lengths?)"); saved through save_skf (".skf" appended) */
int skh_merge(skx_ctx *ctx, const char *const *skf_files, int n_files, const char *out_prefix);
/* generic_modes::delete (generic_modes.rs:192-210): delete_samples then save (".skf" appended unless present) */
int skh_delete(skx_array *a, const char *const *names, int n_names, const char *out_file);
/* generic_modes::weed (generic_modes.rs:213-267): optional weed FASTA (FASTQ refused, ska_ref.rs:206-208), then the filter
 * with threshold floor(n_samples * min_freq) and update_kmers = true when anything is asked for; out_file NULL = no save */
int skh_weed(skx_array *a, const char *weed_file, int reverse, double min_freq, int filter_ambig_as_missing, int filter_type,
             int ambig_mask, int ignore_const_gaps, const char *out_file);
/* CoverageHistogram::fit_histogram + plot_hist (coverage.rs:151-250) on the device-built histogram: two-component Poisson
 * mixture by maximum likelihood (argmin's BFGS + back-tracking line search restated), cutoff = first count at which the
 * coverage component is the likelier one.  text = plot_hist's table (malloc'd; NULL to skip). */
int skh_cov(skx_ctx *ctx, const char *fastq_fwd, const char *fastq_rev, int k, int rc, char **text, uint64_t *len, uint64_t *cutoff);
/* the fit alone on an already truncated histogram (the reference's unit test drives exactly this, coverage.rs:369-385) */
int skh_cov_fit(const double *counts, uint64_t n, double *w0, double *c, uint64_t *cutoff);
/* io_utils::read_input_fastas sample-name rule (io_utils.rs:31-46) */
char *skh_sample_name(const char *path);
/* ---- the same modes over the GPUs of one node, one process per GPU; each function is the body of ONE rank
 * and is collective over `comm` (include/skx.h "Collectives").  The job's samples (all of them, in input order) are dealt to the
 * ranks in contiguous shards; a rank builds the dictionaries of its shard (skx_dictset_build_files), the key tables are all-gathered
 * (skx_keyset_allgather) and the rank holds its own columns over the global rows (skx_array_assemble_lazy).  This is what
 * build_and_merge's thread tree becomes when the workers are GPUs (merge_ska_dict.rs:354-417). */
typedef struct {
    const char *const *names, *const *file1, *const *file2;   /* the whole job; file2[i] may be NULL (file2 itself too) */
    int n_samples;
    int k, rc;
    skx_qual qual;
    int threads;
    double proportion_reads;                                   /* 0 == None */
    const char *output;                                        /* build: prefix of the .skf; align / distance: the file (NULL = stdout, rank 0) */
    int merge_parts;                                           /* build: rank 0 joins the per-rank parts into <output>.skf */
    double min_freq;
    int filter_type, mask_ambig, ignore_const_gaps, filter_ambig_as_missing;    /* align (generic_modes.rs:112-131) */
    int filt_ambig;                                            /* distance: !--allow-ambiguous */
    const skh_dist_extras *extras;                             /* distance: rank 0, which holds the table, also writes these (NULL: none) */
} skh_job;
/* `ska build`: one .skf per rank, <output>.part<r>of<N>.skf = the global rows x that rank's samples (each a valid MergeSkaArray;
 * `ska merge` joins them), or with merge_parts the one file generic_modes::save_skf would write */
int skh_build_sharded(skx_ctx *ctx, skx_comm *comm, const skh_job *job);
/* `ska align`: row statistics reduced over ranks, the filter decided identically everywhere, every rank writes its own samples'
 * records at their offsets of the one output file (write_fasta's order, merge_ska_array.rs:499-517) */
int skh_align_sharded(skx_ctx *ctx, skx_comm *comm, const skh_job *job);
/* `ska distance`: generic_modes::distance's two filters on the reduced statistics, then skx_array_distance_sharded; rank 0 writes the table */
int skh_distance_sharded(skx_ctx *ctx, skx_comm *comm, const skh_job *job);
/* generic_modes.rs:286-306 skalo (`ska lo`): the array of skf_file on the device (skx_array_lo_graph), then compaction, the DFS of depth
 * `depth` from every entry node on `threads` host threads, indels and SNPs on the host.  Writes <out_prefix>_indels.vcf and _snps.fas, and
 * with a single-record `reference` (NULL: none) also _pseudo_genomes.fas and _snps.vcf.  `missing`: the largest fraction of missing samples
 * (f32, as cli.rs declares it); `indel_kmers`: the most indel k-mers a path may hold.  SKX_EEMPTY (after the reference's log line) when the
 * graph has no entry node; SKX_EINVAL with the reference's panic text when the reference file holds more than one record. */
int skh_lo(skx_ctx *ctx, const char *skf_file, const char *reference, const char *out_prefix, float missing, size_t depth, size_t indel_kmers,
           int threads);
/* the `ska` command line (build | align | map | distance | nk | merge | delete | weed | cov | lo); returns the process exit code.
 * `--gpus N` on build / align / distance starts one process per GPU (this executable again, SKX_RANK / SKX_WORLD / SKX_COMM_ID_FILE in
 * their environment) and runs the sharded bodies above; a launcher of one's own sets the same variables. */
int skh_main(int argc, char **argv);
/* `ska --help | -h | help [cmd] | <cmd> --help | --version | -V` (cli.rs:154 `#[command(author, version, about)]`, propagate_version; per-flag
 * help cli.rs:168-459): 1 = answered on stdout (exit code 0), 0 = not a help / version request, 2 = `ska help <unknown>`.  skh_main calls it first. */
int skh_help(int argc, char **argv);
/* a line of the reference's logger (simple_logger: lib.rs:559-563, Warn by default, Info with -v) on stderr: level 0 = ERROR, 1 = WARN, 2 = INFO;
 * target = the Rust module the reference logs it from ("ska::io_utils" ...) */
void skh_log(int level, const char *target, const char *message);

#ifdef __cplusplus
}
#endif
#endif
