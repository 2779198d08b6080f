// ska_help.cpp -- `ska --help | -h | help [cmd]`, `ska <cmd> --help`, `ska --version | -V`: what clap derives from the reference's
// argument structs (cli.rs:154 `#[command(author, version, about)]`, `propagate_version`; per-subcommand arguments cli.rs:168-459),
// laid out the way clap 4 lays its help out (about, usage, arguments, options with defaults and possible values; printed on stdout,
// exit code 0, no banner: the reference parses its arguments before it prints anything, lib.rs:558-565).  The version is the
// reference's (Cargo.toml:3) -- this executable stands in for that release of `ska`; the engine's own extensions are marked.
#include "../../include/skx_host.h"
#include "../../include/skx.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

struct Opt { const char *flag; const char *value; const char *help; };
struct Cmd {
    const char *name, *about, *usage;
    std::vector<Opt> args, opts;
    std::vector<std::pair<const char *, std::vector<Opt>>> sections;   // clap's help_heading groups, after Options
};

const char *const THREADS = "Number of CPU threads [default: 1]";

const std::vector<Cmd> &commands()
{
    static const std::vector<Cmd> C = {
        {"build", "Create a split-kmer file from input sequences", "ska build [OPTIONS] -o <OUTPUT> <SEQ_FILES|-f <FILE_LIST>>",
         {{"[SEQ_FILES]...", "", "List of input FASTA files"}},
         {{"-f", "<FILE_LIST>", "File listing input files (tab separated name, sequences)"},
          {"-o", "<OUTPUT>", "Output prefix"},
          {"-k", "<K>", "K-mer size [default: 31]"},
          {"--proportion-reads", "<PROPORTION_READS>", "Number of reads before stopping"},
          {"--single-strand", "", "Ignore reverse complement (all contigs are oriented along same strand)"},
          {"--min-count", "<MIN_COUNT>", "Minimum k-mer count (with reads)"},
          {"--min-qual", "<MIN_QUAL>", "Minimum k-mer quality (with reads) [default: 20]"},
          {"--qual-filter", "<QUAL_FILTER>", "Quality filtering criteria (with reads) [default: strict] [possible values: no-filter, middle, strict]"},
          {"--threads", "<THREADS>", THREADS},
          {"--gpus", "<GPUS>", "(MI355X engine) Number of GPUs: one rank each, samples sharded by rank"},
          {"--merge", "", "(MI355X engine) With --gpus, join the per-rank files into one"}}},
        {"align", "Write an unordered alignment", "ska align [OPTIONS] <INPUT>...",
         {{"<INPUT>...", "", "A .skf file, or list of .fasta files"}},
         {{"-o", "<OUTPUT>", "Output filename (omit to output to stdout)"},
          {"-m, --min-freq", "<MIN_FREQ>", "Minimum fraction of samples a k-mer has to appear in [default: 0.9]"},
          {"--filter-ambig-as-missing", "", "With min_freq, only count non-ambiguous sites"},
          {"--filter", "<FILTER>", "Filter for constant middle base sites [default: no-const] [possible values: no-filter, no-const, no-ambig, no-ambig-or-const]"},
          {"--ambig-mask", "", "Mask any ambiguous bases in the alignment with 'N'"},
          {"--no-gap-only-sites", "", "Ignore gaps '-' in constant sites (for low coverage samples)"},
          {"--threads", "<THREADS>", THREADS},
          {"--gpus", "<GPUS>", "(MI355X engine) Number of GPUs (with sequence files or -f and the build options)"},
          {"--groups", "<FILE>", "(MI355X engine) One alignment per group from a single load: FILE lists sample name and group label (comma or tab separated; <PREFIX>.clusters.csv of `ska distance --clusters` is taken as it is); writes <OUTPUT>.<label>.aln per group and <OUTPUT>.groups.tsv"},
          {"--min-group-size", "<N>", "(MI355X engine) With --groups: skip groups of fewer than N samples [default: 2]"},
          {"--samples", "<NAMES>", "(MI355X engine) Align only these samples (comma separated), as `ska delete` of the others followed by `ska align` would"},
          {"--samples-file", "<FILE>", "(MI355X engine) The same, sample names from a file (one per line)"}}},
        {"map", "Write an ordered alignment using a reference sequence", "ska map [OPTIONS] <REFERENCE> [INPUT]...",
         {{"<REFERENCE>", "", "Reference FASTA file to map to"}, {"[INPUT]...", "", "A .skf file, or list of .fasta files"}},
         {{"-o", "<OUTPUT>", "Output filename (omit to output to stdout)"},
          {"-f, --format", "<FORMAT>", "Format of output file [default: aln] [possible values: vcf, aln]"},
          {"--ambig-mask", "", "Mask any ambiguous bases in the alignment with 'N'"},
          {"--repeat-mask", "", "Mask any repeats in the alignment with 'N'"},
          {"--threads", "<THREADS>", THREADS}}},
        {"distance", "Calculate SNP distances and k-mer mismatches", "ska distance [OPTIONS] <SKF_FILE>",
         {{"<SKF_FILE>", "", "Split-kmer (.skf) file to operate on"}},
         {{"-o", "<OUTPUT>", "Output filename (omit to output to stdout)"},
          {"-m, --min-freq", "<MIN_FREQ>", "Minimum fraction of samples a k-mer has to appear in across the entire alignment [default: 0]"},
          {"--allow-ambiguous", "", "Don't filter out ambiguous bases and compute fractional distances"},
          {"--threads", "<THREADS>", THREADS},
          {"--gpus", "<GPUS>", "(MI355X engine) Number of GPUs (with sequence files or -f and the build options)"},
          {"--tree", "<FILE>", "(MI355X engine) Write the midpoint-rooted neighbour-joining tree of the distances (Newick) to this file"},
          {"--clusters", "<PREFIX>", "(MI355X engine) Write single-linkage clusters to <PREFIX>.clusters.csv and their graph to <PREFIX>.graph.dot"},
          {"--cluster-snps", "<N>", "(MI355X engine) Largest SNP distance that links two samples (with --clusters) [default: 10]"},
          {"--cluster-mismatches", "<P>", "(MI355X engine) Largest mismatch proportion that links two samples (with --clusters) [default: 1.0]"},
          {"--no-table", "", "(MI355X engine) With --tree / --clusters: write those files only, from a banded sweep that never forms the table (no <PREFIX>.graph.dot; see --max-snps for the lines themselves)"},
          {"--sites", "<PREFIX>", "(MI355X engine) With --max-snps / --max-mismatches / --closest / --mst: list the split k-mers behind each printed line's Distance, and the base either sample has there, in <PREFIX>.sites.tsv"},
          {"--sites-max", "<N>", "(MI355X engine) With --sites: refuse to list more than N sites [default: 134217728]"},
          {"--query", "<NAMES>", "(MI355X engine) Print only the table's lines that name one of these samples (comma separated)"},
          {"--query-file", "<FILE>", "(MI355X engine) The same, sample names from a file (one per line)"},
          {"--query-skf", "<FILE>", "(MI355X engine) Merge this .skf into <SKF_FILE> in memory and print the lines that name one of its samples"},
          {"--max-snps", "<N>", "(MI355X engine) Print only the lines whose SNP distance is at most N"},
          {"--max-mismatches", "<P>", "(MI355X engine) Print only the lines whose mismatch proportion is at most P"},
          {"--closest", "<K>", "(MI355X engine) Print only the lines that join a sample to one of its K closest (among the lines the two thresholds keep)"},
          {"--mst", "", "(MI355X engine) Print only the lines of the table's minimum spanning forest (among the lines --max-snps / --max-mismatches keep; ties by the line's place in the table)"},
          {"--mst-clusters", "<PREFIX>", "(MI355X engine) With --mst: write every sample's cluster at each level of --levels, and their address, to <PREFIX>.levels.csv"},
          {"--levels", "<L1,L2,...>", "(MI355X engine) SNP distances at which --mst-clusters cuts the forest (1 to 16 numbers, comma separated) [default: 250,100,50,25,10,5,0]"}}},
        {"merge", "Combine multiple split k-mer files", "ska merge -o <OUTPUT> [SKF_FILES]...",
         {{"[SKF_FILES]...", "", "List of input split-kmer (.skf) files"}},
         {{"-o", "<OUTPUT>", "Output prefix"}}},
        {"delete", "Remove samples from a split k-mer file", "ska delete [OPTIONS] --skf-file <SKF_FILE> <-f <FILE_LIST>|NAMES>",
         {{"[NAMES]...", "", "List of sample names to remove"}},
         {{"-s, --skf-file", "<SKF_FILE>", "Split-kmer (.skf) file to operate on"},
          {"-o", "<OUTPUT>", "Output name. If not provided, will overwrite the input file"},
          {"-f", "<FILE_LIST>", "File listing sample names to remove"}}},
        {"weed", "Remove k-mers from a split k-mer file", "ska weed [OPTIONS] <SKF_FILE> [WEED_FILE]",
         {{"<SKF_FILE>", "", "Split-kmer (.skf) file to operate on"}, {"[WEED_FILE]", "", "A FASTA file containing sequences to remove"}},
         {{"-o", "<OUTPUT>", "Output filename (omit to overwrite input file)"},
          {"--reverse", "", "Remove k-mers not in the weed_file"},
          {"-m, --min-freq", "<MIN_FREQ>", "Minimum fraction of samples a k-mer has to appear in [default: 0.9]"},
          {"--filter-ambig-as-missing", "", "With min_freq, only count non-ambiguous sites"},
          {"--filter", "<FILTER>", "Filter for constant middle base sites [default: no-filter] [possible values: no-filter, no-const, no-ambig, no-ambig-or-const]"},
          {"--ambig-mask", "", "Mask any ambiguous bases in the alignment with 'N'"},
          {"--no-gap-only-sites", "", "Ignore gaps '-' in constant sites"}}},
        {"nk", "Get the number of k-mers in a split k-mer file, and other information", "ska nk [OPTIONS] <SKF_FILE>",
         {{"<SKF_FILE>", "", "Split-kmer (.skf) file to operate on"}},
         {{"--full-info", "", "Also write out split-kmers, and middle base matrix"}}},
        {"cov", "Estimate a coverage cutoff using a k-mer count profile (FASTQ only)", "ska cov [OPTIONS] <FASTQ_FWD> <FASTQ_REV>",
         {{"<FASTQ_FWD>", "", "FASTQ file (or .fastq.gz) with forward reads"}, {"<FASTQ_REV>", "", "FASTQ file (or .fastq.gz) with reverse reads"}},
         {{"-k", "<K>", "K-mer size [default: 31]"},
          {"--single-strand", "", "Ignore reverse complement (all reads are oriented along same strand)"}}},
        {"lo", "Finds 'left out' SNPs and INDELs using a graph", "ska lo [OPTIONS] <INPUT_SKF> <OUTPUT>",
         {{"<INPUT_SKF>", "", "input SKA2 file"}, {"<OUTPUT>", "", "prefix of output files"}},
         {},
         {{"input", {{"-r, --reference", "<REFERENCE>", "reference genome for SNP positioning"}}},
          {"output", {{"-m, --missing", "<MISSING>", "maximum fraction of missing data [default: 0.1]"}}},
          {"graph traversal", {{"-d, --depth", "<DEPTH>", "maximum depth of recursive paths [default: 4]"}}},
          {"other", {{"-n, --indel-kmers", "<INDEL_KMERS>", "maximum number of internal indel k-mers [default: 2]"},
                     {"--threads", "<THREADS>", THREADS}}}}},
        {"markers", "(MI355X engine) Find the split k-mers and middle-base alleles that tell each group of samples from everybody else", "ska markers [OPTIONS] --groups <FILE> -o <OUTPUT> <SKF_FILE>",
         {{"<SKF_FILE>", "", "Split-kmer (.skf) file to operate on"}},
         {{"--groups", "<FILE>", "Sample name and group label per line (comma or tab separated; <PREFIX>.clusters.csv of `ska distance --clusters` is taken as it is); samples it does not list count as others"},
          {"-o", "<OUTPUT>", "Output prefix: writes <OUTPUT>.markers.tsv and <OUTPUT>.markers.summary.tsv"},
          {"--min-in", "<P>", "Smallest fraction of a group's samples that must have the split k-mer [default: 1.0]"},
          {"--max-out", "<Q>", "Largest fraction of the other samples that may have a presence marker's split k-mer [default: 0.0]"},
          {"--min-group-size", "<N>", "Do not report groups of fewer than N samples (they still count as others) [default: 1]"},
          {"--kind", "<KIND>", "Markers to report [default: both] [possible values: presence, allele, both]"},
          {"--fasta", "", "Also write <OUTPUT>.<label>.markers.fa per group: `ska weed <SKF_FILE> <that file> --reverse --min-freq 0` keeps exactly its marker rows"}}},
        {"curve", "(MI355X engine) Count the split k-mers present, those passing --min-freq and the variant sites as samples are added one by one", "ska curve [OPTIONS] -o <OUTPUT> <SKF_FILE>",
         {{"<SKF_FILE>", "", "Split-kmer (.skf) file to operate on"}},
         {{"-o", "<OUTPUT>", "Output prefix: writes <OUTPUT>.curve.tsv (per number of samples: minimum, median, maximum and mean over the orders of pan, core, variant and core_variant)"},
          {"--permutations", "<P>", "Number of random orders of the samples, 1 to 10000 [default: 20]"},
          {"--seed", "<N>", "Seed of the random orders [default: 1]"},
          {"--min-freq", "<MIN_FREQ>", "Minimum fraction of the samples added so far a core k-mer has to appear in [default: 0.9]"},
          {"--order-file", "<FILE>", "One order instead of random ones: every sample name of <SKF_FILE> once, one per line (for instance by collection date); also writes <OUTPUT>.curve.permutations.tsv"},
          {"--all-permutations", "", "Also write <OUTPUT>.curve.permutations.tsv: every order's counts, the sample added and the new split k-mers at each step"}}},
        {"screen", "(MI355X engine) Report which samples carry which sequences of a panel, with the coverage and identity of each", "ska screen [OPTIONS] -o <OUTPUT> <SKF_FILE> <PANEL>",
         {{"<SKF_FILE>", "", "Split-kmer (.skf) file to operate on"}, {"<PANEL>", "", "FASTA file of the sequences to look for (genes, replicons, typing loci), one record each"}},
         {{"-o", "<OUTPUT>", "Output prefix: writes <OUTPUT>.screen.tsv (one line per record and sample that pass) and <OUTPUT>.screen.summary.tsv (one line per record)"},
          {"--min-cover", "<C>", "Smallest fraction of a record's split k-mers a sample must have, 0 to 1 [default: 0.9]"},
          {"--min-identity", "<I>", "Smallest fraction of the split k-mers found whose middle base must be the record's, 0 to 1 [default: 0]"},
          {"--matrix", "", "Also write <OUTPUT>.screen.matrix.tsv: records by samples, 1 where the pair passes and 0 where it does not"}}},
        {"qc", "(MI355X engine) Count per sample what tells a sample that should not be in the file, and flag the outliers", "ska qc [OPTIONS] -o <OUTPUT> <SKF_FILE>",
         {{"<SKF_FILE>", "", "Split-kmer (.skf) file to operate on"}},
         {{"-o", "<OUTPUT>", "Output prefix: writes <OUTPUT>.qc.tsv (per sample: split k-mers, ambiguous bases, singletons, core k-mers present and missing, private and minor alleles, flags), <OUTPUT>.qc.summary.tsv and <OUTPUT>.qc.flagged.txt (the flagged names, as `ska delete -f` reads them)"},
          {"--min-freq", "<MIN_FREQ>", "Minimum fraction of the samples a core k-mer has to appear in [default: 0.9]"},
          {"--mad", "<M>", "Flag a sample whose count lies more than M median absolute deviations from the median [default: 5]"}}},
        {"density", "(MI355X engine) Find per sample the stretches of a reference that carry a dense run of SNPs (recombination, to be masked before a tree is built)", "ska density [OPTIONS] -o <OUTPUT> <REFERENCE> <SKF_FILE>",
         {{"<REFERENCE>", "", "Reference FASTA file, as for `ska map`"}, {"<SKF_FILE>", "", "Split-kmer (.skf) file to operate on"}},
         {{"-o", "<OUTPUT>", "Output prefix: writes <OUTPUT>.density.regions.tsv (sample, chromosome, start, end, length, snps), <OUTPUT>.density.summary.tsv (one line per sample) and <OUTPUT>.density.bins.tsv (SNPs and dense SNPs of all samples per window of the reference)"},
          {"--window", "<W>", "Reference positions T SNPs of a sample must lie inside to count as dense, 1 to 2147483648; a convention, not a calibration [default: 1000]"},
          {"--min-snps", "<T>", "Number of consecutive SNPs of a sample inside a window that makes them dense, 2 to 65535; a convention, not a calibration [default: 5]"},
          {"--snps", "", "Also write <OUTPUT>.density.snps.tsv: every SNP (sample, chromosome, position, ref, alt) and whether it is dense"},
          {"--masked-aln", "<FILE>", "Also write `ska map --repeat-mask`'s alignment with every sample's regions overwritten by 'N': what a tree builder takes"}}},
        {"mask", "(MI355X engine) Take regions of a reference out of a .skf, per sample (the regions of `ska density`) or for every sample (a BED file), so that every command runs without them", "ska mask [OPTIONS] -o <OUTPUT> <--regions <FILE>|--dense|--bed <FILE>> <REFERENCE> <SKF_FILE>",
         {{"<REFERENCE>", "", "Reference FASTA file, as for `ska map` and `ska density`"}, {"<SKF_FILE>", "", "Split-kmer (.skf) file to operate on; it is never overwritten"}},
         {{"-o", "<OUTPUT>", "Output .skf file: the input with the cells of the regions made missing ('-') and the rows left without a sample removed"},
          {"--regions", "<FILE>", "Per-sample regions: <PREFIX>.density.regions.tsv of `ska density`, or any tab-separated file with a header line and sample, chromosome, start, end (1-based, inclusive)"},
          {"--dense", "", "Per-sample regions: those `ska density` finds on this file, from the same load; the same output as `ska density` followed by --regions"},
          {"--window", "<W>", "With --dense: reference positions T SNPs of a sample must lie inside to count as dense, 1 to 2147483648; a convention, not a calibration [default: 1000]"},
          {"--min-snps", "<T>", "With --dense: number of consecutive SNPs of a sample inside a window that makes them dense, 2 to 65535; a convention, not a calibration [default: 5]"},
          {"--bed", "<FILE>", "Regions to take out of every sample (phage, mobile elements, repeats): BED with chromosome, 0-based start, exclusive end; their split k-mers are removed"},
          {"--summary", "<PREFIX>", "Also write <PREFIX>.mask.summary.tsv: per sample its intervals, their bases, the sites inside them and the cells masked, then the rows removed"}}},
    };
    return C;
}

// clap's two-column form: flags with a short name start at column 2, long-only flags at column 6
std::string left_of(const Opt &o)
{
    std::string f = o.flag;
    std::string s = (f.size() > 1 && f[0] == '-' && f[1] == '-') ? "      " + f : "  " + f;
    if (o.value && *o.value) s += std::string(" ") + o.value;
    return s;
}
void table(FILE *out, const char *title, const std::vector<Opt> &rows)
{
    if (rows.empty()) return;
    size_t w = 0;
    std::vector<std::string> left;
    for (auto &r : rows) { left.push_back(left_of(r)); if (left.back().size() > w) w = left.back().size(); }
    fprintf(out, "\n%s:\n", title);
    for (size_t i = 0; i < rows.size(); i++) fprintf(out, "%-*s  %s\n", (int)w, left[i].c_str(), rows[i].help);
}
void command_help(FILE *out, const Cmd &c)
{
    fprintf(out, "%s\n\nUsage: %s\n", c.about, c.usage);
    table(out, "Arguments", c.args);
    std::vector<Opt> o = c.opts;
    o.push_back({"-v, --verbose", "", "Show progress messages"});
    o.push_back({"-h, --help", "", "Print help"});
    o.push_back({"-V, --version", "", "Print version"});
    table(out, "Options", o);
    for (auto &sec : c.sections) table(out, sec.first, sec.second);
}
void top_help(FILE *out)
{
    fprintf(out, "Split k-mer analysis\n\nUsage: ska [OPTIONS] <COMMAND>\n\nCommands:\n");
    size_t w = 4;
    for (auto &c : commands()) if (strlen(c.name) > w) w = strlen(c.name);
    for (auto &c : commands()) fprintf(out, "  %-*s  %s\n", (int)w, c.name, c.about);
    fprintf(out, "  %-*s  %s\n", (int)w, "help", "Print this message or the help of the given subcommand(s)");
    std::vector<Opt> o = {{"-v, --verbose", "", "Show progress messages"}, {"-h, --help", "", "Print help"}, {"-V, --version", "", "Print version"}};
    table(out, "Options", o);
}

}  // namespace

// the usage line clap prints under an error of subcommand `cmd` ("ska <cmd> ..."; the top-level one for an unknown name)
const char *skh_usage_line(const char *cmd)
{
    for (auto &c : commands()) if (!strcmp(cmd, c.name)) return c.usage;
    return "ska [OPTIONS] <COMMAND>";
}

// 1: the invocation was a help / version request and has been answered (exit code 0); 0: not one; 2: `ska help <unknown>`
extern "C" int skh_help(int argc, char **argv)
{
    if (argc < 2) return 0;
    const std::string first = argv[1];
    auto is_help = [](const char *s) { return !strcmp(s, "--help") || !strcmp(s, "-h"); };
    auto is_version = [](const char *s) { return !strcmp(s, "--version") || !strcmp(s, "-V"); };
    auto find = [](const std::string &n) -> const Cmd * { for (auto &c : commands()) if (n == c.name) return &c; return nullptr; };
    if (is_help(argv[1])) { top_help(stdout); fflush(stdout); return 1; }
    if (is_version(argv[1])) { printf("ska %s\n", skx_version()); fflush(stdout); return 1; }
    if (first == "help") {
        if (argc < 3) { top_help(stdout); fflush(stdout); return 1; }
        if (const Cmd *c = find(argv[2])) { command_help(stdout, *c); fflush(stdout); return 1; }
        fprintf(stderr, "error: unrecognized subcommand '%s'\n\nUsage: ska [OPTIONS] <COMMAND>\n\nFor more information, try '--help'.\n", argv[2]);
        return 2;
    }
    const Cmd *c = find(first);
    for (int i = 2; i < argc; i++) {
        if (!strcmp(argv[i], "--")) break;
        if (is_help(argv[i])) { if (c) command_help(stdout, *c); else top_help(stdout); fflush(stdout); return 1; }
        if (is_version(argv[i])) { printf("ska-%s %s\n", c ? c->name : first.c_str(), skx_version()); fflush(stdout); return 1; }       // propagate_version
    }
    return 0;
}
