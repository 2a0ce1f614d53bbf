// pansim_cli.cpp -- the `pansim` executable: the reference's command line
// (pansim/src/main.rs:17-152), validation (:195-247), generation loop (:429-528) and
// output files (:321-331, :467-499, :531-553) driving libpansim_hip.so through its C ABI.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pansim_hip.h"

struct Flag { const char *name; const char *help; const char *def; bool takes_value; };

// main.rs:21-151, in declaration order
static const Flag FLAGS[] = {
    { "pop_size", "Number of individuals in population.", "1000", true },
    { "core_size", "Number of nucleotides in core genome.", "1200000", true },
    { "pan_genes", "Total number of genes in pangenome (core + accessory).", "6000", true },
    { "core_genes", "Number of core genes in pangenome.", "2000", true },
    { "avg_gene_freq", "Average proportion of genes in pangenome present in an individual. Includes core and accessory genes.", "0.5", true },
    { "n_gen", "Number of generations to simulate.", "100", true },
    { "max_distances", "Maximum number of pairwise distances to calculate.", "100000", true },
    { "core_mu", "Average core SNP mutation rate (per site per genome per generation in core genome). Must be > 0.0.", "0.05", true },
    { "HR_rate", "Homologous recombination rate, as number of core sites transferred per core genome mutation.", "0.05", true },
    { "HGT_rate", "HGT rate, as number of accessory sites transferred per core genome mutation.", "0.05", true },
    { "rate_genes1", "Average number of accessory genes that are gained/lost per site per genome per generation in gene compartment 1. Must be >= 0.0.", "1.0", true },
    { "rate_genes2", "Average number of accessory genes that are gained/lost per site per genome per generation in gene compartment 2. Must be >= 0.0.", "1000.0", true },
    { "prop_genes2", "Proportion of pangenome made up of compartment 2 genes. Must be 0.0 <= X <= 1.0.", "0.1", true },
    { "prop_positive", "Proportion of pangenome made up of positively selected genes. Must be 0.0 <= X <= 1.0. If negative, neutral selection is simulated.", "-0.1", true },
    { "pos_lambda", "Lambda value for exponential distribution of positively selected genes. Must be > 0.0.", "10.0", true },
    { "neg_lambda", "Lambda value for exponential distribution of negatively selected genes. Must be > 0.0.", "10.0", true },
    { "seed", "Seed for random number generation.", "0", true },
    { "outpref", "Output prefix path.", "distances", true },
    { "print_dist", "Print per-generation average pairwise distances.", nullptr, false },
    { "print_matrices", "Prints core and accessory matrices.", nullptr, false },
    { "print_selection", "Prints selection coefficients.", nullptr, false },
    { "threads", "Number of threads.", "1", true },
    { "verbose", "Prints per generation information.", nullptr, false },
    { "no_control_genome_size", "Removes penalisation of genome sizes deviating from average.", nullptr, false },
    { "genome_size_penalty", "Multiplier for each gene difference between avg_gene_freq and observed value.", "0.99", true },
    { "competition_strength", "Strength of competition felt by strain to all others. 0.0 = no competition", "0.0", true },
};

// not a flag of the reference: number of core-site shards of this process, shard k on device k modulo the
// visible GPUs (include/pansim_hip.h, ps_multi); results do not depend on it
static const Flag EXT_FLAGS[] = {
    { "gpus", "Number of core-site shards, one per GPU (more shards than GPUs share them). Results do not depend on it.", "1", true },
    { "reference_seed_stream", "Draw the selection coefficients from the reference's own seeded stream (ChaCha12 StdRng, restated from the published algorithms of the rand / statrs crates, ziggurat tables recomputed: UNVERIFIED against a Pansim binary) instead of the build's Philox stream.", nullptr, false },
    { "save_state", "Write the state of the run after its last generation to this file (ps_sim_save), beside the usual outputs. One shard only (--gpus 1).", "", true },
    { "print_core_freqs", "Write the core genome's per-site base counts to <outpref>_core_freqs.tsv (one line A, C, G, T per site, tab separated) and its diversity summary to <outpref>_core_diversity.tsv (number of segregating sites, exact sum and mean of ALL pairwise core distances, minor-allele spectrum; docs/CORE_DIVERSITY.md), beside _freqs.txt.", nullptr, false },
    { "print_dist_hist", "Write the joint histogram of (core distance, accessory distance) over ALL pairs of the final population to <outpref>_dist_hist.tsv (core_bin, acc_bin, count per non-empty bin) and its summary to <outpref>_dist_hist_summary.tsv (docs/DISTANCE_HISTOGRAM.md), beside the usual outputs.", nullptr, false },
    { "dist_hist_bins", "Bins of --print_dist_hist as <core>,<accessory>: both at least 1, their product at most 16384.", "64,64", true },
    { "dist_hist_core_max", "Upper end of the core axis of --print_dist_hist as a distance (pairs at or above it land in the last bin and are counted as clamped). Must be > 0.0. Without it the axis ends just above the largest core distance found.", "", true },
    { "print_clusters", "Write the strain clusters of the final population -- the connected components over ALL pairs of the graph that joins two individuals when their core distance is at most --cluster_core_max and their accessory distance at most --cluster_acc_max -- to <outpref>_clusters.tsv (row, label per individual: the label is the smallest row of its cluster) and their summary to <outpref>_clusters_summary.tsv (docs/STRAIN_CLUSTERS.md), beside the usual outputs. Needs at least one of the two thresholds.", nullptr, false },
    { "cluster_core_max", "Largest core distance of a pair that --print_clusters joins. Must be >= 0.0. Without it the core distance is not looked at.", "", true },
    { "cluster_acc_max", "Largest accessory distance of a pair that --print_clusters joins. Must be 0.0 <= X <= 1.0. Without it the accessory distance is not looked at.", "", true },
    { "print_differentiation", "Write how the strain clusters of the final population -- those of --cluster_core_max / --cluster_acc_max, as --print_clusters finds them -- differ: per group its size, pairwise differences, monomorphic sites and private genes to <outpref>_diff_groups.tsv, per pair of groups the core differences over all cross pairs, the fixed sites, the gene differences and the genes fixed either way to <outpref>_diff_between.tsv, per core site the within-group and total differences to <outpref>_diff_sites.tsv, per accessory gene its carriers in every group to <outpref>_diff_genes.tsv and the summary with pi within, pi between and F_ST to <outpref>_diff_summary.tsv (docs/GROUP_DIFFERENTIATION.md), beside the usual outputs. Needs at least one of the two thresholds and pop_size <= 65536.", nullptr, false },
    { "diff_max_groups", "Largest number of groups of --print_differentiation: the largest clusters are taken. Must be 1 <= X <= 16.", "16", true },
    { "diff_min_size", "Smallest cluster that --print_differentiation takes as a group. Must be a whole number >= 1.", "2", true },
    { "print_tree", "Write the single-linkage tree of the final population -- the minimum spanning tree over ALL pairs under the distance chosen by --tree_metric, whose sorted edge weights are the heights at which strains merge -- to <outpref>_tree.tsv (lo, hi, num, den, distance per edge, ascending; the distance is num / den, NaN for an undefined one) and its summary to <outpref>_tree_summary.tsv (docs/LINKAGE_TREE.md), beside the usual outputs.", nullptr, false },
    { "tree_metric", "Distance of --print_tree: core or acc.", "core", true },
    { "print_upgma", "Write the average-linkage (UPGMA) tree of the final population -- the dendrogram over ALL pairs under the distance chosen by --upgma_metric, in which the distance of two clusters is the average over their cross pairs -- to <outpref>_upgma.tsv (node, left, right, size, num, den, distance per merge, in the order the merges are performed; the distance is num / den), as Newick text to <outpref>_upgma.nwk and its summary to <outpref>_upgma_summary.tsv (docs/UPGMA_TREE.md), beside the usual outputs. Needs pop_size <= 16384.", nullptr, false },
    { "upgma_metric", "Distance of --print_upgma: core or acc (acc needs core_genes >= 1).", "core", true },
    { "print_knn", "Write the <print_knn> nearest neighbours of every individual of the final population -- among ALL others, under the distance chosen by --knn_metric, ordered by (distance, row) -- to <outpref>_knn.tsv (row, rank from 1, neighbour, num, den, distance; the distance is num / den, NaN for an undefined one), the lineages at rank <print_knn> -- the connected components of the graph of those neighbours -- to <outpref>_lineages.tsv (row, label: the smallest row of its lineage) and the summary, with the number of lineages and the largest one at every rank up to <print_knn>, to <outpref>_knn_summary.tsv (docs/NEAREST_NEIGHBOURS.md), beside the usual outputs. Must be 1 <= X <= min(pop_size - 1, 128).", "", true },
    { "knn_metric", "Distance of --print_knn: core or acc.", "core", true },
    { "print_genealogy", "Record the parent draws of the last <print_genealogy> generations on the device and write the true genealogy of the final population: the comb to <outpref>_genealogy.tsv (rank, row, coal per individual in the order the engine stores them: coal is the number of generations back at which the individual and the next one share an ancestor, \"beyond\" when the record does not reach it, empty on the last line), its trees to <outpref>_genealogy.nwk (Newick, one line per root, branch lengths in generations), and ALL pairs binned by (divergence time, distance) to <outpref>_clock.tsv (time_bin, dist_bin, count per non-empty bin; time bin <Bt> holds the pairs beyond the record) with the summary and the mean distance per time bin in <outpref>_clock_summary.tsv (docs/GENEALOGY.md), beside the usual outputs. Must be a whole number >= 1. After --load_state the record starts at the loaded generation.", "", true },
    { "clock_bins", "Bins of --print_genealogy's clock histogram as <Bt>,<Bx> (time, distance): both at least 1, Bt at most 1024, (Bt + 1) x Bx at most 16384.", "32,64", true },
    { "clock_metric", "Distance of --print_genealogy's clock histogram: core or acc.", "core", true },
    { "print_ld", "Write the linkage disequilibrium between the loci of the final population -- r^2 and the four-gamete test over all pairs of the selected core sites or accessory genes (--ld_metric) -- to <outpref>_ld.tsv (lag_bin, r2_bin, count per non-empty bin; the lag bin is the floor of log2 of the distance between the two columns), its summary with the pairs and the sum of 65536 r^2 per lag bin to <outpref>_ld_summary.tsv and the selected loci to <outpref>_ld_loci.tsv (column, count) (docs/LINKAGE_DISEQUILIBRIUM.md), beside the usual outputs.", nullptr, false },
    { "ld_metric", "Loci of --print_ld: core (sites) or acc (genes).", "core", true },
    { "ld_max_loci", "Largest number of loci of --print_ld; more candidates are thinned evenly. Must be 1 <= X <= 65536.", "4096", true },
    { "ld_min_minor", "Smallest minor count of a locus of --print_ld. Must be a whole number >= 1.", "1", true },
    { "ld_bins", "Bins of --print_ld as <r2>,<lag>: both at least 1, lag at most 32, their product at most 16384.", "64,1", true },
    { "print_parsimony", "Put the two matrices of the final population on a tree by Fitch parsimony -- <print_parsimony> is upgma (the tree of --upgma_metric), tree (the single-linkage tree of --tree_metric) or genealogy (the recorded one: needs --print_genealogy; equal times are resolved left to right) -- and write the changes of every core site to <outpref>_parsimony_sites.tsv, per accessory gene its changes, gains and losses to <outpref>_parsimony_genes.tsv, per node its parent (-1 for a root), the core sites that change and the genes gained and lost on the branch above it to <outpref>_parsimony_branches.tsv (node, parent, site_changes, gene_gains, gene_losses), the tree with branch lengths in changes per site to <outpref>_parsimony.nwk (Newick, one line per root) and the summary with the homoplasic sites and the consistency index to <outpref>_parsimony_summary.tsv (docs/TREE_PARSIMONY.md), beside the usual outputs. Needs 2 <= pop_size <= 16384.", "", true },
    { "print_tree_compare", "Compare two trees of the final population over ALL pairs of individuals as <a>,<b> -- each of upgma (the tree of --upgma_metric), tree (the single-linkage tree of --tree_metric) or genealogy (the recorded one: needs --print_genealogy), a read as the truth -- and write the pairs binned by the heights at which the two trees join them to <outpref>_tree_compare.tsv (bin_a, bin_b, count per non-empty bin; bin <Ba> / <Bb> holds the pairs a / b does not join), every clade of both trees to <outpref>_tree_compare_clades.tsv (tree, node, size, val, shared: 1 when the other tree has the same clade) and the summary with the cophenetic correlation, the rooted triplets both trees resolve alike and the shared clades to <outpref>_tree_compare_summary.tsv (docs/TREE_COMPARISON.md), beside the usual outputs. Heights are the dense ranks of the merge distances for upgma and tree, the coalescence times for genealogy. Needs 2 <= pop_size <= 16384.", "", true },
    { "tree_compare_bins", "Bins of --print_tree_compare as <Ba>,<Bb>: both at least 1 and at most 1024, (Ba + 1) x (Bb + 1) at most 16384.", "32,32", true },
    { "load_state", "Start from a state file instead of a clonal population: --n_gen stays the TOTAL, generations [saved, n_gen) are run. pop_size, core_size, pan_genes and core_genes must be the file's; every other flag is this command line's (the same flags continue the saved run bit for bit, other flags branch off it). With --print_dist the earlier rows of _per_gen.tsv come from the file, which must have been saved with --print_dist. One shard only (--gpus 1).", "", true },
};

// clap 3's layout (the reference's own `pansim --help`, /root/reference/README.md:40-138): the options sorted by clap's
// key in byte order (uppercase first; -h / -V by their letters), the help text behind a 12-space indent,
// "[default: X]" appended as ordinary words, the whole filled greedily to 100 columns.
static void print_wrapped(const std::string &text, size_t indent, size_t width)
{
    std::string line;
    size_t i = 0;
    while (i < text.size()) {
        size_t j = text.find(' ', i);
        if (j == std::string::npos) j = text.size();
        const std::string word = text.substr(i, j - i);
        i = j + 1;
        if (!line.empty() && indent + line.size() + 1 + word.size() > width) {
            printf("%*s%s\n", (int)indent, "", line.c_str());
            line.clear();
        }
        if (!line.empty()) line += ' ';
        line += word;
    }
    if (!line.empty()) printf("%*s%s\n", (int)indent, "", line.c_str());
}

static void print_flag(const Flag &f, const char *short_name)
{
    if (short_name) printf("    -%s, --%s", short_name, f.name);
    else printf("        --%s", f.name);
    if (f.takes_value) printf(" <%s>", f.name);
    printf("\n");
    std::string text = f.help;
    if (f.takes_value && *f.def) text += std::string(" [default: ") + f.def + "]";      // (the file flags of the extensions have none)
    print_wrapped(text, 12, 100);
}

static void print_help(bool extensions)
{
    printf("pansim 0.1.0\nSamuel Horsfield shorsfield@ebi.ac.uk\n");
    print_wrapped("Runs Wright-Fisher simulation, simulating neutral core genome evolution and two-speed accessory genome evolution.", 0, 100);
    printf("\nUSAGE:\n    pansim [OPTIONS]\n\nOPTIONS:\n");
    static const Flag HELP = { "help", "Print help information", nullptr, false }, VERSION = { "version", "Print version information", nullptr, false };
    std::vector<std::pair<const Flag *, const char *>> all;
    for (const Flag &f : FLAGS) all.push_back({ &f, nullptr });
    all.push_back({ &HELP, "h" });
    all.push_back({ &VERSION, "V" });
    // (clap's sort key: the long name, or for an option with a short one that letter in lower case followed by '0' if it
    // is a lower-case letter and '1' if not: "h0" lands behind genome_size_penalty, "v1" between threads and verbose)
    auto key = [](const std::pair<const Flag *, const char *> &x) {
        if (!x.second) return std::string(x.first->name);
        const char c = x.second[0];
        return std::string(1, (char)tolower(c)) + (islower(c) ? '0' : '1');
    };
    std::sort(all.begin(), all.end(), [&](const std::pair<const Flag *, const char *> &x, const std::pair<const Flag *, const char *> &y) { return key(x) < key(y); });
    for (size_t k = 0; k < all.size(); k++) {
        if (k) printf("\n");
        print_flag(*all[k].first, all[k].second);
    }
    if (extensions) {
        // (not part of the reference's --help: shown by --help-extensions only, so that --help stays the reference's text)
        printf("\nMI355X OPTIONS (not in the reference):\n");
        for (const Flag &f : EXT_FLAGS) {
            print_flag(f, nullptr);
            printf("\n");
        }
        printf("        --help-extensions\n            Print this help with the options above.\n");
    }
}

[[noreturn]] static void die(int code, const std::string &msg)
{
    fprintf(stderr, "%s\n", msg.c_str());
    exit(code);
}

// value_of_t::<f64>(..).unwrap() (main.rs:155-186): a value that does not parse panics (exit 101)
static double as_f64(const std::map<std::string, std::string> &v, const char *name)
{
    const std::string &s = v.at(name);
    char *end = nullptr;
    const double x = strtod(s.c_str(), &end);
    if (s.empty() || *end != 0)
        die(101, "error: Invalid value \"" + s + "\" for '--" + name + "': invalid float literal");
    return x;
}
static uint64_t as_u64(const std::map<std::string, std::string> &v, const char *name)
{
    const std::string &s = v.at(name);
    char *end = nullptr;
    if (s.empty() || s[0] == '-') die(101, "error: Invalid value \"" + s + "\" for '--" + name + "': invalid digit found in string");
    const unsigned long long x = strtoull(s.c_str(), &end, 10);
    if (*end != 0) die(101, "error: Invalid value \"" + s + "\" for '--" + name + "': invalid digit found in string");
    return x;
}
// `raw_f64.round() as usize` (main.rs:155-162): saturating cast
static uint64_t round_usize(double x)
{
    const double r = std::round(x);
    if (!(r > 0.0)) return 0;
    if (r >= 18446744073709551615.0) return UINT64_MAX;
    return (uint64_t)r;
}

static std::string fmt(double v)
{
    char buf[512];
    ps_fmt_f64(v, buf, sizeof buf);
    return buf;
}

// "<core>\t<acc>\n" per pair (main.rs:471-482).  The shortest-round-trip formatting of 2 P doubles
// is the whole cost of the file at cfg5 (33.5 M lines), so chunks of pairs are formatted by the
// host's threads into buffers that are then written in order.
static void write_pairs_tsv(FILE *f, const std::vector<double> &cd, const std::vector<double> &ad)
{
    const uint64_t P = cd.size();
    const uint64_t chunk = 1u << 16;
    const uint64_t nchunks = (P + chunk - 1) / chunk;
    const uint64_t hw = std::thread::hardware_concurrency();
    const unsigned nthreads = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(hw, nchunks), 32));
    for (uint64_t c0 = 0; c0 < nchunks; c0 += nthreads) {
        const unsigned n = (unsigned)std::min<uint64_t>(nthreads, nchunks - c0);
        std::vector<std::string> out(n);
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < n; t++)
            pool.emplace_back([&, t] {
                const uint64_t a = (c0 + t) * chunk, b = std::min(P, a + chunk);
                std::string &o = out[t];
                o.reserve((size_t)(b - a) * 40);
                char buf[512];
                for (uint64_t k = a; k < b; k++) {
                    o.append(buf, (size_t)ps_fmt_f64(cd[k], buf, sizeof buf));
                    o.push_back('\t');
                    o.append(buf, (size_t)ps_fmt_f64(ad[k], buf, sizeof buf));
                    o.push_back('\n');
                }
            });
        for (auto &th : pool) th.join();
        for (unsigned t = 0; t < n; t++) fwrite(out[t].data(), 1, out[t].size(), f);
    }
}

// the output file <outpref><suffix>, created or cut to nothing
static FILE *open_out(const std::string &outpref, const char *suffix)
{
    FILE *f = fopen((outpref + suffix).c_str(), "w");
    if (!f) die(1, "Error: cannot create " + outpref + suffix);
    return f;
}

// the value of a --<name>_metric flag: core (0) or acc (1), the constants of every metric of include/pansim_hip.h
static int32_t metric_flag(std::map<std::string, std::string> &val, const char *name)
{
    const std::string &v = val[name];
    if (v != "core" && v != "acc") die(101, std::string("pansim: --") + name + " must be core or acc, not \"" + v + "\"");
    return v == "acc" ? 1 : 0;
}
static_assert(PS_TREE_CORE == 0 && PS_TREE_ACC == 1 && PS_KNN_CORE == 0 && PS_KNN_ACC == 1 && PS_LD_CORE == 0 && PS_LD_ACC == 1, "metric_flag");

#define CK(call)                                                        \
    do {                                                                \
        if ((call) != PS_OK) die(101, std::string("pansim: ") + ps_last_error()); \
    } while (0)

int main(int argc, char **argv)
{
    std::map<std::string, std::string> val;
    std::map<std::string, bool> present;
    for (const Flag &f : FLAGS) {
        if (f.takes_value) val[f.name] = f.def;
        else present[f.name] = false;
    }
    for (const Flag &f : EXT_FLAGS) {
        if (f.takes_value) val[f.name] = f.def;
        else present[f.name] = false;
    }
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "-h" || a == "--help") { print_help(false); return 0; }
        if (a == "--help-extensions") { print_help(true); return 0; }
        if (a == "-V" || a == "--version") { printf("pansim 0.1.0\n"); return 0; }
        if (a.rfind("--", 0) != 0)
            die(2, "error: Found argument '" + a + "' which wasn't expected, or isn't valid in this context\n\nUSAGE:\n    pansim [OPTIONS]\n\nFor more information try --help");
        std::string name = a.substr(2), value;
        bool has_eq = false;
        const size_t eq = name.find('=');
        if (eq != std::string::npos) { value = name.substr(eq + 1); name = name.substr(0, eq); has_eq = true; }
        const Flag *fl = nullptr;
        for (const Flag &f : FLAGS)
            if (name == f.name) fl = &f;
        for (const Flag &f : EXT_FLAGS)
            if (name == f.name) fl = &f;
        if (!fl)
            die(2, "error: Found argument '--" + name + "' which wasn't expected, or isn't valid in this context\n\nUSAGE:\n    pansim [OPTIONS]\n\nFor more information try --help");
        if (!fl->takes_value) {
            if (has_eq) die(2, "error: The argument '--" + name + "' takes no value");
            present[name] = true;
            continue;
        }
        if (!has_eq) {
            if (i + 1 >= argc)
                die(2, "error: The argument '--" + name + " <" + name + ">' requires a value but none was supplied");
            value = argv[++i];
            // only prop_positive allows a leading hyphen (main.rs:91)
            if (value.rfind("-", 0) == 0 && name != "prop_positive" && value.size() > 1
                && !(value[1] >= '0' && value[1] <= '9') && value[1] != '.')
                die(2, "error: The argument '--" + name + " <" + name + ">' requires a value but none was supplied");
        }
        val[name] = value;
    }

    ps_sim_params p;
    ps_sim_default_params(&p);
    p.pop_size = round_usize(as_f64(val, "pop_size"));                 // main.rs:155-156
    p.core_size = round_usize(as_f64(val, "core_size"));
    p.pan_genes = round_usize(as_f64(val, "pan_genes"));
    p.core_genes = round_usize(as_f64(val, "core_genes"));
    p.avg_gene_freq = as_f64(val, "avg_gene_freq");
    p.HR_rate = as_f64(val, "HR_rate");
    p.HGT_rate = as_f64(val, "HGT_rate");
    {
        const double r = std::round(as_f64(val, "n_gen"));               // `as i32` saturates
        p.n_gen = r >= 2147483647.0 ? 2147483647 : r <= -2147483648.0 ? INT32_MIN : (int32_t)r;
    }
    const std::string outpref = val["outpref"];
    p.max_distances = as_u64(val, "max_distances");                    // main.rs:169 (usize)
    p.core_mu = as_f64(val, "core_mu");
    p.rate_genes1 = as_f64(val, "rate_genes1");
    p.rate_genes2 = as_f64(val, "rate_genes2");
    p.prop_genes2 = as_f64(val, "prop_genes2");
    p.prop_positive = as_f64(val, "prop_positive");
    p.pos_lambda = as_f64(val, "pos_lambda");
    p.neg_lambda = as_f64(val, "neg_lambda");
    (void)as_u64(val, "threads");                                      // main.rs:177; the GPU grid replaces the rayon pool
    (void)as_f64(val, "seed");                                         // main.rs:179
    p.seed = as_u64(val, "seed");                                      // main.rs:180
    p.verbose = present["verbose"];
    p.print_dist = present["print_dist"];
    p.print_matrices = present["print_matrices"];
    p.print_selection = present["print_selection"];
    p.no_control_genome_size = present["no_control_genome_size"];
    p.genome_size_penalty = as_f64(val, "genome_size_penalty");
    p.competition_strength = as_f64(val, "competition_strength");
    p.reference_seed_stream = present["reference_seed_stream"];

    // main.rs:195-247: message on stdout, exit status 0, no files
    char msg[2048];
    if (ps_sim_validate(&p, msg, sizeof msg) != PS_OK) {
        fputs(msg, stdout);
        return 0;
    }
    ps_derived d;
    CK(ps_sim_derive(&p, &d));
    if (p.verbose) printf("avg_gene_freq adjusted to %s\n", fmt(d.avg_gene_freq_adj).c_str()); // main.rs:269-271

    // one ps_sim per core-site shard (one shard: the plain run); main.rs:372-427
    const uint64_t n_shards = as_u64(val, "gpus");
    if (n_shards < 1 || n_shards > 1024) die(101, "pansim: --gpus must be 1..1024");
    const std::string save_state = val["save_state"], load_state = val["load_state"];
    if (n_shards > 1 && !(save_state.empty() && load_state.empty()))
        die(101, "pansim: --save_state / --load_state need --gpus 1: a sharded run is saved shard by shard through the library "
                 "(ps_multi_shard + ps_sim_save) and loaded as one ps_sim per shard");
    // --print_dist_hist: its two optional flags are checked whether or not it is given
    ps_pair_hist_params hist_prm = { 64, 64, 0 };
    {
        const std::string &b = val["dist_hist_bins"];
        unsigned long long bc = 0, ba = 0;
        int used = 0;
        if (sscanf(b.c_str(), "%llu,%llu%n", &bc, &ba, &used) != 2 || (size_t)used != b.size() || b.find_first_of("+- ") != std::string::npos)
            die(101, "pansim: --dist_hist_bins must be <core>,<accessory> (two whole numbers), not \"" + b + "\"");
        if (bc < 1 || ba < 1) die(101, "pansim: --dist_hist_bins must be at least 1 on both axes");
        if (bc > 16384 || ba > 16384 || bc * ba > 16384)
            die(101, "pansim: --dist_hist_bins " + b + ": the product of the two must be at most 16384");
        hist_prm.core_bins = (uint32_t)bc;
        hist_prm.acc_bins = (uint32_t)ba;
        if (!val["dist_hist_core_max"].empty()) {
            const double cm = as_f64(val, "dist_hist_core_max");
            if (!(cm > 0.0) || !std::isfinite(cm)) die(101, "pansim: --dist_hist_core_max must be > 0.0");
            const double span = std::ceil(cm * (double)p.core_size);      // core_span = max(1, ceil(core_max * L))
            hist_prm.core_span = span >= 18446744073709551615.0 ? UINT64_MAX : std::max<uint64_t>(1, (uint64_t)span);
        }
    }
    // --print_clusters: its thresholds are checked whether or not it is given; the integers of docs/STRAIN_CLUSTERS.md
    ps_cluster_params cluster_prm = { UINT64_MAX, 0, 0 };
    if (!val["cluster_core_max"].empty()) {
        const double cm = as_f64(val, "cluster_core_max");
        if (!(cm >= 0.0) || !std::isfinite(cm)) die(101, "pansim: --cluster_core_max must be >= 0.0");
        const double dmax = std::floor(cm * (double)p.core_size);      // core_max_d = floor(core_max * L)
        cluster_prm.core_max_d = dmax >= 18446744073709551615.0 ? UINT64_MAX - 1 : (uint64_t)dmax;
    }
    if (!val["cluster_acc_max"].empty()) {
        const double am = as_f64(val, "cluster_acc_max");
        if (!(am >= 0.0 && am <= 1.0)) die(101, "pansim: --cluster_acc_max must be 0.0 <= X <= 1.0");
        cluster_prm.acc_den = 1u << 20;                                 // acc_num / acc_den = floor(acc_max * 2^20) / 2^20
        cluster_prm.acc_num = (uint32_t)std::floor(am * (double)cluster_prm.acc_den);
    }
    if (present["print_clusters"] && cluster_prm.core_max_d == UINT64_MAX && cluster_prm.acc_den == 0)
        die(101, "pansim: --print_clusters needs --cluster_core_max, --cluster_acc_max or both");
    // --print_differentiation: its two parameters are checked whether or not it is given
    ps_diff_params diff_prm = { 16, 2 };
    {
        auto whole = [&](const char *name, unsigned long long lo, unsigned long long hi, const char *range) {
            const std::string &t = val[name];
            unsigned long long v = 0;
            int used = 0;
            if (sscanf(t.c_str(), "%llu%n", &v, &used) != 1 || (size_t)used != t.size() || t.find_first_of("+- ") != std::string::npos || v < lo || v > hi)
                die(101, std::string("pansim: --") + name + " must be " + range + ", not \"" + t + "\"");
            return (uint32_t)v;
        };
        diff_prm.max_groups = whole("diff_max_groups", 1, PS_GROUPS_MAX, "1 <= X <= 16");
        diff_prm.min_size = whole("diff_min_size", 1, 0xffffffffull, "a whole number >= 1");
    }
    if (present["print_differentiation"]) {
        if (cluster_prm.core_max_d == UINT64_MAX && cluster_prm.acc_den == 0)
            die(101, "pansim: --print_differentiation needs --cluster_core_max, --cluster_acc_max or both");
        if (p.pop_size > 65536) die(101, "pansim: --print_differentiation needs pop_size <= 65536, not --pop_size " + std::to_string(p.pop_size));
    }
    // --print_tree: its metric is checked whether or not it is given
    const ps_tree_params tree_prm = { metric_flag(val, "tree_metric") };
    // --print_upgma: its metric is checked whether or not it is given
    const ps_tree_params upgma_prm = { metric_flag(val, "upgma_metric") };
    // (the limits of ps_upgma_tree that the flags already decide, before any device work; exact after --load_state as well:
    // pop_size and core_genes must be the state file's, ps_sim_load refuses a file that differs)
    if (present["print_upgma"]) {
        if (p.pop_size < 2 || p.pop_size > 16384)
            die(101, "pansim: --print_upgma needs 2 <= pop_size <= 16384, not --pop_size " + std::to_string(p.pop_size));
        if (upgma_prm.metric == PS_TREE_ACC && p.core_genes < 1)
            die(101, "pansim: --upgma_metric acc needs core_genes >= 1, not --core_genes " + std::to_string(p.core_genes));
    }
    // --print_knn: its metric is checked whether or not it is given
    ps_knn_params knn_prm = { metric_flag(val, "knn_metric"), 0 };
    const bool print_knn = !val["print_knn"].empty();
    if (print_knn) {
        const std::string &t = val["print_knn"];
        unsigned long long k = 0;
        int used = 0;
        if (sscanf(t.c_str(), "%llu%n", &k, &used) != 1 || (size_t)used != t.size() || t.find_first_of("+- ") != std::string::npos)
            die(101, "pansim: --print_knn must be a whole number, not \"" + t + "\"");
        if (k < 1 || k > PS_KNN_MAX_K || k + 1 > p.pop_size)
            die(101, "pansim: --print_knn must be 1 <= X <= min(pop_size - 1, 128), not " + t + " with --pop_size " + std::to_string(p.pop_size));
        knn_prm.k = (uint32_t)k;
    }
    // --print_genealogy: the bins and the metric of its clock histogram are checked whether or not it is given
    ps_clock_params clock_prm = { metric_flag(val, "clock_metric"), 32, 64, 0, 0 };
    {
        const std::string &b = val["clock_bins"];
        unsigned long long bt = 0, bx = 0;
        int used = 0;
        if (sscanf(b.c_str(), "%llu,%llu%n", &bt, &bx, &used) != 2 || (size_t)used != b.size() || b.find_first_of("+- ") != std::string::npos)
            die(101, "pansim: --clock_bins must be <Bt>,<Bx> (two whole numbers), not \"" + b + "\"");
        if (bt < 1 || bx < 1) die(101, "pansim: --clock_bins must be at least 1 on both axes");
        if (bt > 1024 || bx > 16384 || (bt + 1) * bx > 16384)
            die(101, "pansim: --clock_bins " + b + ": Bt must be at most 1024 and (Bt + 1) x Bx at most 16384");
        clock_prm.time_bins = (uint32_t)bt;
        clock_prm.dist_bins = (uint32_t)bx;
    }
    // --print_ld: its metric, bins and selection are checked whether or not it is given
    ps_ld_params ld_prm = { 64, 1, 1, 4096 };
    const int32_t ld_metric = metric_flag(val, "ld_metric");
    {
        const std::string &b = val["ld_bins"];
        unsigned long long br = 0, bl = 0;
        int used = 0;
        if (sscanf(b.c_str(), "%llu,%llu%n", &br, &bl, &used) != 2 || (size_t)used != b.size() || b.find_first_of("+- ") != std::string::npos)
            die(101, "pansim: --ld_bins must be <r2>,<lag> (two whole numbers), not \"" + b + "\"");
        if (br < 1 || bl < 1) die(101, "pansim: --ld_bins must be at least 1 on both axes");
        if (bl > 32 || br > 16384 || br * bl > 16384)
            die(101, "pansim: --ld_bins " + b + ": lag must be at most 32 and the product of the two at most 16384");
        ld_prm.r2_bins = (uint32_t)br;
        ld_prm.lag_bins = (uint32_t)bl;
        const std::pair<const char *, uint32_t *> whole[] = { { "ld_max_loci", &ld_prm.max_loci }, { "ld_min_minor", &ld_prm.min_minor } };
        for (const auto &w : whole) {
            const std::string &t = val[w.first];
            unsigned long long v = 0;
            if (sscanf(t.c_str(), "%llu%n", &v, &used) != 1 || (size_t)used != t.size() || t.find_first_of("+- ") != std::string::npos)
                die(101, std::string("pansim: --") + w.first + " must be a whole number, not \"" + t + "\"");
            if (v < 1 || v > 0xffffffffull) die(101, std::string("pansim: --") + w.first + " must be at least 1 and below 2^32, not " + t);
            *w.second = (uint32_t)v;
        }
        if (ld_prm.max_loci > PS_LD_MAX_LOCI) die(101, "pansim: --ld_max_loci must be 1 <= X <= 65536, not " + val["ld_max_loci"]);
    }
    // --print_parsimony: the tree it names, before any device work
    const std::string pars_source = val["print_parsimony"];
    if (!pars_source.empty()) {
        if (pars_source != "upgma" && pars_source != "tree" && pars_source != "genealogy")
            die(101, "pansim: --print_parsimony must be upgma, tree or genealogy, not \"" + pars_source + "\"");
        if (pars_source == "genealogy" && val["print_genealogy"].empty())
            die(101, "pansim: --print_parsimony genealogy needs --print_genealogy: nothing is recorded without it");
        if (p.pop_size < 2 || p.pop_size > PS_PARS_MAX_POP)
            die(101, "pansim: --print_parsimony needs 2 <= pop_size <= 16384, not --pop_size " + std::to_string(p.pop_size));
        if (pars_source == "upgma" && upgma_prm.metric == PS_TREE_ACC && p.core_genes < 1)
            die(101, "pansim: --upgma_metric acc needs core_genes >= 1, not --core_genes " + std::to_string(p.core_genes));
    }
    // --print_tree_compare: the two trees it names and the bins, before any device work
    std::string tcmp_source[2];
    ps_tree_compare_params tcmp_prm = { 32, 32, 0, 0, 1 };
    if (!val["print_tree_compare"].empty()) {
        const std::string &t = val["print_tree_compare"];
        const size_t comma = t.find(',');
        tcmp_source[0] = t.substr(0, comma);
        tcmp_source[1] = comma == std::string::npos ? "" : t.substr(comma + 1);
        for (const std::string &x : tcmp_source)
            if (x != "upgma" && x != "tree" && x != "genealogy")
                die(101, "pansim: --print_tree_compare must be <a>,<b>, each of upgma, tree or genealogy, not \"" + t + "\"");
        if (tcmp_source[0] == tcmp_source[1]) die(101, "pansim: --print_tree_compare needs two different trees, not \"" + t + "\"");
        if ((tcmp_source[0] == "genealogy" || tcmp_source[1] == "genealogy") && val["print_genealogy"].empty())
            die(101, "pansim: --print_tree_compare genealogy needs --print_genealogy: nothing is recorded without it");
        if (p.pop_size < 2 || p.pop_size > PS_PARS_MAX_POP)
            die(101, "pansim: --print_tree_compare needs 2 <= pop_size <= 16384, not --pop_size " + std::to_string(p.pop_size));
        if ((tcmp_source[0] == "upgma" || tcmp_source[1] == "upgma") && upgma_prm.metric == PS_TREE_ACC && p.core_genes < 1)
            die(101, "pansim: --upgma_metric acc needs core_genes >= 1, not --core_genes " + std::to_string(p.core_genes));
        const std::string &b = val["tree_compare_bins"];
        unsigned long long ba = 0, bb = 0;
        int used = 0;
        if (sscanf(b.c_str(), "%llu,%llu%n", &ba, &bb, &used) != 2 || (size_t)used != b.size() || b.find_first_of("+- ") != std::string::npos)
            die(101, "pansim: --tree_compare_bins must be <Ba>,<Bb> (two whole numbers), not \"" + b + "\"");
        if (ba < 1 || bb < 1) die(101, "pansim: --tree_compare_bins must be at least 1 on both axes");
        if (ba > 1024 || bb > 1024 || (ba + 1) * (bb + 1) > 16384)
            die(101, "pansim: --tree_compare_bins " + b + ": both must be at most 1024 and (Ba + 1) x (Bb + 1) at most 16384");
        tcmp_prm.bins_a = (uint32_t)ba;
        tcmp_prm.bins_b = (uint32_t)bb;
    }
    uint32_t record_capacity = 0;
    if (!val["print_genealogy"].empty()) {
        const std::string &t = val["print_genealogy"];
        unsigned long long c = 0;
        int used = 0;
        if (sscanf(t.c_str(), "%llu%n", &c, &used) != 1 || (size_t)used != t.size() || t.find_first_of("+- ") != std::string::npos)
            die(101, "pansim: --print_genealogy must be a whole number, not \"" + t + "\"");
        if (c < 1 || c > 0xffffffffull) die(101, "pansim: --print_genealogy must be 1 <= X < 2^32 generations, not " + t);
        record_capacity = (uint32_t)c;
        // (a coalescence time is a value of ps_tree_compare: at most 2^18 - 1)
        if ((tcmp_source[0] == "genealogy" || tcmp_source[1] == "genealogy") && c > 262143)
            die(101, "pansim: --print_tree_compare genealogy needs --print_genealogy <= 262143 generations, not " + t);
    }
    const uint64_t G = d.pan_size, P = p.max_distances;
    std::vector<double> avg_core(p.n_gen), avg_acc(p.n_gen), std_core(p.n_gen), std_acc(p.n_gen);
    // a fresh run goes through ps_multi (one shard: the plain run); a LOADED run is a plain ps_sim, driven by the ps_sim_*
    // calls ps_multi itself makes for one shard
    ps_multi *multi = nullptr;
    ps_sim *sim = nullptr;
    int32_t g0 = 0;
    if (!load_state.empty()) {
        ps_state_header sh;
        CK(ps_state_info(load_state.c_str(), nullptr, &sh, nullptr, 0));
        if ((uint64_t)p.n_gen < sh.generations_done)
            die(101, "pansim: --n_gen is the total number of generations: " + load_state + " already holds " + std::to_string(sh.generations_done)
                         + ", --n_gen " + std::to_string(p.n_gen) + " asks for fewer");
        g0 = (int32_t)sh.generations_done;
        if (p.print_dist) {
            if (!sh.has_per_gen)
                die(101, "pansim: " + load_state + " was saved without --print_dist: it has no rows of _per_gen.tsv for its "
                             + std::to_string(g0) + " generations, so this run cannot print them");
            std::vector<double> rows(4 * (size_t)g0 + 1);
            CK(ps_state_info(load_state.c_str(), nullptr, nullptr, rows.data(), rows.size()));
            for (int32_t j = 0; j < g0; j++) {
                avg_core[j] = rows[4 * j]; std_core[j] = rows[4 * j + 1]; avg_acc[j] = rows[4 * j + 2]; std_acc[j] = rows[4 * j + 3];
            }
        }
        CK(ps_sim_load(load_state.c_str(), &p, &sim));
        if (p.verbose) printf("Loaded %d generations from %s, running generations %d to %d\n", g0, load_state.c_str(), g0 + 1, p.n_gen);
    } else {
        CK(ps_multi_create(&p, (int)n_shards, nullptr, &multi));
        sim = ps_multi_shard(multi, 0);
    }
    if (record_capacity) CK(multi ? ps_multi_record_ancestry(multi, record_capacity) : ps_sim_record_ancestry(sim, record_capacity));
    auto run = [&](uint32_t first, uint32_t count) { return multi ? ps_multi_run(multi, first, count) : ps_sim_run(sim, first, count); };
    auto sync = [&]() { return multi ? ps_multi_sync(multi) : ps_sim_sync(sim); };
    auto distances = [&](double *c, double *a) { return multi ? ps_multi_pairwise_distances(multi, c, a) : ps_sim_pairwise_distances(sim, c, a); };

    if (p.print_selection) {                                           // main.rs:321-331
        FILE *f = open_out(outpref, "_selection.tsv");
        const double *sel = ps_sim_selection(sim);
        for (uint64_t g = 0; g < G; g++) fprintf(f, "%s%s", g ? "\n" : "", fmt(sel[g]).c_str());
        fputc('\n', f);
        fclose(f);
    }

    ps_population *acc = ps_sim_acc(sim);      // replicated on every shard
    std::vector<double> cd(P), ad(P);
    const bool stepwise = p.print_dist || p.verbose;
    auto final_outputs = [&]() {                                       // main.rs:467-499
        {
            CK(sync());
            CK(distances(cd.data(), ad.data()));
            FILE *f = open_out(outpref, ".tsv");
            write_pairs_tsv(f, cd, ad);
            fclose(f);
            std::vector<double> freqs(G + p.core_genes);
            CK(ps_gene_frequencies(acc, freqs.data()));
            f = open_out(outpref, "_freqs.txt");
            for (double x : freqs) fprintf(f, "%s\n", fmt(x).c_str());
            fclose(f);
        }
        if (present["print_core_freqs"]) {                             // (no counterpart in the reference: docs/CORE_DIVERSITY.md)
            std::vector<uint32_t> cnt(4 * (size_t)p.core_size + 1);
            std::vector<uint64_t> spec((size_t)p.pop_size + 1);
            ps_core_diversity_t dv;
            CK(multi ? ps_multi_site_allele_counts(multi, cnt.data()) : ps_site_allele_counts(ps_sim_core(sim), cnt.data()));
            CK(multi ? ps_multi_core_diversity(multi, &dv, spec.data()) : ps_core_diversity(ps_sim_core(sim), &dv, spec.data()));
            FILE *f = open_out(outpref, "_core_freqs.tsv");
            for (uint64_t s = 0; s < p.core_size; s++) fprintf(f, "%u\t%u\t%u\t%u\n", cnt[4 * s], cnt[4 * s + 1], cnt[4 * s + 2], cnt[4 * s + 3]);
            fclose(f);
            f = open_out(outpref, "_core_diversity.tsv");
            const std::pair<const char *, uint64_t> fields[] = {
                { "pop_size", dv.pop_size }, { "sites", dv.sites }, { "other_cells", dv.other_cells },
                { "segregating_sites", dv.segregating_sites }, { "pair_differences", dv.pair_differences },
                { "base_cells_A", dv.base_cells[0] }, { "base_cells_C", dv.base_cells[1] }, { "base_cells_G", dv.base_cells[2] },
                { "base_cells_T", dv.base_cells[3] } };
            for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
            fprintf(f, "mean_pairwise_distance\t%s\n", fmt(dv.mean_pairwise_distance).c_str());
            for (uint64_t m = 0; m < spec.size(); m++)
                if (spec[m]) fprintf(f, "spectrum\t%llu\t%llu\n", (unsigned long long)m, (unsigned long long)spec[m]);
            fclose(f);
        }
        if (present["print_dist_hist"]) {                              // (no counterpart in the reference: docs/DISTANCE_HISTOGRAM.md)
            std::vector<uint64_t> joint((size_t)hist_prm.core_bins * hist_prm.acc_bins);
            ps_pair_hist_t h;
            CK(multi ? ps_multi_distance_histogram(multi, &hist_prm, &h, joint.data()) : ps_sim_distance_histogram(sim, &hist_prm, &h, joint.data()));
            FILE *f = open_out(outpref, "_dist_hist.tsv");
            for (uint32_t bc = 0; bc < h.core_bins; bc++)
                for (uint32_t ba = 0; ba < h.acc_bins; ba++)
                    if (joint[(size_t)bc * h.acc_bins + ba])
                        fprintf(f, "%u\t%u\t%llu\n", bc, ba, (unsigned long long)joint[(size_t)bc * h.acc_bins + ba]);
            fclose(f);
            f = open_out(outpref, "_dist_hist_summary.tsv");
            const std::pair<const char *, uint64_t> fields[] = {
                { "pop_size", h.pop_size }, { "pairs", h.pairs }, { "core_sites", h.core_sites }, { "core_genes", h.core_genes },
                { "core_bins", h.core_bins }, { "acc_bins", h.acc_bins }, { "core_span", h.core_span },
                { "undefined_pairs", h.undefined_pairs }, { "core_clamped", h.core_clamped }, { "core_d_min", h.core_d_min },
                { "core_d_max", h.core_d_max }, { "core_d_sum", h.core_d_sum } };
            for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
            // the 128-bit square sum as one decimal number
            unsigned __int128 sq = ((unsigned __int128)h.core_d_sqsum_hi << 64) | h.core_d_sqsum_lo;
            std::string dec;
            do { dec.insert(dec.begin(), (char)('0' + (int)(sq % 10))); sq /= 10; } while (sq);
            fprintf(f, "core_d_sqsum\t%s\n", dec.c_str());
            fprintf(f, "mean_core_distance\t%s\n", fmt(h.mean_core_distance).c_str());
            fclose(f);
        }
        if (present["print_clusters"]) {                               // (no counterpart in the reference: docs/STRAIN_CLUSTERS.md)
            std::vector<uint32_t> labels((size_t)p.pop_size);
            ps_cluster_t c;
            CK(multi ? ps_multi_strain_clusters(multi, &cluster_prm, &c, labels.data()) : ps_sim_strain_clusters(sim, &cluster_prm, &c, labels.data()));
            FILE *f = open_out(outpref, "_clusters.tsv");
            for (uint64_t k = 0; k < p.pop_size; k++) fprintf(f, "%llu\t%u\n", (unsigned long long)k, labels[k]);
            fclose(f);
            f = open_out(outpref, "_clusters_summary.tsv");
            const std::pair<const char *, uint64_t> fields[] = {
                { "pop_size", c.pop_size }, { "pairs", c.pairs }, { "core_sites", c.core_sites }, { "core_genes", c.core_genes },
                { "edges", c.edges }, { "clusters", c.clusters }, { "singletons", c.singletons }, { "largest_cluster", c.largest_cluster },
                { "within_pairs", c.within_pairs }, { "undefined_pairs", c.undefined_pairs }, { "core_max_d", cluster_prm.core_max_d },
                { "acc_num", cluster_prm.acc_num }, { "acc_den", cluster_prm.acc_den } };
            for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
            fclose(f);
        }
        if (present["print_differentiation"]) {                        // (no counterpart in the reference: docs/GROUP_DIFFERENTIATION.md)
            const size_t n = (size_t)p.pop_size, M = diff_prm.max_groups, L = (size_t)p.core_size;
            std::vector<uint32_t> labels(n), group_of(n), glabel(M), gsize(M), within(std::max<size_t>(L, 1)), total(std::max<size_t>(L, 1));
            ps_cluster_t c;
            CK(multi ? ps_multi_strain_clusters(multi, &cluster_prm, &c, labels.data()) : ps_sim_strain_clusters(sim, &cluster_prm, &c, labels.data()));
            const size_t G = (size_t)(p.pan_genes - p.core_genes);
            std::vector<uint32_t> gc(std::max<size_t>(G * M, 1));
            std::vector<uint64_t> between(M * M), fixed(M * M), acc_between(M * M), gene_fixed(M * M), gene_private(M);
            ps_diff_t d;
            CK(multi ? ps_multi_group_differentiation(multi, labels.data(), &diff_prm, &d, group_of.data(), glabel.data(), gsize.data(), between.data(),
                                                      fixed.data(), within.data(), total.data(), nullptr, gc.data(), acc_between.data(),
                                                      gene_fixed.data(), gene_private.data())
                     : ps_sim_group_differentiation(sim, labels.data(), &diff_prm, &d, group_of.data(), glabel.data(), gsize.data(), between.data(),
                                                    fixed.data(), within.data(), total.data(), nullptr, gc.data(), acc_between.data(),
                                                    gene_fixed.data(), gene_private.data()));
            const size_t K = (size_t)d.groups;
            FILE *f = open_out(outpref, "_diff_groups.tsv");
            for (size_t g = 0; g < K; g++)
                fprintf(f, "%zu\t%u\t%u\t%llu\t%llu\t%llu\n", g, glabel[g], gsize[g], (unsigned long long)between[g * K + g],
                        (unsigned long long)fixed[g * K + g], (unsigned long long)gene_private[g]);
            fclose(f);
            f = open_out(outpref, "_diff_between.tsv");
            for (size_t g = 0; g < K; g++)
                for (size_t h = g + 1; h < K; h++)
                    fprintf(f, "%zu\t%zu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", g, h, (unsigned long long)gsize[g] * gsize[h],
                            (unsigned long long)between[g * K + h], (unsigned long long)fixed[g * K + h], (unsigned long long)acc_between[g * K + h],
                            (unsigned long long)gene_fixed[g * K + h], (unsigned long long)gene_fixed[h * K + g]);
            fclose(f);
            f = open_out(outpref, "_diff_sites.tsv");
            for (uint64_t s = 0; s < d.sites; s++) fprintf(f, "%u\t%u\n", within[s], total[s]);
            fclose(f);
            f = open_out(outpref, "_diff_genes.tsv");
            for (uint64_t y = 0; y < d.genes; y++)
                for (size_t g = 0; g < K; g++) fprintf(f, "%u%c", gc[y * K + g], g + 1 == K ? '\n' : '\t');
            fclose(f);
            f = open_out(outpref, "_diff_summary.tsv");
            const std::pair<const char *, uint64_t> fields[] = {
                { "pop_size", d.pop_size }, { "sites", d.sites }, { "genes", d.genes }, { "groups", d.groups }, { "assigned", d.assigned },
                { "unassigned", d.unassigned }, { "other_cells", d.other_cells }, { "within_pairs", d.within_pairs },
                { "between_pairs", d.between_pairs }, { "within_differences", d.within_differences },
                { "between_differences", d.between_differences } };
            for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
            fprintf(f, "pi_within\t%s\npi_between\t%s\nfst\t%s\n", fmt(d.pi_within).c_str(), fmt(d.pi_between).c_str(), fmt(d.fst).c_str());
            fprintf(f, "diff_max_groups\t%u\ndiff_min_size\t%u\n", diff_prm.max_groups, diff_prm.min_size);
            fclose(f);
        }
        if (present["print_tree"]) {                                   // (no counterpart in the reference: docs/LINKAGE_TREE.md)
            const size_t n = (size_t)p.pop_size;
            std::vector<uint32_t> lo(n), hi(n);
            std::vector<uint64_t> num(n), den(n);
            ps_tree_t t;
            CK(multi ? ps_multi_linkage_tree(multi, &tree_prm, &t, lo.data(), hi.data(), num.data(), den.data())
                     : ps_sim_linkage_tree(sim, &tree_prm, &t, lo.data(), hi.data(), num.data(), den.data()));
            FILE *f = open_out(outpref, "_tree.tsv");
            for (uint64_t k = 0; k < t.edges; k++)
                fprintf(f, "%u\t%u\t%llu\t%llu\t%s\n", lo[k], hi[k], (unsigned long long)num[k], (unsigned long long)den[k],
                        den[k] ? fmt((double)num[k] / (double)den[k]).c_str() : "NaN");
            fclose(f);
            f = open_out(outpref, "_tree_summary.tsv");
            const std::pair<const char *, uint64_t> fields[] = {
                { "pop_size", t.pop_size }, { "pairs", t.pairs }, { "core_sites", t.core_sites }, { "core_genes", t.core_genes },
                { "metric", t.metric }, { "edges", t.edges }, { "undefined_edges", t.undefined_edges },
                { "distinct_heights", t.distinct_heights } };
            for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
            fclose(f);
        }
        if (present["print_upgma"]) {                                  // (no counterpart in the reference: docs/UPGMA_TREE.md)
            const size_t n = (size_t)p.pop_size;
            std::vector<uint32_t> left(n), right(n), size(n);
            std::vector<uint64_t> num(n), den(n);
            ps_upgma_t t;
            CK(multi ? ps_multi_upgma_tree(multi, &upgma_prm, &t, left.data(), right.data(), size.data(), num.data(), den.data())
                     : ps_sim_upgma_tree(sim, &upgma_prm, &t, left.data(), right.data(), size.data(), num.data(), den.data()));
            FILE *f = open_out(outpref, "_upgma.tsv");
            for (uint64_t k = 0; k < t.merges; k++)
                fprintf(f, "%llu\t%u\t%u\t%u\t%llu\t%llu\t%s\n", (unsigned long long)(t.pop_size + k), left[k], right[k], size[k],
                        (unsigned long long)num[k], (unsigned long long)den[k], fmt((double)num[k] / (double)den[k]).c_str());
            fclose(f);
            uint64_t need = 0;
            CK(ps_upgma_newick(left.data(), right.data(), num.data(), den.data(), t.pop_size, nullptr, 0, &need));
            std::vector<char> text(need);
            CK(ps_upgma_newick(left.data(), right.data(), num.data(), den.data(), t.pop_size, text.data(), need, &need));
            f = open_out(outpref, "_upgma.nwk");
            fprintf(f, "%s\n", text.data());
            fclose(f);
            f = open_out(outpref, "_upgma_summary.tsv");
            const std::pair<const char *, uint64_t> fields[] = {
                { "pop_size", t.pop_size }, { "pairs", t.pairs }, { "core_sites", t.core_sites }, { "core_genes", t.core_genes },
                { "metric", t.metric }, { "merges", t.merges }, { "distinct_heights", t.distinct_heights }, { "root_num", t.root_num },
                { "root_den", t.root_den } };
            for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
            fclose(f);
        }
        if (print_knn) {                                               // (no counterpart in the reference: docs/NEAREST_NEIGHBOURS.md)
            const size_t n = (size_t)p.pop_size, k = knn_prm.k;
            std::vector<uint32_t> nbr(n * k), labels(n);
            std::vector<uint64_t> num(n * k), den(n * k);
            ps_knn_t t;
            CK(multi ? ps_multi_nearest_neighbours(multi, &knn_prm, &t, nbr.data(), num.data(), den.data())
                     : ps_sim_nearest_neighbours(sim, &knn_prm, &t, nbr.data(), num.data(), den.data()));
            FILE *f = open_out(outpref, "_knn.tsv");
            for (size_t e = 0; e < n * k; e++)
                fprintf(f, "%llu\t%llu\t%u\t%llu\t%llu\t%s\n", (unsigned long long)(e / k), (unsigned long long)(e % k + 1), nbr[e],
                        (unsigned long long)num[e], (unsigned long long)den[e], den[e] ? fmt((double)num[e] / (double)den[e]).c_str() : "NaN");
            fclose(f);
            f = open_out(outpref, "_knn_summary.tsv");
            const std::pair<const char *, uint64_t> fields[] = {
                { "pop_size", t.pop_size }, { "pairs", t.pairs }, { "core_sites", t.core_sites }, { "core_genes", t.core_genes },
                { "metric", t.metric }, { "k", t.k }, { "undefined_neighbours", t.undefined_neighbours }, { "graph_edges", t.graph_edges },
                { "mutual_edges", t.mutual_edges } };
            for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
            // the lineages at every rank; the labels of the last one (rank k) are the ones written
            for (uint32_t r = 1; r <= knn_prm.k; r++) {
                ps_lineage_t l;
                CK(ps_lineages_from_neighbours(nbr.data(), n, knn_prm.k, r, &l, labels.data()));
                fprintf(f, "lineages\t%u\t%llu\t%llu\n", r, (unsigned long long)l.lineages, (unsigned long long)l.largest_lineage);
            }
            fclose(f);
            f = open_out(outpref, "_lineages.tsv");
            for (size_t i = 0; i < n; i++) fprintf(f, "%llu\t%u\n", (unsigned long long)i, labels[i]);
            fclose(f);
        }
        if (present["print_ld"]) {                                     // (no counterpart in the reference: docs/LINKAGE_DISEQUILIBRIUM.md)
            const size_t nl = ld_prm.lag_bins, nr = ld_prm.r2_bins;
            std::vector<uint32_t> index(ld_prm.max_loci), count(ld_prm.max_loci);
            std::vector<uint64_t> hist(nl * nr), lag_sum(nl);
            ps_ld_t t;
            CK(multi ? ps_multi_locus_ld(multi, ld_metric, &ld_prm, nullptr, 0, &t, index.data(), count.data(), hist.data(), lag_sum.data())
                     : ps_sim_locus_ld(sim, ld_metric, &ld_prm, nullptr, 0, &t, index.data(), count.data(), hist.data(), lag_sum.data()));
            FILE *f = open_out(outpref, "_ld.tsv");
            for (size_t l = 0; l < nl; l++)
                for (size_t r = 0; r < nr; r++)
                    if (hist[l * nr + r]) fprintf(f, "%llu\t%llu\t%llu\n", (unsigned long long)l, (unsigned long long)r, (unsigned long long)hist[l * nr + r]);
            fclose(f);
            f = open_out(outpref, "_ld_summary.tsv");
            const std::pair<const char *, uint64_t> fields[] = {
                { "pop_size", t.pop_size }, { "metric", (uint64_t)ld_metric }, { "columns", t.columns }, { "candidates", t.candidates }, { "loci", t.loci },
                { "pairs", t.pairs }, { "defined_pairs", t.defined_pairs }, { "undefined_pairs", t.undefined_pairs },
                { "four_gamete_pairs", t.four_gamete_pairs }, { "complete_pairs", t.complete_pairs }, { "positive_pairs", t.positive_pairs },
                { "negative_pairs", t.negative_pairs }, { "sum_q", t.sum_q }, { "r2_bins", t.r2_bins }, { "lag_bins", t.lag_bins },
                { "min_minor", t.min_minor }, { "max_loci", t.max_loci } };
            for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
            fprintf(f, "mean_r2\t%s\n", fmt(t.mean_r2).c_str());
            for (size_t l = 0; l < nl; l++) {
                uint64_t n = 0;
                for (size_t r = 0; r < nr; r++) n += hist[l * nr + r];
                if (n) fprintf(f, "lag\t%llu\t%llu\t%llu\n", (unsigned long long)l, (unsigned long long)n, (unsigned long long)lag_sum[l]);
            }
            fclose(f);
            f = open_out(outpref, "_ld_loci.tsv");
            for (uint64_t k = 0; k < t.loci; k++) fprintf(f, "%u\t%u\n", index[k], count[k]);
            fclose(f);
        }
        if (record_capacity) {                                         // (no counterpart in the reference: docs/GENEALOGY.md)
            const size_t n = (size_t)p.pop_size;
            std::vector<uint32_t> order(n), coal(n);
            ps_genealogy_t g;
            CK(multi ? ps_multi_genealogy(multi, &g, order.data(), coal.data()) : ps_sim_genealogy(sim, &g, order.data(), coal.data()));
            FILE *f = open_out(outpref, "_genealogy.tsv");
            for (size_t r = 0; r < n; r++) {
                if (r + 1 == n) fprintf(f, "%llu\t%u\t\n", (unsigned long long)r, order[r]);
                else if (coal[r] == PS_GEN_BEYOND) fprintf(f, "%llu\t%u\tbeyond\n", (unsigned long long)r, order[r]);
                else fprintf(f, "%llu\t%u\t%u\n", (unsigned long long)r, order[r], coal[r]);
            }
            fclose(f);
            uint64_t need = 0;
            CK(ps_genealogy_newick(order.data(), coal.data(), n, nullptr, 0, &need));
            std::vector<char> text(need);
            CK(ps_genealogy_newick(order.data(), coal.data(), n, text.data(), need, &need));
            f = open_out(outpref, "_genealogy.nwk");
            fputs(text.data(), f);
            fclose(f);
            // (a run that recorded no generation -- a loaded state already at --n_gen -- has no divergence times to bin)
            if (g.depth == 0) fprintf(stderr, "pansim: no generation was recorded: %s_clock.tsv and %s_clock_summary.tsv are not written\n", outpref.c_str(), outpref.c_str());
            else {
                const size_t nt = (size_t)clock_prm.time_bins + 1, bx = clock_prm.dist_bins;
                std::vector<uint64_t> joint(nt * bx), per_time(3 * nt);
                ps_clock_t c;
                CK(multi ? ps_multi_clock_histogram(multi, &clock_prm, &c, joint.data(), per_time.data())
                         : ps_sim_clock_histogram(sim, &clock_prm, &c, joint.data(), per_time.data()));
                f = open_out(outpref, "_clock.tsv");
                for (size_t t = 0; t < nt; t++)
                    for (size_t x = 0; x < bx; x++)
                        if (joint[t * bx + x]) fprintf(f, "%llu\t%llu\t%llu\n", (unsigned long long)t, (unsigned long long)x, (unsigned long long)joint[t * bx + x]);
                fclose(f);
                f = open_out(outpref, "_clock_summary.tsv");
                const std::pair<const char *, uint64_t> fields[] = {
                    { "pop_size", c.pop_size }, { "pairs", c.pairs }, { "core_sites", c.core_sites }, { "core_genes", c.core_genes },
                    { "metric", c.metric }, { "time_bins", c.time_bins }, { "dist_bins", c.dist_bins }, { "time_span", c.time_span },
                    { "core_span", c.core_span }, { "generation", g.generation }, { "capacity", g.capacity }, { "depth", c.depth },
                    { "roots", g.roots }, { "tmrca", g.tmrca }, { "undefined_pairs", c.undefined_pairs }, { "core_clamped", c.core_clamped },
                    { "beyond_pairs", c.beyond_pairs }, { "binned_pairs", c.binned_pairs }, { "num_sum", c.num_sum }, { "den_sum", c.den_sum } };
                for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
                for (size_t t = 0; t < nt; t++)
                    if (per_time[3 * t])
                        fprintf(f, "time\t%llu\t%llu\t%llu\t%llu\n", (unsigned long long)t, (unsigned long long)per_time[3 * t],
                                (unsigned long long)per_time[3 * t + 1], (unsigned long long)per_time[3 * t + 2]);
                fclose(f);
            }
        }
        // one of the three trees as a merge list (left, right: room for pop_size values); vals (may be null): the values
        // --print_tree_compare reads it with -- the dense ranks of its heights, the coalescence times of the genealogy
        auto merge_list = [&](const std::string &source, uint32_t *left, uint32_t *right, uint32_t *vals, uint64_t *M) -> int {
            const size_t n = (size_t)p.pop_size;
            if (source == "upgma") {
                std::vector<uint32_t> size(n);
                std::vector<uint64_t> num(n), den(n);
                ps_upgma_t t;
                CK(multi ? ps_multi_upgma_tree(multi, &upgma_prm, &t, left, right, size.data(), num.data(), den.data())
                         : ps_sim_upgma_tree(sim, &upgma_prm, &t, left, right, size.data(), num.data(), den.data()));
                *M = t.merges;
                if (vals) CK(ps_levels_from_heights(num.data(), den.data(), *M, vals, nullptr));
            } else if (source == "tree") {
                std::vector<uint32_t> lo(n), hi(n);
                std::vector<uint64_t> num(n), den(n);
                ps_tree_t t;
                CK(multi ? ps_multi_linkage_tree(multi, &tree_prm, &t, lo.data(), hi.data(), num.data(), den.data())
                         : ps_sim_linkage_tree(sim, &tree_prm, &t, lo.data(), hi.data(), num.data(), den.data()));
                CK(ps_merges_from_tree(lo.data(), hi.data(), t.edges, n, left, right, M));
                if (vals) CK(ps_levels_from_heights(num.data(), den.data(), *M, vals, nullptr));
            } else {
                std::vector<uint32_t> order(n), coal(n);
                ps_genealogy_t g;
                CK(multi ? ps_multi_genealogy(multi, &g, order.data(), coal.data()) : ps_sim_genealogy(sim, &g, order.data(), coal.data()));
                CK(ps_merges_from_genealogy(order.data(), coal.data(), n, left, right, vals, M));
            }
            return 0;
        };
        if (!pars_source.empty()) {                                    // (no counterpart in the reference: docs/TREE_PARSIMONY.md)
            const size_t n = (size_t)p.pop_size, L = (size_t)p.core_size, G = (size_t)(p.pan_genes - p.core_genes);
            std::vector<uint32_t> left(n), right(n);
            uint64_t M = 0;
            CK(merge_list(pars_source, left.data(), right.data(), nullptr, &M));
            if (M == 0) fprintf(stderr, "pansim: the %s of --print_parsimony has no merge: the _parsimony files are not written\n", pars_source.c_str());
            else {
                const size_t nodes = n + (size_t)M;
                std::vector<uint32_t> sites(std::max<size_t>(L, 1)), gch(std::max<size_t>(G, 1)), ggn(std::max<size_t>(G, 1)), gls(std::max<size_t>(G, 1));
                std::vector<uint64_t> hist(PS_PARS_BINS), bch(nodes), bgn(nodes), bls(nodes);
                ps_parsimony_t t;
                CK(multi ? ps_multi_tree_parsimony(multi, left.data(), right.data(), M, &t, sites.data(), hist.data(), bch.data(), gch.data(), ggn.data(),
                                                   gls.data(), bgn.data(), bls.data())
                         : ps_sim_tree_parsimony(sim, left.data(), right.data(), M, &t, sites.data(), hist.data(), bch.data(), gch.data(), ggn.data(),
                                                 gls.data(), bgn.data(), bls.data()));
                FILE *f = open_out(outpref, "_parsimony_sites.tsv");
                for (uint64_t s = 0; s < t.sites; s++) fprintf(f, "%u\n", sites[s]);
                fclose(f);
                f = open_out(outpref, "_parsimony_genes.tsv");
                for (uint64_t y = 0; y < t.genes; y++) fprintf(f, "%u\t%u\t%u\n", gch[y], ggn[y], gls[y]);
                fclose(f);
                std::vector<long long> parent(nodes, -1);
                for (uint64_t k = 0; k < M; k++) parent[left[k]] = parent[right[k]] = (long long)(n + k);
                f = open_out(outpref, "_parsimony_branches.tsv");
                for (size_t x = 0; x < nodes; x++)
                    fprintf(f, "%zu\t%lld\t%llu\t%llu\t%llu\n", x, parent[x], (unsigned long long)bch[x], (unsigned long long)bgn[x], (unsigned long long)bls[x]);
                fclose(f);
                // Newick, one line per root: an explicit stack (a caterpillar is pop_size deep); text entries are negative
                f = open_out(outpref, "_parsimony.nwk");
                auto tail = [&](size_t x) { return parent[x] >= 0 ? ":" + fmt(t.sites ? (double)bch[x] / (double)t.sites : 0.0) : std::string(); };
                for (size_t root = n; root < nodes; root++) {
                    if (parent[root] >= 0) continue;
                    std::vector<long long> stack{ (long long)root };
                    while (!stack.empty()) {
                        const long long e = stack.back();
                        stack.pop_back();
                        if (e == -1) fputs(",", f);
                        else if (e < -1) fprintf(f, ")%s", tail((size_t)(-e - 2)).c_str());
                        else if ((size_t)e < n) fprintf(f, "%lld%s", e, tail((size_t)e).c_str());
                        else {
                            fputs("(", f);
                            stack.insert(stack.end(), { -e - 2, (long long)right[(size_t)e - n], -1, (long long)left[(size_t)e - n] });
                        }
                    }
                    fputs(";\n", f);
                }
                fclose(f);
                f = open_out(outpref, "_parsimony_summary.tsv");
                const std::pair<const char *, uint64_t> fields[] = {
                    { "pop_size", t.pop_size }, { "sites", t.sites }, { "genes", t.genes }, { "merges", t.merges }, { "trees", t.trees },
                    { "covered_leaves", t.covered_leaves }, { "spanning", t.spanning }, { "total_changes", t.total_changes },
                    { "changed_sites", t.changed_sites }, { "max_changes", t.max_changes }, { "gene_total_changes", t.gene_total_changes },
                    { "gene_total_gains", t.gene_total_gains }, { "gene_total_losses", t.gene_total_losses }, { "min_changes", t.min_changes },
                    { "excess_changes", t.excess_changes }, { "homoplasic_sites", t.homoplasic_sites } };
                for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
                fprintf(f, "ci\t%s\ntree\t%s\n", fmt(t.ci).c_str(), pars_source.c_str());
                fclose(f);
            }
        }
        if (!tcmp_source[0].empty()) {                                 // (no counterpart in the reference: docs/TREE_COMPARISON.md)
            const size_t n = (size_t)p.pop_size;
            std::vector<uint32_t> left[2], right[2], vals[2];
            uint64_t M[2] = { 0, 0 };
            for (int x = 0; x < 2; x++) {
                left[x].resize(n);
                right[x].resize(n);
                vals[x].resize(n);
                CK(merge_list(tcmp_source[x], left[x].data(), right[x].data(), vals[x].data(), &M[x]));
            }
            if (M[0] == 0 || M[1] == 0)
                fprintf(stderr, "pansim: the %s of --print_tree_compare has no merge: the _tree_compare files are not written\n",
                        tcmp_source[M[0] == 0 ? 0 : 1].c_str());
            else {
                const size_t na = (size_t)tcmp_prm.bins_a + 1, nb = (size_t)tcmp_prm.bins_b + 1;
                std::vector<uint64_t> joint(na * nb);
                std::vector<uint8_t> in_other[2] = { std::vector<uint8_t>(M[0]), std::vector<uint8_t>(M[1]) };
                ps_tree_compare_t t;
                CK(multi ? ps_multi_tree_compare(multi, left[0].data(), right[0].data(), vals[0].data(), M[0], left[1].data(), right[1].data(),
                                                 vals[1].data(), M[1], &tcmp_prm, &t, joint.data(), in_other[0].data(), in_other[1].data())
                         : ps_sim_tree_compare(sim, left[0].data(), right[0].data(), vals[0].data(), M[0], left[1].data(), right[1].data(),
                                               vals[1].data(), M[1], &tcmp_prm, &t, joint.data(), in_other[0].data(), in_other[1].data()));
                FILE *f = open_out(outpref, "_tree_compare.tsv");
                for (size_t a = 0; a < na; a++)
                    for (size_t b = 0; b < nb; b++)
                        if (joint[a * nb + b]) fprintf(f, "%zu\t%zu\t%llu\n", a, b, (unsigned long long)joint[a * nb + b]);
                fclose(f);
                // the clades: the merges whose parent carries another value (or that have none), with the leaves below them
                f = open_out(outpref, "_tree_compare_clades.tsv");
                for (int x = 0; x < 2; x++) {
                    std::vector<long long> parent(M[x], -1);
                    std::vector<uint32_t> size(M[x]);
                    for (uint64_t k = 0; k < M[x]; k++) {
                        size[k] = 0;
                        for (uint32_t c : { left[x][k], right[x][k] }) {
                            size[k] += c < n ? 1u : size[c - n];
                            if (c >= n) parent[c - n] = (long long)k;
                        }
                    }
                    for (uint64_t k = 0; k < M[x]; k++)
                        if (parent[k] < 0 || vals[x][(size_t)parent[k]] != vals[x][k])
                            fprintf(f, "%s\t%llu\t%u\t%u\t%u\n", tcmp_source[x].c_str(), (unsigned long long)(n + k), size[k], vals[x][k], (unsigned)in_other[x][k]);
                }
                fclose(f);
                f = open_out(outpref, "_tree_compare_summary.tsv");
                const std::pair<const char *, uint64_t> fields[] = {
                    { "pop_size", t.pop_size }, { "merges_a", t.merges_a }, { "merges_b", t.merges_b }, { "pairs", t.pairs },
                    { "joined_both", t.joined_both }, { "joined_a_only", t.joined_a_only }, { "joined_b_only", t.joined_b_only },
                    { "joined_neither", t.joined_neither }, { "sum_a", t.sum_a }, { "sum_b", t.sum_b }, { "sum_aa", t.sum_aa }, { "sum_bb", t.sum_bb },
                    { "sum_ab", t.sum_ab }, { "triples", t.triples }, { "resolved_a", t.resolved_a }, { "resolved_b", t.resolved_b },
                    { "shared_triplets", t.shared_triplets }, { "clades_a", t.clades_a }, { "clades_b", t.clades_b }, { "shared_clades", t.shared_clades },
                    { "rf_distance", t.rf_distance }, { "bins_a", t.bins_a }, { "bins_b", t.bins_b }, { "span_a", t.span_a }, { "span_b", t.span_b } };
                for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
                const std::pair<const char *, double> doubles[] = {
                    { "cophenetic_r", t.cophenetic_r }, { "triplet_recall", t.triplet_recall }, { "triplet_precision", t.triplet_precision },
                    { "clade_recall", t.clade_recall }, { "clade_precision", t.clade_precision } };
                for (const auto &x : doubles) fprintf(f, "%s\t%s\n", x.first, fmt(x.second).c_str());
                fprintf(f, "a\t%s\nb\t%s\n", tcmp_source[0].c_str(), tcmp_source[1].c_str());
                fclose(f);
            }
        }
    };
    if (!stepwise && p.n_gen > g0) CK(run((uint32_t)g0, (uint32_t)(p.n_gen - g0)));      // main.rs:429-464
    if (g0 > 0 && g0 == p.n_gen) final_outputs();                       // (a loaded state that is already at --n_gen)
    for (int32_t j = g0; j < p.n_gen; j++) {
        if (stepwise) CK(run((uint32_t)j, 1));
        if (j == p.n_gen - 1) final_outputs();
        if (p.print_dist) {                                            // main.rs:502-519
            CK(sync());
            CK(distances(cd.data(), ad.data()));
            CK(ps_standard_deviation(cd.data(), P, &std_core[j], &avg_core[j]));
            CK(ps_standard_deviation(ad.data(), P, &std_acc[j], &avg_acc[j]));
        }
        if (p.verbose) {                                               // main.rs:522-526
            printf("Finished gen: %d\n", j + 1);
            double gf = 0.0;
            CK(sync());
            CK(ps_calc_gene_freq(acc, &gf));
            printf("avg_gene_freq: %s\n", fmt(gf).c_str());
        }
    }
    if (p.print_dist) {                                                // main.rs:531-548
        FILE *f = open_out(outpref, "_per_gen.tsv");
        for (int32_t j = 0; j < p.n_gen; j++)
            fprintf(f, "%s\t%s\t%s\t%s\n", fmt(avg_core[j]).c_str(), fmt(std_core[j]).c_str(),
                    fmt(avg_acc[j]).c_str(), fmt(std_acc[j]).c_str());
        fclose(f);
    }
    if (p.print_matrices) {                                            // main.rs:550-553 (errors ignored)
        if (multi) (void)ps_multi_write(multi, outpref.c_str());
        else if (ps_write(ps_sim_core(sim), outpref.c_str()) == PS_OK) (void)ps_write(acc, outpref.c_str());
    }
    if (!save_state.empty()) {
        // the rows of _per_gen.tsv travel with the state, so that a continuation with --print_dist prints all of them
        std::vector<double> rows;
        for (int32_t j = 0; p.print_dist && j < p.n_gen; j++) rows.insert(rows.end(), { avg_core[j], std_core[j], avg_acc[j], std_acc[j] });
        rows.push_back(0.0);                                           // (never an empty vector's null pointer)
        CK(ps_sim_save(sim, save_state.c_str(), p.print_dist ? rows.data() : nullptr));
    }
    if (multi) ps_multi_destroy(multi);
    else ps_sim_destroy(sim);
    return 0;
}
