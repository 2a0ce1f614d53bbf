// pansim_cli.cpp -- the `pansim` executable: the reference's command line
// (pansim/src/main.rs:17-152), validation (:195-247), generation loop (:429-528) and
// output files (:321-331, :467-499, :531-553) driving libpansim_hip.so through its C ABI.
// The read-outs the reference does not have are in cli_readouts.h.
#include <thread>

#include "cli_readouts.h"

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

static uint64_t as_u64(const Vals &v, const char *name)
{
    const std::string &s = v.at(name);
    char *end = nullptr;
    const unsigned long long x = strtoull(s.c_str(), &end, 10);
    if (s.empty() || s[0] == '-' || *end != 0) die(101, "error: Invalid value \"" + s + "\" for '--" + name + "': invalid digit found in string");
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

// every flag, the reference's and the extensions'
template <class F> static void each_flag(F fn)
{
    for (const Flag &f : FLAGS) fn(f);
    for (const Flag &f : EXT_FLAGS) fn(f);
}

// the command line as clap reads it (main.rs:17-152): the value of every flag, its default where it is not given
static void parse_args(int argc, char **argv, Vals &val, Switches &present)
{
    each_flag([&](const Flag &f) { if (f.takes_value) val[f.name] = f.def; else present[f.name] = false; });
    auto unexpected = [](const std::string &a) {
        die(2, "error: Found argument '" + a + "' which wasn't expected, or isn't valid in this context\n\nUSAGE:\n    pansim [OPTIONS]\n\nFor more information try --help");
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "-h" || a == "--help") { print_help(false); exit(0); }
        if (a == "--help-extensions") { print_help(true); exit(0); }
        if (a == "-V" || a == "--version") { printf("pansim 0.1.0\n"); exit(0); }
        if (a.rfind("--", 0) != 0) unexpected(a);
        std::string name = a.substr(2), value;
        bool has_eq = false;
        const size_t eq = name.find('=');
        if (eq != std::string::npos) { value = name.substr(eq + 1); name = name.substr(0, eq); has_eq = true; }
        const Flag *fl = nullptr;
        each_flag([&](const Flag &f) { if (name == f.name) fl = &f; });
        if (!fl) unexpected("--" + name);
        if (!fl->takes_value) {
            if (has_eq) die(2, "error: The argument '--" + name + "' takes no value");
            present[name] = true;
            continue;
        }
        if (!has_eq) {
            auto no_value = [&]() { die(2, "error: The argument '--" + name + " <" + name + ">' requires a value but none was supplied"); };
            if (i + 1 >= argc) no_value();
            value = argv[++i];
            // only prop_positive allows a leading hyphen (main.rs:91)
            if (value.rfind("-", 0) == 0 && name != "prop_positive" && value.size() > 1 && !(value[1] >= '0' && value[1] <= '9') && value[1] != '.') no_value();
        }
        val[name] = value;
    }
}

// main.rs:155-186: the reference's flags as parameters, parsed in its order
static ps_sim_params read_params(Vals &val, Switches &present)
{
    ps_sim_params p;
    ps_sim_default_params(&p);
    p.pop_size = round_usize(as_f64(val, "pop_size"));                 // main.rs:155-156
    p.core_size = round_usize(as_f64(val, "core_size"));
    p.pan_genes = round_usize(as_f64(val, "pan_genes"));
    p.core_genes = round_usize(as_f64(val, "core_genes"));
    p.avg_gene_freq = as_f64(val, "avg_gene_freq");
    p.HR_rate = as_f64(val, "HR_rate");
    p.HGT_rate = as_f64(val, "HGT_rate");
    const double r = std::round(as_f64(val, "n_gen"));                 // `as i32` saturates
    p.n_gen = r >= 2147483647.0 ? 2147483647 : r <= -2147483648.0 ? INT32_MIN : (int32_t)r;
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
    return p;
}

// main.rs:467-499: the reference's two files of the final population, then the read-outs of cli_readouts.h
static void final_outputs(const Run &run, const Options &o, uint64_t G, std::vector<double> &cd, std::vector<double> &ad)
{
    CK(run.call(ps_multi_sync, ps_sim_sync));
    CK(run.call(ps_multi_pairwise_distances, ps_sim_pairwise_distances, cd.data(), ad.data()));
    Out pairs(run, ".tsv");
    write_pairs_tsv(pairs, cd, ad);
    std::vector<double> freqs(G + run.p.core_genes);
    CK(ps_gene_frequencies(ps_sim_acc(run.sim), freqs.data()));
    Out freqs_txt(run, "_freqs.txt");
    for (double x : freqs) fprintf(freqs_txt, "%s\n", fmt(x).c_str());
    if (o.core_freqs) write_core_freqs(run);
    if (o.hist.on) write_hist(run, o);
    if (o.clusters.on) write_clusters(run, o);
    if (o.diff.on) write_differentiation(run, o);
    if (o.tree.on) write_tree(run, o);
    if (o.upgma.on) write_upgma(run, o);
    if (o.knn.k) write_knn(run, o);
    if (o.ld.on) write_ld(run, o);
    if (o.record_capacity) write_genealogy(run, o);
    if (!o.pars_source.empty()) write_parsimony(run, o);
    if (!o.tcmp_source[0].empty()) write_tree_compare(run, o);
}

int main(int argc, char **argv)
{
    Vals val;
    Switches present;
    parse_args(argc, argv, val, present);
    const ps_sim_params p = read_params(val, present);
    const std::string outpref = val["outpref"];

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
    // the flags of the read-outs, before any device work; their order decides the message when two of them are wrong
    Options o = {};
    o.core_freqs = present["print_core_freqs"];
    parse_hist(val, present, p, o);
    parse_clusters(val, present, p, o);
    parse_differentiation(val, present, p, o);
    parse_tree(val, present, o);
    parse_upgma(val, present, p, o);
    parse_knn(val, p, o);
    parse_clock(val, o);
    parse_ld(val, present, o);
    parse_parsimony(val, p, o);
    parse_tree_compare(val, p, o);
    parse_genealogy(val, o);

    const uint64_t G = d.pan_size, P = p.max_distances;
    // the rows of _per_gen.tsv: avg_core, std_core, avg_acc, std_acc per generation (and one value more: never an empty vector)
    std::vector<double> per_gen(4 * (size_t)p.n_gen + 1);
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
            CK(ps_state_info(load_state.c_str(), nullptr, nullptr, per_gen.data(), 4 * (size_t)g0 + 1));
        }
        CK(ps_sim_load(load_state.c_str(), &p, &sim));
        if (p.verbose) printf("Loaded %d generations from %s, running generations %d to %d\n", g0, load_state.c_str(), g0 + 1, p.n_gen);
    } else {
        CK(ps_multi_create(&p, (int)n_shards, nullptr, &multi));
        sim = ps_multi_shard(multi, 0);
    }
    const Run run = { multi, sim, p, outpref };
    if (o.record_capacity) CK(run.call(ps_multi_record_ancestry, ps_sim_record_ancestry, o.record_capacity));

    if (p.print_selection) {                                           // main.rs:321-331
        Out f(run, "_selection.tsv");
        const double *sel = ps_sim_selection(sim);
        for (uint64_t g = 0; g < G; g++) fprintf(f, "%s%s", g ? "\n" : "", fmt(sel[g]).c_str());
        fputc('\n', f);
    }

    ps_population *acc = ps_sim_acc(sim);      // replicated on every shard
    std::vector<double> cd(P), ad(P);
    const bool stepwise = p.print_dist || p.verbose;
    if (!stepwise && p.n_gen > g0) CK(run.call(ps_multi_run, ps_sim_run, (uint32_t)g0, (uint32_t)(p.n_gen - g0)));      // main.rs:429-464
    if (g0 > 0 && g0 == p.n_gen) final_outputs(run, o, G, cd, ad);     // (a loaded state that is already at --n_gen)
    for (int32_t j = g0; j < p.n_gen; j++) {
        if (stepwise) CK(run.call(ps_multi_run, ps_sim_run, (uint32_t)j, 1));
        if (j == p.n_gen - 1) final_outputs(run, o, G, cd, ad);
        if (p.print_dist) {                                            // main.rs:502-519
            CK(run.call(ps_multi_sync, ps_sim_sync));
            CK(run.call(ps_multi_pairwise_distances, ps_sim_pairwise_distances, cd.data(), ad.data()));
            CK(ps_standard_deviation(cd.data(), P, &per_gen[4 * j + 1], &per_gen[4 * j]));
            CK(ps_standard_deviation(ad.data(), P, &per_gen[4 * j + 3], &per_gen[4 * j + 2]));
        }
        if (p.verbose) {                                               // main.rs:522-526
            printf("Finished gen: %d\n", j + 1);
            double gf = 0.0;
            CK(run.call(ps_multi_sync, ps_sim_sync));
            CK(ps_calc_gene_freq(acc, &gf));
            printf("avg_gene_freq: %s\n", fmt(gf).c_str());
        }
    }
    if (p.print_dist) {                                                // main.rs:531-548
        Out f(run, "_per_gen.tsv");
        for (int32_t j = 0; j < p.n_gen; j++)
            fprintf(f, "%s\t%s\t%s\t%s\n", fmt(per_gen[4 * j]).c_str(), fmt(per_gen[4 * j + 1]).c_str(), fmt(per_gen[4 * j + 2]).c_str(),
                    fmt(per_gen[4 * j + 3]).c_str());
    }
    if (p.print_matrices) {                                            // main.rs:550-553 (errors ignored)
        if (multi) (void)ps_multi_write(multi, outpref.c_str());
        else if (ps_write(ps_sim_core(sim), outpref.c_str()) == PS_OK) (void)ps_write(acc, outpref.c_str());
    }
    // the rows of _per_gen.tsv travel with the state, so that a continuation with --print_dist prints all of them
    if (!save_state.empty()) CK(ps_sim_save(sim, save_state.c_str(), p.print_dist ? per_gen.data() : nullptr));
    if (multi) ps_multi_destroy(multi);
    else ps_sim_destroy(sim);
    return 0;
}
