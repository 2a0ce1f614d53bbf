// cli_readouts.h -- the read-outs of the `pansim` executable that the reference does not have (--help-extensions), each
// written once for the sharded run (ps_multi) and the loaded one (ps_sim): per read-out one parse_X, its flags checked before
// any device work in the order main calls them, and one write_X, its files.  Part of pansim_cli.cpp, which alone includes it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../include/pansim_hip.h"

using Vals = std::map<std::string, std::string>;        // the value of every flag that takes one
using Switches = std::map<std::string, bool>;           // whether a flag without a value was given

[[noreturn]] static void die(int code, const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); exit(code); }
static void CK(int rc) { if (rc != PS_OK) die(101, std::string("pansim: ") + ps_last_error()); }

// value_of_t::<f64>(..).unwrap() (main.rs:155-186): a value that does not parse panics (exit 101)
static double as_f64(const Vals &v, const char *name)
{
    const std::string &s = v.at(name);
    char *end = nullptr;
    const double x = strtod(s.c_str(), &end);
    if (s.empty() || *end != 0) die(101, "error: Invalid value \"" + s + "\" for '--" + name + "': invalid float literal");
    return x;
}

static std::string fmt(double v) { char buf[512]; ps_fmt_f64(v, buf, sizeof buf); return buf; }

// the value of a --<name>_metric flag: core (0) or acc (1), the constants of every metric of include/pansim_hip.h
static int32_t metric_flag(Vals &val, const char *name)
{
    const std::string &v = val[name];
    if (v != "core" && v != "acc") die(101, std::string("pansim: --") + name + " must be core or acc, not \"" + v + "\"");
    return v == "acc" ? 1 : 0;
}
static_assert(PS_TREE_CORE == 0 && PS_TREE_ACC == 1 && PS_KNN_CORE == 0 && PS_KNN_ACC == 1 && PS_LD_CORE == 0 && PS_LD_ACC == 1, "metric_flag");

// the value of --<name> as one whole number in [lo, hi]; `words` is what the flag's message says it must be
static unsigned long long whole_flag(Vals &val, const char *name, const char *words = "a whole number", unsigned long long lo = 0,
                                     unsigned long long hi = ~0ull)
{
    const std::string &t = val[name];
    unsigned long long v = 0;
    int used = 0;
    if (sscanf(t.c_str(), "%llu%n", &v, &used) != 1 || (size_t)used != t.size() || t.find_first_of("+- ") != std::string::npos || v < lo || v > hi)
        die(101, std::string("pansim: --") + name + " must be " + words + ", not \"" + t + "\"");
    return v;
}

// the value of --<name> as <a>,<b> bins: both at least 1, a <= max_a, b <= max_b and (a + more_a) x (b + more_b) <= 16384, the room
// of a joint histogram.  `axes` is how the flag's message names the two, `limits` how it words the last three.
static void bins_flag(Vals &val, const char *name, const char *axes, unsigned long long max_a, unsigned long long max_b, unsigned more_a,
                      unsigned more_b, const char *limits, uint32_t *bins_a, uint32_t *bins_b)
{
    const std::string &t = val[name];
    unsigned long long a = 0, b = 0;
    int used = 0;
    if (sscanf(t.c_str(), "%llu,%llu%n", &a, &b, &used) != 2 || (size_t)used != t.size() || t.find_first_of("+- ") != std::string::npos)
        die(101, std::string("pansim: --") + name + " must be " + axes + " (two whole numbers), not \"" + t + "\"");
    if (a < 1 || b < 1) die(101, std::string("pansim: --") + name + " must be at least 1 on both axes");
    if (a > max_a || b > max_b || (a + more_a) * (b + more_b) > 16384) die(101, std::string("pansim: --") + name + " " + t + ": " + limits);
    *bins_a = (uint32_t)a;
    *bins_b = (uint32_t)b;
}

// a fresh run goes through ps_multi (one shard: the plain run); a LOADED run is a plain ps_sim, driven by the ps_sim_*
// calls ps_multi itself makes for one shard
struct Run {
    ps_multi *multi;
    ps_sim *sim;
    ps_sim_params p;
    std::string outpref;
    // an entry the library has for both: its ps_multi_ and ps_sim_ forms with the arguments behind the handle
    template <class FM, class FS, class... A> int call(FM fm, FS fs, A... args) const { return multi ? fm(multi, args...) : fs(sim, args...); }
};

// the output file <outpref><suffix>, created or cut to nothing; closed where its scope ends
struct Out {
    FILE *f;
    Out(const Run &run, const char *suffix) : f(fopen((run.outpref + suffix).c_str(), "w")) { if (!f) die(1, "Error: cannot create " + run.outpref + suffix); }
    Out(const Out &) = delete;
    ~Out() { fclose(f); }
    operator FILE *() const { return f; }
};

// "<name>\t<value>" per line: the integers of a summary
static void write_fields(FILE *f, std::initializer_list<std::pair<const char *, uint64_t>> fields)
{
    for (const auto &x : fields) fprintf(f, "%s\t%llu\n", x.first, (unsigned long long)x.second);
}

// <outpref><suffix> with "<row>\t<col>\t<count>" per non-empty bin of a rows x cols histogram
static void write_bins(const Run &run, const char *suffix, const std::vector<uint64_t> &counts, size_t rows, size_t cols)
{
    Out out(run, suffix);
    for (size_t r = 0; r < rows; r++)
        for (size_t c = 0; c < cols; c++)
            if (counts[r * cols + c]) fprintf(out, "%zu\t%zu\t%llu\n", r, c, (unsigned long long)counts[r * cols + c]);
}

// <outpref><suffix> with the text of a ps_*_newick entry and `end`; fetch(text, capacity, &need) is called twice: for the size, then the text
template <class F> static void write_newick(const Run &run, const char *suffix, const char *end, F fetch)
{
    uint64_t need = 0;
    CK(fetch(nullptr, 0, &need));
    std::vector<char> text(need);
    CK(fetch(text.data(), need, &need));
    Out out(run, suffix);
    fprintf(out, "%s%s", text.data(), end);
}

// the parent of every node of a merge list over n leaves (merge k is node n + k), -1 for a root
static std::vector<long long> merge_parents(const uint32_t *left, const uint32_t *right, uint64_t M, size_t n)
{
    std::vector<long long> parent(n + (size_t)M, -1);
    for (uint64_t k = 0; k < M; k++) parent[left[k]] = parent[right[k]] = (long long)(n + k);
    return parent;
}

// the strain clusters of --cluster_core_max / --cluster_acc_max: the label of every individual
static std::vector<uint32_t> strain_labels(const Run &run, const ps_cluster_params &prm, ps_cluster_t *c)
{
    std::vector<uint32_t> labels((size_t)run.p.pop_size);
    CK(run.call(ps_multi_strain_clusters, ps_sim_strain_clusters, &prm, c, labels.data()));
    return labels;
}

// "<num / den>", NaN for an undefined distance
static std::string ratio(uint64_t num, uint64_t den) { return den ? fmt((double)num / (double)den) : "NaN"; }

// what the flags of every read-out ask for; `on`: its --print_ flag was given
struct Options {
    bool core_freqs;
    struct { bool on; ps_pair_hist_params prm; } hist;
    struct { bool on; ps_cluster_params prm; } clusters;
    struct { bool on; ps_diff_params prm; } diff;
    struct { bool on; ps_tree_params prm; } tree, upgma;
    ps_knn_params knn;                     // k 0: not asked for
    ps_clock_params clock;
    struct { bool on; int32_t metric; ps_ld_params prm; } ld;
    std::string pars_source;               // empty: not asked for
    std::string tcmp_source[2];
    ps_tree_compare_params tcmp;
    uint32_t record_capacity;              // of --print_genealogy; 0: not asked for
};

static void parse_hist(Vals &val, Switches &present, const ps_sim_params &p, Options &o)   // --print_dist_hist: its flags are checked whether or not it is given
{
    o.hist = { present["print_dist_hist"], { 64, 64, 0 } };
    bins_flag(val, "dist_hist_bins", "<core>,<accessory>", 16384, 16384, 0, 0, "the product of the two must be at most 16384", &o.hist.prm.core_bins,
              &o.hist.prm.acc_bins);
    if (!val["dist_hist_core_max"].empty()) {
        const double cm = as_f64(val, "dist_hist_core_max");
        if (!(cm > 0.0) || !std::isfinite(cm)) die(101, "pansim: --dist_hist_core_max must be > 0.0");
        const double span = std::ceil(cm * (double)p.core_size);      // core_span = max(1, ceil(core_max * L))
        o.hist.prm.core_span = span >= 18446744073709551615.0 ? UINT64_MAX : std::max<uint64_t>(1, (uint64_t)span);
    }
}

static void parse_clusters(Vals &val, Switches &present, const ps_sim_params &p, Options &o)   // --print_clusters: as parse_hist; the integers of docs/STRAIN_CLUSTERS.md
{
    ps_cluster_params &prm = o.clusters.prm = { UINT64_MAX, 0, 0 };
    o.clusters.on = present["print_clusters"];
    if (!val["cluster_core_max"].empty()) {
        const double cm = as_f64(val, "cluster_core_max");
        if (!(cm >= 0.0) || !std::isfinite(cm)) die(101, "pansim: --cluster_core_max must be >= 0.0");
        const double dmax = std::floor(cm * (double)p.core_size);      // core_max_d = floor(core_max * L)
        prm.core_max_d = dmax >= 18446744073709551615.0 ? UINT64_MAX - 1 : (uint64_t)dmax;
    }
    if (!val["cluster_acc_max"].empty()) {
        const double am = as_f64(val, "cluster_acc_max");
        if (!(am >= 0.0 && am <= 1.0)) die(101, "pansim: --cluster_acc_max must be 0.0 <= X <= 1.0");
        prm.acc_den = 1u << 20;                                         // acc_num / acc_den = floor(acc_max * 2^20) / 2^20
        prm.acc_num = (uint32_t)std::floor(am * (double)prm.acc_den);
    }
    if (o.clusters.on && prm.core_max_d == UINT64_MAX && prm.acc_den == 0)
        die(101, "pansim: --print_clusters needs --cluster_core_max, --cluster_acc_max or both");
}

static void parse_differentiation(Vals &val, Switches &present, const ps_sim_params &p, Options &o)   // --print_differentiation: as parse_hist
{
    o.diff.on = present["print_differentiation"];
    o.diff.prm.max_groups = (uint32_t)whole_flag(val, "diff_max_groups", "1 <= X <= 16", 1, PS_GROUPS_MAX);
    o.diff.prm.min_size = (uint32_t)whole_flag(val, "diff_min_size", "a whole number >= 1", 1, 0xffffffffull);
    if (o.diff.on) {
        if (o.clusters.prm.core_max_d == UINT64_MAX && o.clusters.prm.acc_den == 0)
            die(101, "pansim: --print_differentiation needs --cluster_core_max, --cluster_acc_max or both");
        if (p.pop_size > 65536) die(101, "pansim: --print_differentiation needs pop_size <= 65536, not --pop_size " + std::to_string(p.pop_size));
    }
}

// --print_tree, --print_upgma: the metric is checked whether or not the flag is given
static void parse_tree(Vals &val, Switches &present, Options &o) { o.tree = { present["print_tree"], { metric_flag(val, "tree_metric") } }; }
// (the limits of a read-out that builds a tree, the UPGMA one if `upgma`, that the flags already decide, before any device work; exact
// after --load_state as well: pop_size and core_genes must be the state file's, ps_sim_load refuses a file that differs)
static void check_tree(const char *flag, bool upgma, const ps_sim_params &p, const Options &o)
{
    if (p.pop_size < 2 || p.pop_size > PS_PARS_MAX_POP)
        die(101, std::string("pansim: --") + flag + " needs 2 <= pop_size <= 16384, not --pop_size " + std::to_string(p.pop_size));
    if (upgma && o.upgma.prm.metric == PS_TREE_ACC && p.core_genes < 1)
        die(101, "pansim: --upgma_metric acc needs core_genes >= 1, not --core_genes " + std::to_string(p.core_genes));
}
static void parse_upgma(Vals &val, Switches &present, const ps_sim_params &p, Options &o)
{
    o.upgma = { present["print_upgma"], { metric_flag(val, "upgma_metric") } };
    if (o.upgma.on) check_tree("print_upgma", true, p, o);
}

static void parse_knn(Vals &val, const ps_sim_params &p, Options &o)   // --print_knn: its metric is checked whether or not it is given
{
    o.knn = { metric_flag(val, "knn_metric"), 0 };
    if (val["print_knn"].empty()) return;
    const unsigned long long k = whole_flag(val, "print_knn");
    if (k < 1 || k > PS_KNN_MAX_K || k + 1 > p.pop_size)
        die(101, "pansim: --print_knn must be 1 <= X <= min(pop_size - 1, 128), not " + val["print_knn"] + " with --pop_size " + std::to_string(p.pop_size));
    o.knn.k = (uint32_t)k;
}

static void parse_clock(Vals &val, Options &o)   // --print_genealogy: the bins and the metric of its clock histogram, checked whether or not it is given
{
    o.clock = { metric_flag(val, "clock_metric"), 32, 64, 0, 0 };
    bins_flag(val, "clock_bins", "<Bt>,<Bx>", 1024, 16384, 1, 0, "Bt must be at most 1024 and (Bt + 1) x Bx at most 16384", &o.clock.time_bins,
              &o.clock.dist_bins);
}

static void parse_ld(Vals &val, Switches &present, Options &o)   // --print_ld: its metric, bins and selection are checked whether or not it is given
{
    o.ld = { present["print_ld"], metric_flag(val, "ld_metric"), { 64, 1, 1, 4096 } };
    bins_flag(val, "ld_bins", "<r2>,<lag>", 16384, 32, 0, 0, "lag must be at most 32 and the product of the two at most 16384", &o.ld.prm.r2_bins,
              &o.ld.prm.lag_bins);
    const std::pair<const char *, uint32_t *> whole[] = { { "ld_max_loci", &o.ld.prm.max_loci }, { "ld_min_minor", &o.ld.prm.min_minor } };
    for (const auto &w : whole) {
        const unsigned long long v = whole_flag(val, w.first);
        if (v < 1 || v > 0xffffffffull) die(101, std::string("pansim: --") + w.first + " must be at least 1 and below 2^32, not " + val[w.first]);
        *w.second = (uint32_t)v;
    }
    if (o.ld.prm.max_loci > PS_LD_MAX_LOCI) die(101, "pansim: --ld_max_loci must be 1 <= X <= 65536, not " + val["ld_max_loci"]);
}

static bool is_tree_source(const std::string &x) { return x == "upgma" || x == "tree" || x == "genealogy"; }

static void parse_parsimony(Vals &val, const ps_sim_params &p, Options &o)   // --print_parsimony: the tree it names, before any device work
{
    const std::string &s = o.pars_source = val["print_parsimony"];
    if (s.empty()) return;
    if (!is_tree_source(s)) die(101, "pansim: --print_parsimony must be upgma, tree or genealogy, not \"" + s + "\"");
    if (s == "genealogy" && val["print_genealogy"].empty())
        die(101, "pansim: --print_parsimony genealogy needs --print_genealogy: nothing is recorded without it");
    check_tree("print_parsimony", s == "upgma", p, o);
}

// whether one of the two trees of --print_tree_compare is `source`
static bool compares(const Options &o, const char *source) { return o.tcmp_source[0] == source || o.tcmp_source[1] == source; }

static void parse_tree_compare(Vals &val, const ps_sim_params &p, Options &o)   // --print_tree_compare: the two trees it names and the bins, before any device work
{
    o.tcmp = { 32, 32, 0, 0, 1 };
    const std::string &t = val["print_tree_compare"];
    if (t.empty()) return;
    const size_t comma = t.find(',');
    o.tcmp_source[0] = t.substr(0, comma);
    o.tcmp_source[1] = comma == std::string::npos ? "" : t.substr(comma + 1);
    for (const std::string &x : o.tcmp_source)
        if (!is_tree_source(x)) die(101, "pansim: --print_tree_compare must be <a>,<b>, each of upgma, tree or genealogy, not \"" + t + "\"");
    if (o.tcmp_source[0] == o.tcmp_source[1]) die(101, "pansim: --print_tree_compare needs two different trees, not \"" + t + "\"");
    if (compares(o, "genealogy") && val["print_genealogy"].empty())
        die(101, "pansim: --print_tree_compare genealogy needs --print_genealogy: nothing is recorded without it");
    check_tree("print_tree_compare", compares(o, "upgma"), p, o);
    bins_flag(val, "tree_compare_bins", "<Ba>,<Bb>", 1024, 1024, 1, 1, "both must be at most 1024 and (Ba + 1) x (Bb + 1) at most 16384", &o.tcmp.bins_a,
              &o.tcmp.bins_b);
}

static void parse_genealogy(Vals &val, Options &o)   // --print_genealogy: the generations to record
{
    const std::string &t = val["print_genealogy"];
    if (t.empty()) return;
    const unsigned long long c = whole_flag(val, "print_genealogy");
    if (c < 1 || c > 0xffffffffull) die(101, "pansim: --print_genealogy must be 1 <= X < 2^32 generations, not " + t);
    o.record_capacity = (uint32_t)c;
    // (a coalescence time is a value of ps_tree_compare: at most 2^18 - 1)
    if (compares(o, "genealogy") && c > 262143)
        die(101, "pansim: --print_tree_compare genealogy needs --print_genealogy <= 262143 generations, not " + t);
}

static void write_core_freqs(const Run &run)                        // --print_core_freqs (docs/CORE_DIVERSITY.md)
{
    const ps_sim_params &p = run.p;
    std::vector<uint32_t> cnt(4 * (size_t)p.core_size + 1);
    std::vector<uint64_t> spec((size_t)p.pop_size + 1);
    ps_core_diversity_t dv;
    // (a run has no entry of its own for these two: the loaded one asks its core matrix)
    CK(run.multi ? ps_multi_site_allele_counts(run.multi, cnt.data()) : ps_site_allele_counts(ps_sim_core(run.sim), cnt.data()));
    CK(run.multi ? ps_multi_core_diversity(run.multi, &dv, spec.data()) : ps_core_diversity(ps_sim_core(run.sim), &dv, spec.data()));
    Out sites_tsv(run, "_core_freqs.tsv");
    for (uint64_t s = 0; s < p.core_size; s++) fprintf(sites_tsv, "%u\t%u\t%u\t%u\n", cnt[4 * s], cnt[4 * s + 1], cnt[4 * s + 2], cnt[4 * s + 3]);
    Out summary(run, "_core_diversity.tsv");
    write_fields(summary, { { "pop_size", dv.pop_size }, { "sites", dv.sites }, { "other_cells", dv.other_cells },
                            { "segregating_sites", dv.segregating_sites }, { "pair_differences", dv.pair_differences },
                            { "base_cells_A", dv.base_cells[0] }, { "base_cells_C", dv.base_cells[1] }, { "base_cells_G", dv.base_cells[2] },
                            { "base_cells_T", dv.base_cells[3] } });
    fprintf(summary, "mean_pairwise_distance\t%s\n", fmt(dv.mean_pairwise_distance).c_str());
    for (uint64_t m = 0; m < spec.size(); m++)
        if (spec[m]) fprintf(summary, "spectrum\t%llu\t%llu\n", (unsigned long long)m, (unsigned long long)spec[m]);
}

static void write_hist(const Run &run, const Options &o)            // --print_dist_hist (docs/DISTANCE_HISTOGRAM.md)
{
    std::vector<uint64_t> joint((size_t)o.hist.prm.core_bins * o.hist.prm.acc_bins);
    ps_pair_hist_t h;
    CK(run.call(ps_multi_distance_histogram, ps_sim_distance_histogram, &o.hist.prm, &h, joint.data()));
    write_bins(run, "_dist_hist.tsv", joint, h.core_bins, h.acc_bins);
    Out summary(run, "_dist_hist_summary.tsv");
    write_fields(summary, { { "pop_size", h.pop_size }, { "pairs", h.pairs }, { "core_sites", h.core_sites }, { "core_genes", h.core_genes },
                            { "core_bins", h.core_bins }, { "acc_bins", h.acc_bins }, { "core_span", h.core_span },
                            { "undefined_pairs", h.undefined_pairs }, { "core_clamped", h.core_clamped }, { "core_d_min", h.core_d_min },
                            { "core_d_max", h.core_d_max }, { "core_d_sum", h.core_d_sum } });
    // the 128-bit square sum as one decimal number
    unsigned __int128 sq = ((unsigned __int128)h.core_d_sqsum_hi << 64) | h.core_d_sqsum_lo;
    std::string dec;
    do { dec.insert(dec.begin(), (char)('0' + (int)(sq % 10))); sq /= 10; } while (sq);
    fprintf(summary, "core_d_sqsum\t%s\nmean_core_distance\t%s\n", dec.c_str(), fmt(h.mean_core_distance).c_str());
}

static void write_clusters(const Run &run, const Options &o)        // --print_clusters (docs/STRAIN_CLUSTERS.md)
{
    const ps_cluster_params &prm = o.clusters.prm;
    ps_cluster_t c;
    const std::vector<uint32_t> labels = strain_labels(run, prm, &c);
    Out clusters(run, "_clusters.tsv");
    for (size_t k = 0; k < labels.size(); k++) fprintf(clusters, "%zu\t%u\n", k, labels[k]);
    Out summary(run, "_clusters_summary.tsv");
    write_fields(summary, { { "pop_size", c.pop_size }, { "pairs", c.pairs }, { "core_sites", c.core_sites }, { "core_genes", c.core_genes },
                            { "edges", c.edges }, { "clusters", c.clusters }, { "singletons", c.singletons },
                            { "largest_cluster", c.largest_cluster }, { "within_pairs", c.within_pairs }, { "undefined_pairs", c.undefined_pairs },
                            { "core_max_d", prm.core_max_d }, { "acc_num", prm.acc_num }, { "acc_den", prm.acc_den } });
}

static void write_differentiation(const Run &run, const Options &o) // --print_differentiation (docs/GROUP_DIFFERENTIATION.md)
{
    const ps_sim_params &p = run.p;
    const size_t n = (size_t)p.pop_size, M = o.diff.prm.max_groups, L = (size_t)p.core_size, G = (size_t)(p.pan_genes - p.core_genes);
    std::vector<uint32_t> group_of(n), glabel(M), gsize(M), within(std::max<size_t>(L, 1)), total(std::max<size_t>(L, 1)), gc(std::max<size_t>(G * M, 1));
    std::vector<uint64_t> between(M * M), fixed(M * M), acc_between(M * M), gene_fixed(M * M), gene_private(M);
    ps_cluster_t c;
    const std::vector<uint32_t> labels = strain_labels(run, o.clusters.prm, &c);
    ps_diff_t d;
    CK(run.call(ps_multi_group_differentiation, ps_sim_group_differentiation, labels.data(), &o.diff.prm, &d, group_of.data(), glabel.data(),
                gsize.data(), between.data(), fixed.data(), within.data(), total.data(), nullptr, gc.data(), acc_between.data(), gene_fixed.data(),
                gene_private.data()));
    const size_t K = (size_t)d.groups;
    Out groups(run, "_diff_groups.tsv");
    for (size_t g = 0; g < K; g++)
        fprintf(groups, "%zu\t%u\t%u\t%llu\t%llu\t%llu\n", g, glabel[g], gsize[g], (unsigned long long)between[g * K + g],
                (unsigned long long)fixed[g * K + g], (unsigned long long)gene_private[g]);
    Out pairs(run, "_diff_between.tsv");
    for (size_t g = 0; g < K; g++)
        for (size_t h = g + 1; h < K; h++)
            fprintf(pairs, "%zu\t%zu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", g, h, (unsigned long long)gsize[g] * gsize[h],
                    (unsigned long long)between[g * K + h], (unsigned long long)fixed[g * K + h], (unsigned long long)acc_between[g * K + h],
                    (unsigned long long)gene_fixed[g * K + h], (unsigned long long)gene_fixed[h * K + g]);
    Out sites(run, "_diff_sites.tsv");
    for (uint64_t s = 0; s < d.sites; s++) fprintf(sites, "%u\t%u\n", within[s], total[s]);
    Out genes(run, "_diff_genes.tsv");
    for (uint64_t y = 0; y < d.genes; y++)
        for (size_t g = 0; g < K; g++) fprintf(genes, "%u%c", gc[y * K + g], g + 1 == K ? '\n' : '\t');
    Out summary(run, "_diff_summary.tsv");
    write_fields(summary, { { "pop_size", d.pop_size }, { "sites", d.sites }, { "genes", d.genes }, { "groups", d.groups },
                            { "assigned", d.assigned }, { "unassigned", d.unassigned }, { "other_cells", d.other_cells },
                            { "within_pairs", d.within_pairs }, { "between_pairs", d.between_pairs }, { "within_differences", d.within_differences },
                            { "between_differences", d.between_differences } });
    fprintf(summary, "pi_within\t%s\npi_between\t%s\nfst\t%s\n", fmt(d.pi_within).c_str(), fmt(d.pi_between).c_str(), fmt(d.fst).c_str());
    fprintf(summary, "diff_max_groups\t%u\ndiff_min_size\t%u\n", o.diff.prm.max_groups, o.diff.prm.min_size);
}

static void write_tree(const Run &run, const Options &o)            // --print_tree (docs/LINKAGE_TREE.md)
{
    const size_t n = (size_t)run.p.pop_size;
    std::vector<uint32_t> lo(n), hi(n);
    std::vector<uint64_t> num(n), den(n);
    ps_tree_t t;
    CK(run.call(ps_multi_linkage_tree, ps_sim_linkage_tree, &o.tree.prm, &t, lo.data(), hi.data(), num.data(), den.data()));
    Out tree(run, "_tree.tsv");
    for (uint64_t k = 0; k < t.edges; k++)
        fprintf(tree, "%u\t%u\t%llu\t%llu\t%s\n", lo[k], hi[k], (unsigned long long)num[k], (unsigned long long)den[k], ratio(num[k], den[k]).c_str());
    Out summary(run, "_tree_summary.tsv");
    write_fields(summary, { { "pop_size", t.pop_size }, { "pairs", t.pairs }, { "core_sites", t.core_sites }, { "core_genes", t.core_genes },
                            { "metric", t.metric }, { "edges", t.edges }, { "undefined_edges", t.undefined_edges },
                            { "distinct_heights", t.distinct_heights } });
}

static void write_upgma(const Run &run, const Options &o)           // --print_upgma (docs/UPGMA_TREE.md)
{
    const size_t n = (size_t)run.p.pop_size;
    std::vector<uint32_t> left(n), right(n), size(n);
    std::vector<uint64_t> num(n), den(n);
    ps_upgma_t t;
    CK(run.call(ps_multi_upgma_tree, ps_sim_upgma_tree, &o.upgma.prm, &t, left.data(), right.data(), size.data(), num.data(), den.data()));
    Out upgma(run, "_upgma.tsv");
    for (uint64_t k = 0; k < t.merges; k++)
        fprintf(upgma, "%llu\t%u\t%u\t%u\t%llu\t%llu\t%s\n", (unsigned long long)(t.pop_size + k), left[k], right[k], size[k],
                (unsigned long long)num[k], (unsigned long long)den[k], fmt((double)num[k] / (double)den[k]).c_str());
    write_newick(run, "_upgma.nwk", "\n", [&](char *text, uint64_t cap, uint64_t *need) {
        return ps_upgma_newick(left.data(), right.data(), num.data(), den.data(), t.pop_size, text, cap, need);
    });
    Out summary(run, "_upgma_summary.tsv");
    write_fields(summary, { { "pop_size", t.pop_size }, { "pairs", t.pairs }, { "core_sites", t.core_sites }, { "core_genes", t.core_genes },
                            { "metric", t.metric }, { "merges", t.merges }, { "distinct_heights", t.distinct_heights }, { "root_num", t.root_num },
                            { "root_den", t.root_den } });
}

static void write_knn(const Run &run, const Options &o)             // --print_knn (docs/NEAREST_NEIGHBOURS.md)
{
    const size_t n = (size_t)run.p.pop_size, k = o.knn.k;
    std::vector<uint32_t> nbr(n * k), labels(n);
    std::vector<uint64_t> num(n * k), den(n * k);
    ps_knn_t t;
    CK(run.call(ps_multi_nearest_neighbours, ps_sim_nearest_neighbours, &o.knn, &t, nbr.data(), num.data(), den.data()));
    Out knn(run, "_knn.tsv");
    for (size_t e = 0; e < n * k; e++)
        fprintf(knn, "%zu\t%zu\t%u\t%llu\t%llu\t%s\n", e / k, e % k + 1, nbr[e], (unsigned long long)num[e], (unsigned long long)den[e],
                ratio(num[e], den[e]).c_str());
    Out summary(run, "_knn_summary.tsv");
    write_fields(summary, { { "pop_size", t.pop_size }, { "pairs", t.pairs }, { "core_sites", t.core_sites }, { "core_genes", t.core_genes },
                            { "metric", t.metric }, { "k", t.k }, { "undefined_neighbours", t.undefined_neighbours },
                            { "graph_edges", t.graph_edges }, { "mutual_edges", t.mutual_edges } });
    // the lineages at every rank; the labels of the last one (rank k) are the ones written
    for (uint32_t r = 1; r <= o.knn.k; r++) {
        ps_lineage_t l;
        CK(ps_lineages_from_neighbours(nbr.data(), n, o.knn.k, r, &l, labels.data()));
        fprintf(summary, "lineages\t%u\t%llu\t%llu\n", r, (unsigned long long)l.lineages, (unsigned long long)l.largest_lineage);
    }
    Out lineages(run, "_lineages.tsv");
    for (size_t i = 0; i < n; i++) fprintf(lineages, "%zu\t%u\n", i, labels[i]);
}

static void write_ld(const Run &run, const Options &o)              // --print_ld (docs/LINKAGE_DISEQUILIBRIUM.md)
{
    const ps_ld_params &prm = o.ld.prm;
    const size_t nl = prm.lag_bins, nr = prm.r2_bins;
    std::vector<uint32_t> index(prm.max_loci), count(prm.max_loci);
    std::vector<uint64_t> hist(nl * nr), lag_sum(nl);
    ps_ld_t t;
    CK(run.call(ps_multi_locus_ld, ps_sim_locus_ld, o.ld.metric, &prm, nullptr, 0, &t, index.data(), count.data(), hist.data(), lag_sum.data()));
    write_bins(run, "_ld.tsv", hist, nl, nr);
    Out summary(run, "_ld_summary.tsv");
    write_fields(summary, { { "pop_size", t.pop_size }, { "metric", (uint64_t)o.ld.metric }, { "columns", t.columns }, { "candidates", t.candidates },
                            { "loci", t.loci }, { "pairs", t.pairs }, { "defined_pairs", t.defined_pairs }, { "undefined_pairs", t.undefined_pairs },
                            { "four_gamete_pairs", t.four_gamete_pairs }, { "complete_pairs", t.complete_pairs },
                            { "positive_pairs", t.positive_pairs }, { "negative_pairs", t.negative_pairs }, { "sum_q", t.sum_q },
                            { "r2_bins", t.r2_bins }, { "lag_bins", t.lag_bins }, { "min_minor", t.min_minor }, { "max_loci", t.max_loci } });
    fprintf(summary, "mean_r2\t%s\n", fmt(t.mean_r2).c_str());
    for (size_t l = 0; l < nl; l++) {
        uint64_t n = 0;
        for (size_t r = 0; r < nr; r++) n += hist[l * nr + r];
        if (n) fprintf(summary, "lag\t%zu\t%llu\t%llu\n", l, (unsigned long long)n, (unsigned long long)lag_sum[l]);
    }
    Out loci(run, "_ld_loci.tsv");
    for (uint64_t k = 0; k < t.loci; k++) fprintf(loci, "%u\t%u\n", index[k], count[k]);
}

static void write_genealogy(const Run &run, const Options &o)       // --print_genealogy: the comb, its trees and the clock histogram (docs/GENEALOGY.md)
{
    const size_t n = (size_t)run.p.pop_size;
    std::vector<uint32_t> order(n), coal(n);
    ps_genealogy_t g;
    CK(run.call(ps_multi_genealogy, ps_sim_genealogy, &g, order.data(), coal.data()));
    Out genealogy(run, "_genealogy.tsv");
    for (size_t r = 0; r < n; r++)
        fprintf(genealogy, "%zu\t%u\t%s\n", r, order[r], r + 1 == n ? "" : coal[r] == PS_GEN_BEYOND ? "beyond" : std::to_string(coal[r]).c_str());
    write_newick(run, "_genealogy.nwk", "", [&](char *text, uint64_t cap, uint64_t *need) {
        return ps_genealogy_newick(order.data(), coal.data(), n, text, cap, need);
    });
    // (a run that recorded no generation -- a loaded state already at --n_gen -- has no divergence times to bin)
    if (g.depth == 0) {
        fprintf(stderr, "pansim: no generation was recorded: %s_clock.tsv and %s_clock_summary.tsv are not written\n", run.outpref.c_str(), run.outpref.c_str());
        return;
    }
    const size_t nt = (size_t)o.clock.time_bins + 1, bx = o.clock.dist_bins;
    std::vector<uint64_t> joint(nt * bx), per_time(3 * nt);
    ps_clock_t c;
    CK(run.call(ps_multi_clock_histogram, ps_sim_clock_histogram, &o.clock, &c, joint.data(), per_time.data()));
    write_bins(run, "_clock.tsv", joint, nt, bx);
    Out summary(run, "_clock_summary.tsv");
    write_fields(summary, { { "pop_size", c.pop_size }, { "pairs", c.pairs }, { "core_sites", c.core_sites }, { "core_genes", c.core_genes },
                            { "metric", c.metric }, { "time_bins", c.time_bins }, { "dist_bins", c.dist_bins }, { "time_span", c.time_span },
                            { "core_span", c.core_span }, { "generation", g.generation }, { "capacity", g.capacity }, { "depth", c.depth },
                            { "roots", g.roots }, { "tmrca", g.tmrca }, { "undefined_pairs", c.undefined_pairs }, { "core_clamped", c.core_clamped },
                            { "beyond_pairs", c.beyond_pairs }, { "binned_pairs", c.binned_pairs }, { "num_sum", c.num_sum },
                            { "den_sum", c.den_sum } });
    for (size_t t = 0; t < nt; t++)
        if (per_time[3 * t])
            fprintf(summary, "time\t%zu\t%llu\t%llu\t%llu\n", t, (unsigned long long)per_time[3 * t], (unsigned long long)per_time[3 * t + 1],
                    (unsigned long long)per_time[3 * t + 2]);
}

// one of the three trees as a merge list: merge k joins the nodes left[k] and right[k]; vals (on demand): the values
// --print_tree_compare reads it with -- the dense ranks of its heights, the coalescence times of the genealogy
struct Merges { std::vector<uint32_t> left, right, vals; uint64_t M; };
static Merges merge_list(const Run &run, const Options &o, const std::string &source, bool with_vals)
{
    const size_t n = (size_t)run.p.pop_size;
    Merges m = { std::vector<uint32_t>(n), std::vector<uint32_t>(n), std::vector<uint32_t>(with_vals ? n : 0), 0 };
    uint32_t *const vals = with_vals ? m.vals.data() : nullptr;
    std::vector<uint32_t> a(n), b(n);                                   // size | lo, hi | order, coal
    std::vector<uint64_t> num(n), den(n);
    if (source == "genealogy") {
        ps_genealogy_t g;
        CK(run.call(ps_multi_genealogy, ps_sim_genealogy, &g, a.data(), b.data()));
        CK(ps_merges_from_genealogy(a.data(), b.data(), n, m.left.data(), m.right.data(), vals, &m.M));
        return m;
    }
    if (source == "upgma") {
        ps_upgma_t t;
        CK(run.call(ps_multi_upgma_tree, ps_sim_upgma_tree, &o.upgma.prm, &t, m.left.data(), m.right.data(), a.data(), num.data(), den.data()));
        m.M = t.merges;
    } else {
        ps_tree_t t;
        CK(run.call(ps_multi_linkage_tree, ps_sim_linkage_tree, &o.tree.prm, &t, a.data(), b.data(), num.data(), den.data()));
        CK(ps_merges_from_tree(a.data(), b.data(), t.edges, n, m.left.data(), m.right.data(), &m.M));
    }
    if (vals) CK(ps_levels_from_heights(num.data(), den.data(), m.M, vals, nullptr));
    return m;
}

static void write_parsimony(const Run &run, const Options &o)       // --print_parsimony (docs/TREE_PARSIMONY.md)
{
    const ps_sim_params &p = run.p;
    const size_t n = (size_t)p.pop_size, L = (size_t)p.core_size, G = (size_t)(p.pan_genes - p.core_genes);
    const Merges m = merge_list(run, o, o.pars_source, false);
    const uint64_t M = m.M;
    if (M == 0) {
        fprintf(stderr, "pansim: the %s of --print_parsimony has no merge: the _parsimony files are not written\n", o.pars_source.c_str());
        return;
    }
    const size_t nodes = n + (size_t)M;
    std::vector<uint32_t> sites(std::max<size_t>(L, 1)), gch(std::max<size_t>(G, 1)), ggn(std::max<size_t>(G, 1)), gls(std::max<size_t>(G, 1));
    std::vector<uint64_t> hist(PS_PARS_BINS), bch(nodes), bgn(nodes), bls(nodes);
    ps_parsimony_t t;
    CK(run.call(ps_multi_tree_parsimony, ps_sim_tree_parsimony, m.left.data(), m.right.data(), M, &t, sites.data(), hist.data(), bch.data(), gch.data(),
                ggn.data(), gls.data(), bgn.data(), bls.data()));
    Out sites_tsv(run, "_parsimony_sites.tsv");
    for (uint64_t s = 0; s < t.sites; s++) fprintf(sites_tsv, "%u\n", sites[s]);
    Out genes_tsv(run, "_parsimony_genes.tsv");
    for (uint64_t y = 0; y < t.genes; y++) fprintf(genes_tsv, "%u\t%u\t%u\n", gch[y], ggn[y], gls[y]);
    const std::vector<long long> parent = merge_parents(m.left.data(), m.right.data(), M, n);
    Out branches(run, "_parsimony_branches.tsv");
    for (size_t x = 0; x < nodes; x++)
        fprintf(branches, "%zu\t%lld\t%llu\t%llu\t%llu\n", x, parent[x], (unsigned long long)bch[x], (unsigned long long)bgn[x], (unsigned long long)bls[x]);
    // Newick, one line per root: an explicit stack (a caterpillar is pop_size deep); text entries are negative
    auto tail = [&](size_t x) { return parent[x] >= 0 ? ":" + fmt(t.sites ? (double)bch[x] / (double)t.sites : 0.0) : std::string(); };
    Out nwk(run, "_parsimony.nwk");
    for (size_t root = n; root < nodes; root++) {
        if (parent[root] >= 0) continue;
        std::vector<long long> stack{ (long long)root };
        while (!stack.empty()) {
            const long long e = stack.back();
            stack.pop_back();
            if (e == -1) fputs(",", nwk);
            else if (e < -1) fprintf(nwk, ")%s", tail((size_t)(-e - 2)).c_str());
            else if ((size_t)e < n) fprintf(nwk, "%lld%s", e, tail((size_t)e).c_str());
            else {
                fputs("(", nwk);
                stack.insert(stack.end(), { -e - 2, (long long)m.right[(size_t)e - n], -1, (long long)m.left[(size_t)e - n] });
            }
        }
        fputs(";\n", nwk);
    }
    Out summary(run, "_parsimony_summary.tsv");
    write_fields(summary, { { "pop_size", t.pop_size }, { "sites", t.sites }, { "genes", t.genes }, { "merges", t.merges }, { "trees", t.trees },
                            { "covered_leaves", t.covered_leaves }, { "spanning", t.spanning }, { "total_changes", t.total_changes },
                            { "changed_sites", t.changed_sites }, { "max_changes", t.max_changes }, { "gene_total_changes", t.gene_total_changes },
                            { "gene_total_gains", t.gene_total_gains }, { "gene_total_losses", t.gene_total_losses },
                            { "min_changes", t.min_changes }, { "excess_changes", t.excess_changes }, { "homoplasic_sites", t.homoplasic_sites } });
    fprintf(summary, "ci\t%s\ntree\t%s\n", fmt(t.ci).c_str(), o.pars_source.c_str());
}

static void write_tree_compare(const Run &run, const Options &o)    // --print_tree_compare (docs/TREE_COMPARISON.md)
{
    const size_t n = (size_t)run.p.pop_size;
    const Merges m[2] = { merge_list(run, o, o.tcmp_source[0], true), merge_list(run, o, o.tcmp_source[1], true) };
    if (m[0].M == 0 || m[1].M == 0) {
        fprintf(stderr, "pansim: the %s of --print_tree_compare has no merge: the _tree_compare files are not written\n",
                o.tcmp_source[m[0].M == 0 ? 0 : 1].c_str());
        return;
    }
    const size_t na = (size_t)o.tcmp.bins_a + 1, nb = (size_t)o.tcmp.bins_b + 1;
    std::vector<uint64_t> joint(na * nb);
    std::vector<uint8_t> in_other[2] = { std::vector<uint8_t>(m[0].M), std::vector<uint8_t>(m[1].M) };
    ps_tree_compare_t t;
    CK(run.call(ps_multi_tree_compare, ps_sim_tree_compare, m[0].left.data(), m[0].right.data(), m[0].vals.data(), m[0].M, m[1].left.data(), m[1].right.data(),
                m[1].vals.data(), m[1].M, &o.tcmp, &t, joint.data(), in_other[0].data(), in_other[1].data()));
    write_bins(run, "_tree_compare.tsv", joint, na, nb);
    // the clades: the merges whose parent carries another value (or that have none), with the leaves below them
    Out clades(run, "_tree_compare_clades.tsv");
    for (int x = 0; x < 2; x++) {
        const std::vector<uint32_t> &left = m[x].left, &right = m[x].right, &vals = m[x].vals;
        const std::vector<long long> parent = merge_parents(left.data(), right.data(), m[x].M, n);
        std::vector<uint32_t> size(m[x].M);
        for (uint64_t k = 0; k < m[x].M; k++)
            for (uint32_t c : { left[k], right[k] }) size[k] += c < n ? 1u : size[c - n];
        for (uint64_t k = 0; k < m[x].M; k++)
            if (parent[n + k] < 0 || vals[(size_t)parent[n + k] - n] != vals[k])
                fprintf(clades, "%s\t%llu\t%u\t%u\t%u\n", o.tcmp_source[x].c_str(), (unsigned long long)(n + k), size[k], vals[k], (unsigned)in_other[x][k]);
    }
    Out summary(run, "_tree_compare_summary.tsv");
    write_fields(summary, { { "pop_size", t.pop_size }, { "merges_a", t.merges_a }, { "merges_b", t.merges_b }, { "pairs", t.pairs },
                            { "joined_both", t.joined_both }, { "joined_a_only", t.joined_a_only }, { "joined_b_only", t.joined_b_only },
                            { "joined_neither", t.joined_neither }, { "sum_a", t.sum_a }, { "sum_b", t.sum_b }, { "sum_aa", t.sum_aa },
                            { "sum_bb", t.sum_bb }, { "sum_ab", t.sum_ab }, { "triples", t.triples }, { "resolved_a", t.resolved_a },
                            { "resolved_b", t.resolved_b }, { "shared_triplets", t.shared_triplets }, { "clades_a", t.clades_a },
                            { "clades_b", t.clades_b }, { "shared_clades", t.shared_clades }, { "rf_distance", t.rf_distance },
                            { "bins_a", t.bins_a }, { "bins_b", t.bins_b }, { "span_a", t.span_a }, { "span_b", t.span_b } });
    fprintf(summary, "cophenetic_r\t%s\ntriplet_recall\t%s\ntriplet_precision\t%s\nclade_recall\t%s\nclade_precision\t%s\n", fmt(t.cophenetic_r).c_str(),
            fmt(t.triplet_recall).c_str(), fmt(t.triplet_precision).c_str(), fmt(t.clade_recall).c_str(), fmt(t.clade_precision).c_str());
    fprintf(summary, "a\t%s\nb\t%s\n", o.tcmp_source[0].c_str(), o.tcmp_source[1].c_str());
}
