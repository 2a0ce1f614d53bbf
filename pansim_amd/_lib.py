"""ctypes loader for libpansim_hip.so (the C ABI of include/pansim_hip.h).

The library is built in-tree by `make -C pansim_amd/csrc` (see __graft_entry__.build).
There is no fallback: if the shared object is missing, loading fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PANSIM_HIP_LIBRARY") or os.path.join(_HERE, "libpansim_hip.so")

PS_OK = 0
PS_ERR_INVALID, PS_ERR_NO_DEVICE, PS_ERR_OOM, PS_ERR_WEIGHTS, PS_ERR_IO, PS_ERR_STATE = -1, -2, -3, -4, -5, -6


class PansimError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libpansim_hip error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("pop_size", C.c_uint64), ("ncols", C.c_uint64), ("global_cols", C.c_uint64),
                ("col_offset", C.c_uint64), ("core_genes", C.c_uint64), ("seed", C.c_uint64),
                ("core", C.c_int32), ("device", C.c_int32)]


class SimParams(C.Structure):
    _fields_ = [("pop_size", C.c_uint64), ("core_size", C.c_uint64), ("pan_genes", C.c_uint64),
                ("core_genes", C.c_uint64), ("avg_gene_freq", C.c_double), ("HR_rate", C.c_double),
                ("HGT_rate", C.c_double), ("n_gen", C.c_int32), ("max_distances", C.c_uint64),
                ("core_mu", C.c_double), ("rate_genes1", C.c_double), ("rate_genes2", C.c_double),
                ("prop_genes2", C.c_double), ("prop_positive", C.c_double),
                ("pos_lambda", C.c_double), ("neg_lambda", C.c_double), ("seed", C.c_uint64),
                ("print_dist", C.c_int32), ("print_matrices", C.c_int32),
                ("print_selection", C.c_int32), ("verbose", C.c_int32),
                ("no_control_genome_size", C.c_int32), ("genome_size_penalty", C.c_double),
                ("competition_strength", C.c_double), ("shard_rank", C.c_int32),
                ("shard_count", C.c_int32), ("device", C.c_int32), ("reference_seed_stream", C.c_int32)]


class Derived(C.Structure):
    _fields_ = [("pan_size", C.c_uint64), ("avg_gene_freq_adj", C.c_double),
                ("avg_gene_num", C.c_int32), ("n_core_mutations", C.c_double),
                ("n_recombinations_core", C.c_double), ("n_recombinations_pan_total", C.c_double),
                ("n_comp", C.c_int32), ("comp_begin", C.c_uint64 * 2), ("comp_end", C.c_uint64 * 2),
                ("n_pan_mutations", C.c_double * 2), ("n_recombinations_pan", C.c_double * 2)]


class StateHeader(C.Structure):
    """ps_state_header: what ps_state_info reads from a state file (docs/STATE_FORMAT.md)"""
    _fields_ = [("version", C.c_uint32), ("core_encoding", C.c_uint32), ("generations_done", C.c_uint64),
                ("pan_size", C.c_uint64), ("site_begin", C.c_uint64), ("site_end", C.c_uint64), ("pitch", C.c_uint64),
                ("core_offset", C.c_uint64), ("core_bytes", C.c_uint64), ("acc_offset", C.c_uint64),
                ("acc_bytes", C.c_uint64), ("maps_offset", C.c_uint64), ("maps_bytes", C.c_uint64),
                ("per_gen_offset", C.c_uint64), ("per_gen_bytes", C.c_uint64), ("has_row_maps", C.c_int32),
                ("core_rows_overridden", C.c_int32), ("acc_rows_overridden", C.c_int32), ("has_per_gen", C.c_int32)]


PS_STATE_PACKED2, PS_STATE_RAW8 = 1, 2


class CoreDiversity(C.Structure):
    """ps_core_diversity_t: the summary of ps_core_diversity / ps_diversity_from_counts (docs/CORE_DIVERSITY.md)"""
    _fields_ = [("pop_size", C.c_uint64), ("sites", C.c_uint64), ("other_cells", C.c_uint64),
                ("segregating_sites", C.c_uint64), ("pair_differences", C.c_uint64), ("base_cells", C.c_uint64 * 4),
                ("mean_pairwise_distance", C.c_double)]


class PairHistParams(C.Structure):
    """ps_pair_hist_params: the bins of ps_distance_histogram (docs/DISTANCE_HISTOGRAM.md); core_span 0 = automatic"""
    _fields_ = [("core_bins", C.c_uint32), ("acc_bins", C.c_uint32), ("core_span", C.c_uint64)]


class PairHist(C.Structure):
    """ps_pair_hist_t: the summary of ps_distance_histogram / ps_histogram_from_counts"""
    _fields_ = [("pop_size", C.c_uint64), ("pairs", C.c_uint64), ("core_sites", C.c_uint64), ("core_genes", C.c_uint64),
                ("core_bins", C.c_uint32), ("acc_bins", C.c_uint32), ("core_span", C.c_uint64),
                ("undefined_pairs", C.c_uint64), ("core_clamped", C.c_uint64), ("core_d_min", C.c_uint64),
                ("core_d_max", C.c_uint64), ("core_d_sum", C.c_uint64), ("core_d_sqsum_lo", C.c_uint64),
                ("core_d_sqsum_hi", C.c_uint64), ("mean_core_distance", C.c_double)]


class ClusterParams(C.Structure):
    """ps_cluster_params: the thresholds of ps_strain_clusters (docs/STRAIN_CLUSTERS.md); core_max_d 2^64 - 1 = no core
    criterion, acc_den 0 = no accessory criterion"""
    _fields_ = [("core_max_d", C.c_uint64), ("acc_num", C.c_uint32), ("acc_den", C.c_uint32)]


class Clusters(C.Structure):
    """ps_cluster_t: the summary of ps_strain_clusters / ps_clusters_from_counts"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "pairs", "core_sites", "core_genes", "edges", "clusters", "singletons",
                                                 "largest_cluster", "within_pairs", "undefined_pairs", "rounds")]


PS_TREE_CORE, PS_TREE_ACC = 0, 1


class TreeParams(C.Structure):
    """ps_tree_params: the metric of ps_linkage_tree (docs/LINKAGE_TREE.md), PS_TREE_CORE or PS_TREE_ACC"""
    _fields_ = [("metric", C.c_int32)]


class Tree(C.Structure):
    """ps_tree_t: the summary of ps_linkage_tree / ps_tree_from_counts"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "pairs", "core_sites", "core_genes", "metric", "edges", "undefined_edges",
                                                 "distinct_heights", "rounds")]


class Upgma(C.Structure):
    """ps_upgma_t: the summary of ps_upgma_tree / ps_upgma_from_counts (docs/UPGMA_TREE.md)"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "pairs", "core_sites", "core_genes", "metric", "merges", "distinct_heights",
                                                 "root_num", "root_den", "rounds")]


class Nj(C.Structure):
    """ps_nj_t: the summary of ps_neighbour_joining / ps_nj_from_counts (docs/NEIGHBOUR_JOINING.md)"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "pairs", "core_sites", "core_genes", "metric", "joins", "negative_branches")]


PS_BOOT_LINKAGE, PS_BOOT_UPGMA, PS_BOOT_NJ = 0, 1, 2


class BootstrapParams(C.Structure):
    """ps_bootstrap_params: the method, the replicates, the draws per replicate (0: the core sites) and the key of the draw of
    ps_bootstrap_support (docs/BOOTSTRAP_SUPPORT.md)"""
    _fields_ = [("method", C.c_int32), ("replicates", C.c_uint32), ("draws", C.c_uint64), ("seed", C.c_uint64)]


class Bootstrap(C.Structure):
    """ps_bootstrap_t: the summary of ps_bootstrap_support"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "pairs", "core_sites", "core_genes", "method", "replicates", "draws", "merges",
                                                 "support_sum", "supported_50", "supported_70", "supported_95")]


PS_KNN_CORE, PS_KNN_ACC, PS_KNN_MAX_K = 0, 1, 128


class KnnParams(C.Structure):
    """ps_knn_params: the metric (PS_KNN_CORE or PS_KNN_ACC) and k of ps_nearest_neighbours (docs/NEAREST_NEIGHBOURS.md)"""
    _fields_ = [("metric", C.c_int32), ("k", C.c_uint32)]


class Knn(C.Structure):
    """ps_knn_t: the summary of ps_nearest_neighbours / ps_neighbours_from_counts"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "pairs", "core_sites", "core_genes", "metric", "k", "undefined_neighbours",
                                                 "graph_edges", "mutual_edges")]


class Lineages(C.Structure):
    """ps_lineage_t: the summary of ps_lineages_from_neighbours"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "rank", "edges", "lineages", "largest_lineage", "within_pairs")]


PS_GEN_BEYOND = 0xffffffff


class Genealogy(C.Structure):
    """ps_genealogy_t: the summary of ps_sim_genealogy (docs/GENEALOGY.md)"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "generation", "capacity", "depth", "roots", "tmrca")]


class GenClusters(C.Structure):
    """ps_gen_clusters_t: the summary of ps_genealogy_clusters"""
    _fields_ = [(name, C.c_uint64) for name in ("clusters", "largest", "within_pairs")]


PS_LD_CORE, PS_LD_ACC, PS_LD_MAX_LOCI = 0, 1, 65536


class LdParams(C.Structure):
    """ps_ld_params: the bins and the automatic selection of ps_locus_ld (docs/LINKAGE_DISEQUILIBRIUM.md)"""
    _fields_ = [("r2_bins", C.c_uint32), ("lag_bins", C.c_uint32), ("min_minor", C.c_uint32), ("max_loci", C.c_uint32)]


class Ld(C.Structure):
    """ps_ld_t: the summary of ps_locus_ld / ps_ld_from_counts"""
    _fields_ = ([(name, C.c_uint64) for name in ("pop_size", "columns", "candidates", "loci", "pairs", "defined_pairs", "undefined_pairs",
                                                  "four_gamete_pairs", "complete_pairs", "positive_pairs", "negative_pairs", "sum_q")]
                + [("mean_r2", C.c_double)]
                + [(name, C.c_uint64) for name in ("r2_bins", "lag_bins", "min_minor", "max_loci")])


PS_GS_NONE = 0xFFFFFFFF


class GsParams(C.Structure):
    """ps_gs_params: the bins, the automatic selection of both sides and the strong threshold of ps_gene_site_ld
    (docs/GENE_SITE_ASSOCIATION.md)"""
    _fields_ = [(name, C.c_uint32) for name in ("r2_bins", "freq_bins", "site_min_minor", "gene_min_minor", "max_sites", "max_genes", "strong_q")]


class Gs(C.Structure):
    """ps_gs_t: the summary of ps_gene_site_ld / ps_gene_site_from_counts"""
    _fields_ = ([(name, C.c_uint64) for name in ("pop_size", "site_columns", "gene_columns", "site_candidates", "gene_candidates", "sites", "genes",
                                                  "pairs", "defined_pairs", "undefined_pairs", "four_gamete_pairs", "complete_pairs",
                                                  "positive_pairs", "negative_pairs", "strong_pairs", "genes_tagged", "sites_tagging", "sum_q")]
                + [("mean_r2", C.c_double)]
                + [(name, C.c_uint64) for name in ("r2_bins", "freq_bins", "site_min_minor", "gene_min_minor", "max_sites", "max_genes", "strong_q")])


class GsSide(C.Structure):
    """ps_gs_side: the per-locus arrays of one side of ps_gene_site_ld, any of them NULL"""
    _fields_ = [(name, C.c_void_p) for name in ("index", "count", "best", "best_q", "strong", "best_sign")]


class MlstParams(C.Structure):
    """ps_mlst_params: the loci, the bins, the complex threshold and the fingerprint keys of ps_allele_profiles
    (docs/ALLELE_PROFILES.md)"""
    _fields_ = [(name, C.c_uint32) for name in ("n_loci", "dist_bins", "complex_max", "key_bits")] + [("key_seed", C.c_uint64)]


class Mlst(C.Structure):
    """ps_mlst_t: the summary of ps_allele_profiles / ps_profiles_from_alleles"""
    _fields_ = ([(name, C.c_uint64) for name in ("pop_size", "pairs", "core_sites", "loci", "sites_covered", "alleles_total", "max_alleles",
                                                  "monomorphic_loci", "sequence_types", "singleton_sts", "largest_st", "identical_pairs",
                                                  "complexes", "largest_complex", "edges", "sum_d", "min_d", "max_d")]
                + [("mean_distance", C.c_double)]
                + [(name, C.c_uint64) for name in ("dist_bins", "complex_max", "rounds")])


# &params, bounds | &summary, locus_alleles, locus_same_pairs, st, complex, hist, profiles: the tail of every ps_*allele_profiles entry
_MLST = [C.POINTER(MlstParams), C.c_void_p, C.POINTER(Mlst)] + [C.c_void_p] * 6


class ClockParams(C.Structure):
    """ps_clock_params: the metric, bins and spans of ps_sim_clock_histogram (docs/GENEALOGY.md); a span of 0 = automatic"""
    _fields_ = [("metric", C.c_int32), ("time_bins", C.c_uint32), ("dist_bins", C.c_uint32), ("time_span", C.c_uint64),
                ("core_span", C.c_uint64)]


class Clock(C.Structure):
    """ps_clock_t: the summary of ps_sim_clock_histogram / ps_clock_from_counts"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "pairs", "core_sites", "core_genes", "metric", "time_bins", "dist_bins",
                                                 "time_span", "core_span", "depth", "undefined_pairs", "core_clamped", "beyond_pairs",
                                                 "binned_pairs", "num_sum", "den_sum")]


PS_GROUPS_MAX = 16


class DiffParams(C.Structure):
    """ps_diff_params: the group rules of ps_group_differentiation (docs/GROUP_DIFFERENTIATION.md)"""
    _fields_ = [("max_groups", C.c_uint32), ("min_size", C.c_uint32)]


class Diff(C.Structure):
    """ps_diff_t: the summary of ps_group_differentiation / ps_differentiation_from_counts"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "sites", "genes", "groups", "assigned", "unassigned", "other_cells",
                                                 "within_pairs", "between_pairs", "within_differences", "between_differences")] + \
               [(name, C.c_double) for name in ("pi_within", "pi_between", "fst")]


PS_PARS_BINS, PS_PARS_MAX_POP = 64, 16384


class Parsimony(C.Structure):
    """ps_parsimony_t: the summary of ps_tree_parsimony / ps_parsimony_from_rows (docs/TREE_PARSIMONY.md)"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "sites", "genes", "merges", "trees", "covered_leaves", "spanning",
                                                 "total_changes", "changed_sites", "max_changes", "gene_total_changes",
                                                 "gene_total_gains", "gene_total_losses", "min_changes", "excess_changes",
                                                 "homoplasic_sites")] + [("ci", C.c_double)]


PS_NNI_MAX_POP, PS_NNI_NONE = 8192, 2**63 - 1


class NniParams(C.Structure):
    """ps_nni_params: the limits of ps_tree_nni (docs/PARSIMONY_SEARCH.md)"""
    _fields_ = [("max_rounds", C.c_uint32), ("moves_per_round", C.c_uint32)]


class Nni(C.Structure):
    """ps_nni_t: the summary of ps_tree_nni / ps_nni_from_rows"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "sites", "merges", "rounds", "passes", "rollbacks", "moves", "local_optimum",
                                                 "start_changes", "total_changes", "min_changes", "candidates_last")]


# the tree, the parameters, the summary, the returned tree, round_changes, the four move arrays, move_cap: the tail of every ps_*nni entry that searches
_NNI = [C.c_void_p] * 2 + [C.c_uint64, C.POINTER(NniParams), C.POINTER(Nni)] + [C.c_void_p] * 7 + [C.c_uint64]


PS_LIK_MAX_POP, PS_LIK_MIN_LENGTH, PS_LIK_MAX_LENGTH = 2048, 1e-8, 10.0


class MlParams(C.Structure):
    """ps_ml_params: the limits of ps_tree_ml_lengths (docs/TREE_LIKELIHOOD.md)"""
    _fields_ = [("max_rounds", C.c_uint32), ("eps_lnl", C.c_double)]


class Likelihood(C.Structure):
    """ps_likelihood_t: the summary of ps_tree_likelihood / ps_tree_ml_lengths and their host restatements"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "sites", "merges", "clamped_lengths", "missing_cells", "rounds", "passes",
                                                 "rollbacks", "converged")] + \
               [(name, C.c_double) for name in ("lnl", "start_lnl", "tree_length")]


# the tree, the lengths, merges, the summary, site_mant, site_exp, branch_g, branch_h: the tail of every entry that evaluates
_LIK = [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(Likelihood)] + [C.c_void_p] * 4
# the tree, the start lengths, merges, the parameters, the summary, length_out, round_lnl, round_cap: of every entry that optimises
_ML = [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(MlParams), C.POINTER(Likelihood)] + [C.c_void_p] * 2 + [C.c_uint64]


PS_MODEL_MAX_CATEGORIES, PS_MODEL_MAX_POP_DERIV = 8, 1536


class SubstModelC(C.Structure):
    """ps_subst_model: F81 base frequencies, the root distribution, the rate categories and the optional site classes
    (docs/TREE_MODEL.md)"""
    _fields_ = [("freq", C.c_double * 4), ("root", C.c_double * 4), ("categories", C.c_uint32), ("rate", C.c_double * 8),
                ("weight", C.c_double * 8), ("site_class", C.c_void_p), ("site_classes", C.c_uint64)]


class ModelLikelihood(C.Structure):
    """ps_model_likelihood_t: the summary of ps_tree_model_likelihood / ps_tree_model_ml_lengths and their host restatements"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "sites", "merges", "clamped_lengths", "missing_cells", "rounds", "passes",
                                                 "rollbacks", "converged", "categories", "classed")] + \
               [(name, C.c_double) for name in ("lnl", "start_lnl", "tree_length", "beta", "mean_rate")]


# the tree, the lengths, merges, the model, the summary, site_mant, site_exp, site_rate, branch_g, branch_h, branch_q
_MODEL = [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(SubstModelC), C.POINTER(ModelLikelihood)] + [C.c_void_p] * 6
# the tree, the start lengths, merges, the model, the parameters, the summary, length_out, round_lnl, round_cap
_MODEL_ML = [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(SubstModelC), C.POINTER(MlParams), C.POINTER(ModelLikelihood)] + [C.c_void_p] * 2 + [C.c_uint64]


PS_MODEL_NNI_MAX_POP = 1024


class MlNniParams(C.Structure):
    """ps_ml_nni_params: the limits of ps_tree_model_nni (docs/LIKELIHOOD_SEARCH.md)"""
    _fields_ = [("max_rounds", C.c_uint32), ("moves_per_round", C.c_uint32), ("length_rounds", C.c_uint32), ("eps_gain", C.c_double)]


class MlNni(C.Structure):
    """ps_ml_nni_t: the summary of ps_tree_model_nni / ps_model_nni_from_rows"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "sites", "merges", "rounds", "passes", "length_passes", "rollbacks", "moves",
                                                 "local_optimum", "candidates_last", "zero_sites", "clamped_lengths", "missing_cells")] + \
               [(name, C.c_double) for name in ("start_lnl", "lnl")]


# the tree, the lengths, merges, the model, lnl, delta_mant, delta_exp, zero_sites: the tail of every entry that makes one search pass
_MNNI_DELTAS = [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(SubstModelC), C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
# the tree, the start lengths, merges, the model, the parameters, the summary, the returned tree, length_out, round_lnl, the four
# move arrays, move_cap
_MNNI = [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(SubstModelC), C.POINTER(MlNniParams), C.POINTER(MlNni)] + [C.c_void_p] * 8 + [C.c_uint64]


PS_ANC_MAX_POP, PS_ANC_MAX_POP_MIX = 2304, 1536


class Ancestral(C.Structure):
    """ps_ancestral_t: the summary of ps_tree_ancestral_states / ps_ancestral_from_rows (docs/ANCESTRAL_STATES.md)"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "sites", "merges", "categories", "classed", "masked_cells", "zero_sites",
                                                 "missing_cells", "clamped_lengths")] + \
               [(name, C.c_double) for name in ("lnl", "mean_conf", "total_diff")]


# the tree, the lengths, merges, the model, min_posterior, the summary, the new handle (or the host rows), node_conf, branch_diff
_ANC = [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(SubstModelC), C.c_double, C.POINTER(Ancestral)] + [C.c_void_p] * 3


PS_GENE_MAX_POP, PS_GENE_MAX_POP_MIX = 2304, 1792


class GeneModelC(C.Structure):
    """ps_gene_model: the two-state gain / loss chain of the accessory genes: pi, the root distribution, the rate classes and the
    optional gene classes (docs/GENE_MODEL.md)"""
    _fields_ = [("freq", C.c_double * 2), ("root", C.c_double * 2), ("categories", C.c_uint32), ("rate", C.c_double * 8),
                ("weight", C.c_double * 8), ("gene_class", C.c_void_p), ("gene_classes", C.c_uint64)]


class GeneFitParams(C.Structure):
    """ps_gene_fit_params: what ps_tree_gene_fit fits and when it ends"""
    _fields_ = [("fit_rates", C.c_uint32), ("fit_freq", C.c_uint32), ("fit_weights", C.c_uint32), ("max_rounds", C.c_uint32),
                ("eps_lnl", C.c_double)]


class GeneSummary(C.Structure):
    """ps_gene_t: the summary of the ps_tree_gene_* entries and their host restatements"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "genes", "merges", "categories", "classed", "zero_genes", "clamped_lengths",
                                                 "rounds", "passes", "converged")] + \
               [(name, C.c_double) for name in ("lnl", "start_lnl", "beta", "mean_rate", "total_gains", "total_losses", "mean_conf",
                                                "total_genes")]


# the tree, the lengths, merges, the model, the summary: the head of every gene entry; then gene_mant, gene_exp, gene_post, gene_rate
_GENE = [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(GeneModelC), C.POINTER(GeneSummary)]
_GENE_LIK = _GENE + [C.c_void_p] * 4
# ... the new handle (or the host rows), node_conf, node_genes, branch_gains, branch_losses, gene_gains, gene_losses
_GENE_ANC = _GENE + [C.c_void_p] * 7
# the tree, the lengths, merges, the model, the parameters, the summary, rate_out, weight_out, freq_out, round_lnl, round_cap
_GENE_FIT = [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(GeneModelC), C.POINTER(GeneFitParams), C.POINTER(GeneSummary)] + [C.c_void_p] * 4 + [C.c_uint64]


class TreeCompareParams(C.Structure):
    """ps_tree_compare_params"""
    _fields_ = [("bins_a", C.c_uint32), ("bins_b", C.c_uint32), ("span_a", C.c_uint64), ("span_b", C.c_uint64), ("triplets", C.c_int32)]


class TreeCompare(C.Structure):
    """ps_tree_compare_t: the summary of ps_tree_compare / ps_tree_compare_from_merges (docs/TREE_COMPARISON.md)"""
    _fields_ = [(name, C.c_uint64) for name in ("pop_size", "merges_a", "merges_b", "pairs", "joined_both", "joined_a_only",
                                                 "joined_b_only", "joined_neither", "sum_a", "sum_b", "sum_aa", "sum_bb", "sum_ab",
                                                 "triples", "resolved_a", "resolved_b", "shared_triplets", "clades_a", "clades_b",
                                                 "shared_clades", "rf_distance", "bins_a", "bins_b", "span_a", "span_b")] + \
               [(name, C.c_double) for name in ("cophenetic_r", "triplet_recall", "triplet_precision", "clade_recall", "clade_precision")]


# the two trees, the parameters, the summary, joint, in_b, in_a: the tail of every ps_*tree_compare* entry
_TCMP = [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 3 + [C.c_uint64, C.POINTER(TreeCompareParams), C.POINTER(TreeCompare)] + [C.c_void_p] * 3

# every symbol include/pansim_hip.h declares (tests/test_host_logic.py::test_library_exports_every_declared_symbol checks the header against this)
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_vp, _u64, _u32, _i32, _f64, _int = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_double, C.c_int
# ps_exchange_fn: int (*)(void *ctx, void *d_words, uint64_t n_words, void *hip_stream)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)


def _run_forms(name, tail):
    """the entries of a read-out of the regular shape, its arguments behind the handles typed once:
    ps_X(core, acc, tail...), ps_sim_X(sim, tail...) and ps_multi_X(multi, tail...)"""
    return {"ps_" + name: (_int, [_vp, _vp] + tail), "ps_sim_" + name: (_int, [_vp] + tail), "ps_multi_" + name: (_int, [_vp] + tail)}


SIGNATURES = {
    "ps_last_error": (C.c_char_p, []),
    "ps_abi_version": (_int, []),
    "ps_device_count": (_int, []),
    "ps_population_create": (_int, [C.POINTER(Config), _vp, C.POINTER(_vp)]),
    "ps_population_destroy": (None, [_vp]),
    "ps_init_vector": (_int, [_u64, _int, _u64, _u64, _f64, _u8p]),
    "ps_load_matrix": (_int, [_vp, _u8p]),
    "ps_read_matrix": (_int, [_vp, _u8p]),
    "ps_set_rates": (_int, [_vp, _int, _f64p, _f64p, _u64p, _u64p]),
    "ps_set_site_rates": (_int, [_vp, _int, _f64p, _f64p, _vp, _vp]),
    "ps_site_tables": (_int, [_int, _u64, _int, _f64p, _f64p, _vp, _vp, _vp, _vp, _vp]),
    "ps_next_generation": (_int, [_vp, _u32p]),
    "ps_mutate_alleles": (_int, [_vp, _u32]),
    "ps_recombine": (_int, [_vp, _u32]),
    "ps_step": (_int, [_vp, _u32, _u32p, _int]),
    "ps_set_donor_shard": (_int, [_vp, _u32, _u32, _vp, _vp]),
    "ps_sample_indices": (_int, [_vp, _u32, _i32, _f64p, _f64p, _int, _int, _f64, _f64, _u32p]),
    "ps_fitness_terms": (_int, [_vp, _f64p, _i32p, _f64p]),
    "ps_sample_weights": (_int, [_i32p, _f64p, _u64, _u64, _i32, _f64p, _int, _f64, _f64, _f64p]),
    "ps_draw_parents": (_int, [_f64p, _u64, _u64, _u32, _u32p]),
    "ps_average_distance": (_int, [_vp, _f64p]),
    "ps_average_distance_rows": (_int, [_vp, _u64, _u64, _f64p]),
    "ps_pairwise_distances": (_int, [_vp, _u64, _u32p, _u32p, _f64p]),
    "ps_pairwise_counts": (_int, [_vp, _u64, _u32p, _u32p, _vp, _vp, _int]),
    "ps_last_pair_form": (_int, [_vp]),
    "ps_last_sweep_form": (_int, [_vp]),
    "ps_gene_frequencies": (_int, [_vp, _f64p]),
    "ps_site_allele_counts": (_int, [_vp, _vp]),
    "ps_core_diversity": (_int, [_vp, C.POINTER(CoreDiversity), _vp]),
    "ps_diversity_from_counts": (_int, [_vp, _u64, _u64, C.POINTER(CoreDiversity), _vp]),
    "ps_core_diversity_timing": (_int, [_vp, C.POINTER(_f64)]),
    "ps_calc_gene_freq": (_int, [_vp, C.POINTER(_f64)]),
    "ps_write": (_int, [_vp, C.c_char_p]),
    "ps_sync": (_int, [_vp]),
    "ps_set_tuning": (_int, [_vp, C.c_char_p, C.c_int64]),
    "ps_get_tuning": (_int, [_vp, C.c_char_p, C.POINTER(C.c_int64)]),
    "ps_tuning_key": (C.c_char_p, [_u32]),
    "ps_poisson_table": (_u32, [_f64, _u32p, _u32p, _u32]),
    "ps_hamming_bitwise_fast": (_int, [_u8p, _u8p, C.c_size_t, C.POINTER(_u32)]),
    "ps_jaccard_distance_fast": (_int, [_u8p, _u8p, C.c_size_t, C.POINTER(_u32), C.POINTER(_u32)]),
    "ps_standard_deviation": (_int, [_f64p, _u64, C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_int_to_base": (C.c_char, [C.c_uint8]),
    "ps_fmt_f64": (_int, [_f64, C.c_char_p, C.c_size_t]),
    "ps_sim_default_params": (None, [C.POINTER(SimParams)]),
    "ps_sim_validate": (_int, [C.POINTER(SimParams), C.c_char_p, C.c_size_t]),
    "ps_sim_derive": (_int, [C.POINTER(SimParams), C.POINTER(Derived)]),
    "ps_selection_coefficients": (_int, [_u64, _u64, _f64, _f64, _f64, _f64p]),
    "ps_sample_pairs": (_int, [_u64, _u64, _u64, _u32p, _u32p]),
    "ps_reference_selection_coefficients": (_int, [_u64, _u64, _f64, _f64, _f64, _f64p]),
    "ps_chacha_block": (None, [_u32p, _u64, _u64, _int, _u32p]),
    "ps_sim_create": (_int, [C.POINTER(SimParams), C.POINTER(_vp)]),
    "ps_sim_destroy": (None, [_vp]),
    "ps_sim_run": (_int, [_vp, _u32, _u32]),
    "ps_sim_sync": (_int, [_vp]),
    "ps_sim_set_exchange": (_int, [_vp, _vp, _vp]),
    "ps_sim_set_site_weights": (_int, [_vp, _vp, _vp, _vp]),
    "ps_sim_emulate_exchange": (_int, [_vp, _int]),
    "ps_sim_exchange_stats": (_int, [_vp, _int, C.POINTER(_u64), C.POINTER(_u64)]),
    "ps_sim_emulated_link_time": (_int, [_vp, _int, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_rccl_available": (_int, []),
    "ps_rccl_unique_id": (_int, [_u8p]),
    "ps_rccl_exchange_create": (_int, [_u8p, _int, _int, _int, C.POINTER(_vp)]),
    "ps_rccl_exchange_destroy": (None, [_vp]),
    "ps_exchange_rccl": (_int, [_vp, _vp, _u64, _vp]),
    "ps_rccl_exchange_stats": (_int, [_vp, _int, C.POINTER(_u64), C.POINTER(_u64)]),
    "ps_sim_core": (_vp, [_vp]),
    "ps_sim_acc": (_vp, [_vp]),
    "ps_sim_selection": (C.POINTER(_f64), [_vp]),
    "ps_sim_range1": (C.POINTER(_u32), [_vp]),
    "ps_sim_range2": (C.POINTER(_u32), [_vp]),
    "ps_sim_last_parents": (_int, [_vp, _u32p]),
    "ps_sim_sweep_timing": (_int, [_vp, _int, C.POINTER(_u64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_sim_enable_timing": (_int, [_vp, _int]),
    "ps_sim_pairwise_distances": (_int, [_vp, _f64p, _f64p]),
    "ps_sim_distance_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_sim_host_timing": (_int, [_vp, _int, C.POINTER(_u64), C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_sim_save": (_int, [_vp, C.c_char_p, _vp]),
    "ps_sim_load": (_int, [C.c_char_p, C.POINTER(SimParams), C.POINTER(_vp)]),
    "ps_sim_generations_done": (_u32, [_vp]),
    "ps_state_info": (_int, [C.c_char_p, C.POINTER(SimParams), C.POINTER(StateHeader), _vp, _u64]),
    "ps_multi_create": (_int, [C.POINTER(SimParams), _int, C.POINTER(_int), C.POINTER(_vp)]),
    "ps_multi_destroy": (None, [_vp]),
    "ps_multi_shards": (_int, [_vp]),
    "ps_multi_shard": (_vp, [_vp, _int]),
    "ps_multi_run": (_int, [_vp, _u32, _u32]),
    "ps_multi_sync": (_int, [_vp]),
    "ps_multi_pairwise_counts": (_int, [_vp, _u32p]),
    "ps_multi_pairwise_distances": (_int, [_vp, _f64p, _f64p]),
    "ps_multi_average_distance": (_int, [_vp, _int, _f64p]),
    "ps_multi_site_allele_counts": (_int, [_vp, _vp]),
    "ps_multi_core_diversity": (_int, [_vp, C.POINTER(CoreDiversity), _vp]),
    **_run_forms("distance_histogram", [C.POINTER(PairHistParams), C.POINTER(PairHist), _vp]),
    "ps_histogram_from_counts": (_int, [_vp, _vp, _vp, _u64, _u64, _u64, C.POINTER(PairHistParams), C.POINTER(PairHist), _vp]),
    "ps_distance_histogram_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64)]),
    **_run_forms("strain_clusters", [C.POINTER(ClusterParams), C.POINTER(Clusters), _vp]),
    "ps_clusters_from_counts": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _u64, C.POINTER(ClusterParams), C.POINTER(Clusters), _vp]),
    "ps_strain_clusters_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    **_run_forms("linkage_tree", [C.POINTER(TreeParams), C.POINTER(Tree), _vp, _vp, _vp, _vp]),
    "ps_tree_from_counts": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _u64, C.POINTER(TreeParams), C.POINTER(Tree), _vp, _vp, _vp, _vp]),
    "ps_linkage_tree_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    **_run_forms("upgma_tree", [C.POINTER(TreeParams), C.POINTER(Upgma), _vp, _vp, _vp, _vp, _vp]),
    "ps_upgma_from_counts": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _u64, C.POINTER(TreeParams), C.POINTER(Upgma), _vp, _vp, _vp, _vp,
                                    _vp]),
    "ps_upgma_newick": (_int, [_vp, _vp, _vp, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "ps_upgma_tree_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    **_run_forms("neighbour_joining", [C.POINTER(TreeParams), C.POINTER(Nj), _vp, _vp, _vp, _vp]),
    "ps_nj_from_counts": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _u64, C.POINTER(TreeParams), C.POINTER(Nj), _vp, _vp, _vp, _vp]),
    "ps_nj_newick": (_int, [_vp, _vp, _vp, _vp, _u64, _f64, _vp, _u64, C.POINTER(_u64)]),
    "ps_neighbour_joining_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    **_run_forms("bootstrap_support", [C.POINTER(BootstrapParams), _vp, C.POINTER(Bootstrap), _vp, _vp, _vp, _vp]),
    "ps_bootstrap_sites": (_int, [_u64, _u32, _u64, _u64, _u64, _u64, _vp]),
    "ps_bootstrap_from_merges": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _int, _vp, _vp]),
    "ps_bootstrap_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    **_run_forms("nearest_neighbours",[C.POINTER(KnnParams), C.POINTER(Knn), _vp, _vp, _vp]),
    "ps_neighbours_from_counts": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _u64, C.POINTER(KnnParams), C.POINTER(Knn), _vp, _vp, _vp]),
    "ps_lineages_from_neighbours": (_int, [_vp, _u64, C.c_uint32, C.c_uint32, C.POINTER(Lineages), _vp]),
    "ps_nearest_neighbours_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_sim_record_ancestry": (_int, [_vp, _u32]),
    "ps_multi_record_ancestry": (_int, [_vp, _u32]),
    "ps_sim_genealogy": (_int, [_vp, C.POINTER(Genealogy), _vp, _vp]),
    "ps_multi_genealogy": (_int, [_vp, C.POINTER(Genealogy), _vp, _vp]),
    "ps_genealogy_pair": (_int, [_vp, _vp, _u64, _u32, _u32, C.POINTER(_u32)]),
    "ps_genealogy_pairs": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "ps_genealogy_clusters": (_int, [_vp, _vp, _u64, _u32, _u32, _vp, C.POINTER(GenClusters)]),
    "ps_genealogy_newick": (_int, [_vp, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "ps_sim_clock_histogram": (_int, [_vp, C.POINTER(ClockParams), C.POINTER(Clock), _vp, _vp]),
    "ps_multi_clock_histogram": (_int, [_vp, C.POINTER(ClockParams), C.POINTER(Clock), _vp, _vp]),
    "ps_clock_from_counts": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _u64, _u64, C.POINTER(ClockParams), C.POINTER(Clock), _vp, _vp]),
    "ps_clock_histogram_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_locus_ld": (_int, [_vp, C.POINTER(LdParams), _vp, _u32, C.POINTER(Ld), _vp, _vp, _vp, _vp]),
    "ps_sim_locus_ld": (_int, [_vp, C.c_int32, C.POINTER(LdParams), _vp, _u32, C.POINTER(Ld), _vp, _vp, _vp, _vp]),
    "ps_multi_locus_ld": (_int, [_vp, C.c_int32, C.POINTER(LdParams), _vp, _u32, C.POINTER(Ld), _vp, _vp, _vp, _vp]),
    "ps_ld_select_loci": (_int, [_vp, _u64, _u64, _u32, _u32, _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "ps_ld_from_counts": (_int, [_vp, _vp, _vp, _u64, _u64, C.POINTER(LdParams), C.POINTER(Ld), _vp, _vp]),
    "ps_locus_ld_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_gene_site_ld": (_int, [_vp, _vp, C.POINTER(GsParams), _vp, _u32, _vp, _u32, C.POINTER(Gs), C.POINTER(GsSide), C.POINTER(GsSide), _vp, _vp]),
    "ps_sim_gene_site_ld": (_int, [_vp, C.POINTER(GsParams), _vp, _u32, _vp, _u32, C.POINTER(Gs), C.POINTER(GsSide), C.POINTER(GsSide), _vp, _vp]),
    "ps_multi_gene_site_ld": (_int, [_vp, C.POINTER(GsParams), _vp, _u32, _vp, _u32, C.POINTER(Gs), C.POINTER(GsSide), C.POINTER(GsSide), _vp, _vp]),
    "ps_gene_site_from_counts": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, C.POINTER(GsParams), C.POINTER(Gs), C.POINTER(GsSide),
                                        C.POINTER(GsSide), _vp, _vp]),
    "ps_gene_site_ld_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_allele_profiles": (_int, [_vp] + _MLST),
    "ps_sim_allele_profiles": (_int, [_vp] + _MLST),
    "ps_multi_allele_profiles": (_int, [_vp] + _MLST),
    "ps_profiles_from_alleles": (_int, [_vp, _u64, C.POINTER(MlstParams), C.POINTER(Mlst)] + [_vp] * 6),
    "ps_allele_profiles_timing": (_int, [_vp] + [C.POINTER(_f64)] * 5),
    "ps_population_pool": (_int, [_vp, _vp, _vp, _u32, C.POINTER(_vp)]),
    "ps_population_subset": (_int, [_vp, _vp, _u64, C.POINTER(_vp)]),
    "ps_sim_subset": (_int, [_vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_vp)]),
    "ps_multi_subset": (_int, [_vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_vp)]),
    "ps_population_subset_timing": (_int, [_vp, C.POINTER(_f64)]),
    "ps_genealogy_restrict": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp]),
    "ps_groups_from_labels": (_int, [_vp, _u64, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    **_run_forms("group_differentiation", [_vp, C.POINTER(DiffParams), C.POINTER(Diff)] + [_vp] * 12),
    "ps_differentiation_from_counts": (_int, [_vp, _u64, _u32, _vp, C.POINTER(Diff), _vp, _vp, _vp, _vp]),
    "ps_group_differentiation_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    **_run_forms("tree_parsimony", [_vp, _vp, _u64, C.POINTER(Parsimony)] + [_vp] * 8),
    "ps_tree_parsimony_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_merges_from_tree": (_int, [_vp, _vp, _u64, _u64, _vp, _vp, C.POINTER(_u64)]),
    "ps_merges_from_genealogy": (_int, [_vp, _vp, _u64, _vp, _vp, _vp, C.POINTER(_u64)]),
    "ps_parsimony_schedule": (_int, [_vp, _vp, _u64, _u64, _vp, C.POINTER(_u32)]),
    "ps_parsimony_from_rows": (_int, [_vp, _u64, _u64, _int, _vp, _vp, _u64, C.POINTER(Parsimony)] + [_vp] * 8),
    "ps_tree_compare": (_int, [_vp] + _TCMP),
    "ps_sim_tree_compare": (_int, [_vp] + _TCMP),
    "ps_multi_tree_compare": (_int, [_vp] + _TCMP),
    "ps_tree_compare_from_merges": (_int, [_u64] + _TCMP),
    "ps_levels_from_heights": (_int, [_vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "ps_tree_compare_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_tree_nni_deltas": (_int, [_vp, _vp, _vp, _u64, C.POINTER(_u64), _vp]),
    "ps_tree_nni": (_int, [_vp] + _NNI),
    "ps_sim_tree_nni": (_int, [_vp] + _NNI),
    "ps_multi_tree_nni": (_int, [_vp] + _NNI),
    "ps_tree_nni_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_nni_deltas_from_rows": (_int, [_vp, _u64, _u64, _vp, _vp, _u64, C.POINTER(_u64), _vp]),
    "ps_nni_from_rows": (_int, [_vp, _u64, _u64] + _NNI),
    "ps_merges_canonical": (_int, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "ps_nni_apply": (_int, [_vp, _vp, _u64, _u64, _u32, _u32, _vp, _vp]),
    "ps_tree_likelihood": (_int, [_vp] + _LIK),
    "ps_sim_tree_likelihood": (_int, [_vp] + _LIK),
    "ps_multi_tree_likelihood": (_int, [_vp] + _LIK),
    "ps_tree_ml_lengths": (_int, [_vp] + _ML),
    "ps_sim_tree_ml_lengths": (_int, [_vp] + _ML),
    "ps_multi_tree_ml_lengths": (_int, [_vp] + _ML),
    "ps_tree_likelihood_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_likelihood_from_rows": (_int, [_vp, _u64, _u64] + _LIK),
    "ps_ml_lengths_from_rows": (_int, [_vp, _u64, _u64] + _ML),
    "ps_jc_lengths_from_changes": (_int, [_vp, _u64, _u64, _vp]),
    "ps_tree_model_likelihood": (_int, [_vp] + _MODEL),
    "ps_sim_tree_model_likelihood": (_int, [_vp] + _MODEL),
    "ps_multi_tree_model_likelihood": (_int, [_vp] + _MODEL),
    "ps_tree_model_ml_lengths": (_int, [_vp] + _MODEL_ML),
    "ps_sim_tree_model_ml_lengths": (_int, [_vp] + _MODEL_ML),
    "ps_multi_tree_model_ml_lengths": (_int, [_vp] + _MODEL_ML),
    "ps_tree_model_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_model_likelihood_from_rows": (_int, [_vp, _u64, _u64] + _MODEL),
    "ps_model_ml_lengths_from_rows": (_int, [_vp, _u64, _u64] + _MODEL_ML),
    "ps_f81_lengths_from_changes": (_int, [_vp, _u64, _u64, _vp, _vp]),
    "ps_tree_model_nni_deltas": (_int, [_vp] + _MNNI_DELTAS),
    "ps_sim_tree_model_nni_deltas": (_int, [_vp] + _MNNI_DELTAS),
    "ps_multi_tree_model_nni_deltas": (_int, [_vp] + _MNNI_DELTAS),
    "ps_tree_model_nni": (_int, [_vp] + _MNNI),
    "ps_sim_tree_model_nni": (_int, [_vp] + _MNNI),
    "ps_multi_tree_model_nni": (_int, [_vp] + _MNNI),
    "ps_tree_model_nni_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_tree_ancestral_states": (_int, [_vp] + _ANC),
    "ps_sim_tree_ancestral_states": (_int, [_vp] + _ANC),
    "ps_multi_tree_ancestral_states": (_int, [_vp] + _ANC),
    "ps_ancestral_states_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_ancestral_from_rows": (_int, [_vp, _u64, _u64] + _ANC),
    "ps_tree_gene_likelihood": (_int, [_vp] + _GENE_LIK),
    "ps_sim_tree_gene_likelihood": (_int, [_vp] + _GENE_LIK),
    "ps_multi_tree_gene_likelihood": (_int, [_vp] + _GENE_LIK),
    "ps_tree_gene_ancestral": (_int, [_vp] + _GENE_ANC),
    "ps_sim_tree_gene_ancestral": (_int, [_vp] + _GENE_ANC),
    "ps_multi_tree_gene_ancestral": (_int, [_vp] + _GENE_ANC),
    "ps_tree_gene_fit": (_int, [_vp] + _GENE_FIT),
    "ps_sim_tree_gene_fit": (_int, [_vp] + _GENE_FIT),
    "ps_multi_tree_gene_fit": (_int, [_vp] + _GENE_FIT),
    "ps_tree_gene_timing": (_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "ps_gene_likelihood_from_rows": (_int, [_vp, _u64, _u64] + _GENE_LIK),
    "ps_gene_ancestral_from_rows": (_int, [_vp, _u64, _u64] + _GENE_ANC),
    "ps_gene_fit_from_rows": (_int, [_vp, _u64, _u64] + _GENE_FIT),
    "ps_model_nni_deltas_from_rows": (_int, [_vp, _u64, _u64] + _MNNI_DELTAS),
    "ps_model_nni_from_rows": (_int, [_vp, _u64, _u64] + _MNNI),
    "ps_merges_canonical_lengths": (_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "ps_nni_apply_lengths": (_int, [_vp, _vp, _vp, _u64, _u64, _u32, _u32, _vp, _vp, _vp]),
    "ps_multi_set_site_weights": (_int, [_vp, _vp, _vp, _vp]),
    "ps_multi_write": (_int, [_vp, C.c_char_p]),
}

_lib = None


def load():
    """Load libpansim_hip.so; raises if it has not been built (no fallback).

    A process that also uses torch (pansim_amd.distributed, bench.py) must `import torch` BEFORE this call: torch wheels
    bundle their own HIP / HSA / RCCL libraries under the same sonames, and only when they are loaded first does the
    process end up with a single HIP runtime (tests/conftest.py has the details)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libpansim_hip.so is missing at %s: build it with `python -c \"import __graft_entry__ as g; "
            "g.build()\"` (or `make -C pansim_amd/csrc`).  pansim_amd has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != PS_OK:
        raise PansimError(rc, load().ps_last_error().decode(errors="replace"))
    return rc
