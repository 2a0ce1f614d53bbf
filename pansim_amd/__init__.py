"""pansim_amd -- MI355X (gfx950) drop-in for the per-generation hot path of bacpop/Pansim.

The package is a thin host-side mirror of the reference's `Population` API and main() loop
over the C ABI of libpansim_hip.so (include/pansim_hip.h).  All compute runs in hand-written
HIP kernels; there is no CPU fallback and importing the API without the built library fails.
"""
from ._lib import LIB_PATH, PansimError, load  # noqa: F401
from .population import (DistanceHistogram, GroupDifferentiation, LinkageTree, NearestNeighbours, Population, StrainClusters, UpgmaTree, clusters_from_counts, differentiation_from_counts, diversity_from_counts, draw_parents, groups_from_labels,  # noqa: F401
                         fmt_f64, hamming_bitwise_fast, histogram_from_counts, init_vector, int_to_base, jaccard_distance_fast, neighbours_from_counts,
                         sample_weights, site_tables, standard_deviation, tree_from_counts, upgma_from_counts, upgma_newick)
from .linkage import LocusLd, ld_from_counts, ld_select_loci  # noqa: F401
from .association import GeneSiteLd, gene_site_from_counts  # noqa: F401
from .mlst import AlleleProfiles, profiles_from_alleles  # noqa: F401
from .samples import genealogy_restrict, pool  # noqa: F401
from .joining import NeighbourJoiningTree, nj_from_counts, nj_newick  # noqa: F401
from .bootstrap import BootstrapSupport, bootstrap_from_merges, bootstrap_sites  # noqa: F401
from .genealogy import (PS_GEN_BEYOND, ClockHistogram, GenealogyResult, clock_from_counts, genealogy_clusters, genealogy_newick,  # noqa: F401
                        genealogy_pair, genealogy_pairs)
from .parsimony import (PS_PARS_BINS, PS_PARS_MAX_POP, TreeParsimony, merges_from_genealogy, merges_from_tree, parsimony_from_rows,  # noqa: F401
                        parsimony_schedule)
from .search import PS_NNI_MAX_POP, PS_NNI_NONE, ParsimonySearch, merges_canonical, nni_apply, nni_deltas_from_rows, nni_from_rows  # noqa: F401
from .likelihood import (PS_LIK_MAX_LENGTH, PS_LIK_MAX_POP, PS_LIK_MIN_LENGTH, MlLengths, TreeLikelihood, jc_lengths_from_changes,  # noqa: F401
                         likelihood_from_rows, ml_lengths_from_rows)
from .models import (PS_MODEL_MAX_CATEGORIES, PS_MODEL_MAX_POP_DERIV, ModelLikelihood, ModelMlLengths, SubstModel,  # noqa: F401
                     f81_lengths_from_changes, gamma_bounds, gamma_rates, model_likelihood_from_rows, model_ml_lengths_from_rows)
from .ml_search import (PS_MODEL_NNI_MAX_POP, LikelihoodSearch, ModelNniDeltas, merges_canonical_lengths, model_nni_deltas_from_rows,  # noqa: F401
                        model_nni_from_rows, nni_apply_lengths)
from .ancestral import PS_ANC_MAX_POP, PS_ANC_MAX_POP_MIX, AncestralStates, ancestral_from_rows  # noqa: F401
from .gene_model import (PS_GENE_MAX_POP, PS_GENE_MAX_POP_MIX, GeneAncestral, GeneFit, GeneLikelihood, GeneModel,  # noqa: F401
                         gene_ancestral_from_rows, gene_fit_from_rows, gene_likelihood_from_rows)
from .tree_compare import TreeComparison, levels_from_heights, tree_compare_from_merges  # noqa: F401
from .simulation import (DEFAULTS, MultiSimulation, Simulation, derive, make_params, sample_pairs,  # noqa: F401
                         selection_coefficients, state_info, validate)

__version__ = "0.1.0"
