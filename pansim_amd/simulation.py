"""The reference's main() as a library (pansim/src/main.rs:155-553) over the C ABI:
parameter validation/derivation, the seeded host draws and the generation loop.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import Derived, SimParams, StateHeader, check
from .gene_model import _GeneReadouts
from .population import Population, fmt_f64, standard_deviation

# flag names and defaults of main.rs:21-151
DEFAULTS = dict(pop_size=1000, core_size=1200000, pan_genes=6000, core_genes=2000, avg_gene_freq=0.5,
                n_gen=100, max_distances=100000, core_mu=0.05, HR_rate=0.05, HGT_rate=0.05,
                rate_genes1=1.0, rate_genes2=1000.0, prop_genes2=0.1, prop_positive=-0.1,
                pos_lambda=10.0, neg_lambda=10.0, seed=0, genome_size_penalty=0.99,
                competition_strength=0.0, print_dist=0, print_matrices=0, print_selection=0,
                verbose=0, no_control_genome_size=0, shard_rank=0, shard_count=1, device=-1,
                reference_seed_stream=0)


def make_params(**kw):
    p = SimParams()
    _lib.load().ps_sim_default_params(C.byref(p))
    for k, v in kw.items():
        if k not in DEFAULTS:
            raise TypeError("unknown parameter %r" % k)
        setattr(p, k, v)
    return p


def validate(params):
    """main.rs:195-247 -> (ok, stdout text the reference prints before `return Ok(())`)"""
    buf = C.create_string_buffer(2048)
    rc = _lib.load().ps_sim_validate(C.byref(params), buf, 2048)
    return rc == 0, buf.value.decode()


def derive(params):
    """main.rs:259-367"""
    d = Derived()
    check(_lib.load().ps_sim_derive(C.byref(params), C.byref(d)))
    return d


def selection_coefficients(seed, n_genes, prop_positive, pos_lambda, neg_lambda):
    out = np.zeros(n_genes, np.float64)
    check(_lib.load().ps_selection_coefficients(int(seed), int(n_genes), float(prop_positive),
                                                float(pos_lambda), float(neg_lambda), out))
    return out


def sample_pairs(seed, pop_size, max_distances):
    r1 = np.zeros(max_distances, np.uint32)
    r2 = np.zeros(max_distances, np.uint32)
    check(_lib.load().ps_sample_pairs(int(seed), int(pop_size), int(max_distances), r1, r2))
    return r1, r2


def state_info(path, per_gen=False):
    """the header of a state file, no device touched (ps_state_info): dict(params=SimParams, header=StateHeader,
    generations_done, encoding "packed2" / "raw8"; per_gen=True adds per_gen, the (generations_done, 4) rows, or None)"""
    lib = _lib.load()
    p, h = SimParams(), StateHeader()
    check(lib.ps_state_info(os.fsencode(path), C.byref(p), C.byref(h), None, 0))
    out = dict(params=p, header=h, generations_done=int(h.generations_done),
               encoding={_lib.PS_STATE_PACKED2: "packed2", _lib.PS_STATE_RAW8: "raw8"}[h.core_encoding])
    if per_gen:
        out["per_gen"] = None
        if h.has_per_gen:
            rows = np.zeros(max(h.per_gen_bytes // 8, 1))
            check(lib.ps_state_info(os.fsencode(path), None, None, rows.ctypes.data, rows.size))
            out["per_gen"] = rows[:h.per_gen_bytes // 8].reshape(-1, 4)
    return out


class _Readouts:
    """The outputs and read-outs a run has in both of its forms, written once.  Simulation resolves them to the ps_sim_
    entries of the library and MultiSimulation to the ps_multi_ ones (`_prefix`); `_core_width` is the core width of the
    per-site arrays a call returns and `_timed` the Simulation whose core handle holds the device times of the last call."""

    def _entry(self, name):
        return getattr(self._lib, self._prefix + name)

    def run(self, count, first_generation=None):
        """main.rs:429-464 for `count` generations (asynchronous; call sync()) (ps_sim_run / ps_multi_run)"""
        g0 = self.generation if first_generation is None else int(first_generation)
        check(self._entry("run")(self._h, g0, int(count)))
        self.generation = g0 + int(count)

    def sync(self):
        check(self._entry("sync")(self._h))

    # -- outputs of main.rs:467-499 ---------------------------------------------------
    def final_distances(self):
        """main.rs:467-470 (ps_sim_pairwise_distances / ps_multi_pairwise_distances: both matrices' kernels enqueued together)"""
        P = self.params.max_distances
        core, acc = np.zeros(P), np.zeros(P)
        check(self._entry("pairwise_distances")(self._h, core, acc))
        return core, acc

    # -- the read-outs over ALL pairs and sites: behind every queued generation and without a change of state (the run
    # continues as if it had not been asked); rows, labels and leaves in the reference's row order.  Of a sharded run they
    # cover ALL core sites: the shards' band counts, integers and matrices are added on shard 0, their per-site arrays
    # concatenated, and the accessory side comes from shard 0's replica ---------------------------------------------
    def distance_histogram(self, core_bins=64, acc_bins=64, core_max=None, core_span=None):
        """Population.distance_histogram() of the run's two matrices (ps_sim_distance_histogram / ps_multi_distance_histogram)"""
        from .population import _hist_call, _hist_params
        prm = _hist_params(core_bins, acc_bins, core_max, self.params.core_size, core_span)
        return _hist_call(self._entry("distance_histogram"), prm, self._h)

    def strain_clusters(self, core_max=None, acc_max=None, core_max_d=None, acc_ratio=None):
        """Population.strain_clusters() of the run's two matrices (ps_sim_strain_clusters / ps_multi_strain_clusters)"""
        from .population import _cluster_call, _cluster_params
        prm = _cluster_params(self.params.core_size, core_max, acc_max, core_max_d, acc_ratio)
        return _cluster_call(self._entry("strain_clusters"), prm, self.params.pop_size, self._h)

    def group_differentiation(self, labels, max_groups=16, min_size=1, per_site=False, counts=False):
        """Population.group_differentiation() of the run's two matrices (ps_sim_group_differentiation /
        ps_multi_group_differentiation)"""
        from .population import _diff_call
        return _diff_call(self._entry("group_differentiation"), labels, self.params.pop_size, self._core_width,
                          self.pan_genome.ncols, max_groups, min_size, per_site, counts, True, self._h)

    def tree_parsimony(self, left, right, per_site=False, branches=False, genes=False):
        """Population.tree_parsimony() of the run's two matrices (ps_sim_tree_parsimony / ps_multi_tree_parsimony)"""
        from .parsimony import _pars_call
        return _pars_call(self._entry("tree_parsimony"), left, right, self.params.pop_size, self._core_width,
                          self.pan_genome.ncols if genes else 0, per_site, branches, genes, self._h)

    def tree_parsimony_timing(self):
        """device ms of (the schedule's upload, the core pass, the gene pass) of the last tree_parsimony()"""
        return self._timed.core_genome.tree_parsimony_timing()

    def tree_compare(self, a, b, bins=(32, 32), spans=(0, 0), triplets=True, values=None):
        """Population.tree_compare() on the run's core handle, shard 0's of a sharded run: trees are global (ps_sim_tree_compare /
        ps_multi_tree_compare): `tree_compare(genealogy(), upgma_tree())`"""
        from .tree_compare import _compare_call
        return _compare_call(self._entry("tree_compare"), self._h, a, b, bins, spans, triplets, values)

    def tree_compare_timing(self):
        """device ms of (the uploads and the tables, the pass over all pairs) of the last tree_compare()"""
        return self._timed.core_genome.tree_compare_timing()

    def linkage_tree(self, metric="core"):
        """Population.linkage_tree() of the run's two matrices (ps_sim_linkage_tree / ps_multi_linkage_tree)"""
        from .population import _tree_call, _tree_params
        return _tree_call(self._entry("linkage_tree"), _tree_params(metric), self.params.pop_size, self._h)

    def upgma_tree(self, metric="core"):
        """Population.upgma_tree() of the run's two matrices (ps_sim_upgma_tree / ps_multi_upgma_tree)"""
        from .population import _tree_params, _upgma_call
        return _upgma_call(self._entry("upgma_tree"), _tree_params(metric), self.params.pop_size, self._h)

    def nearest_neighbours(self, k, metric="core"):
        """Population.nearest_neighbours() of the run's two matrices (ps_sim_nearest_neighbours / ps_multi_nearest_neighbours)"""
        from .population import _knn_call, _knn_params
        return _knn_call(self._entry("nearest_neighbours"), _knn_params(k, metric), self.params.pop_size, self._h)

    # -- the recorded genealogy (docs/GENEALOGY.md) --------------------------------------
    def record_ancestry(self, capacity):
        """keep the parent draws of the last `capacity` generations on the device (ps_sim_record_ancestry /
        ps_multi_record_ancestry: every shard draws the same parents, shard 0 records alone); 0 switches the recording off.
        The matrices of the run do not change by a bit."""
        check(self._entry("record_ancestry")(self._h, int(capacity)))

    def genealogy(self):
        """the comb of the present population from the recorded draws (ps_sim_genealogy / ps_multi_genealogy) -> a
        GenealogyResult with order, coal, pair(i, j), clusters(t), newick(); rows in the reference's row order"""
        from .genealogy import _genealogy_call
        return _genealogy_call(self._entry("genealogy"), self.params.pop_size, self._h)

    def clock_histogram(self, metric="core", time_bins=32, dist_bins=64, time_span=None, core_max=None, core_span=None):
        """ALL pairs binned by (divergence time from the record, distance) (ps_sim_clock_histogram / ps_multi_clock_histogram)
        -> a ClockHistogram"""
        from .genealogy import _clock_call, _clock_params
        prm = _clock_params(metric, time_bins, dist_bins, time_span, core_max, self.params.core_size, core_span)
        return _clock_call(self._entry("clock_histogram"), prm, self._h)

    def clock_histogram_timing(self):
        """device ms of (the count kernels; the comb, the table and the binning) of the last clock_histogram()"""
        t = [C.c_double(), C.c_double()]
        check(self._lib.ps_clock_histogram_timing(self._lib.ps_sim_core(self._timed._h), *map(C.byref, t)))
        return tuple(x.value for x in t)

    def locus_ld(self, metric="core", r2_bins=64, lag_bins=1, min_minor=1, max_loci=4096, loci=None):
        """linkage disequilibrium between the core sites (every shard selects and packs its own, shard 0 contracts and bins;
        columns are global) or the accessory genes of the run (ps_sim_locus_ld / ps_multi_locus_ld;
        docs/LINKAGE_DISEQUILIBRIUM.md) -> a LocusLd"""
        from .linkage import _ld_call, _ld_params, _metric
        m = _metric(metric)
        return _ld_call(self._entry("locus_ld"), _ld_params(r2_bins, lag_bins, min_minor, max_loci), loci, self._h, m)


class _Associations:
    """The read-outs that pair the run's two matrices along the axis of LOCI, written once for both forms of a run as
    `_Readouts` writes the others (it resolves them through the same `_entry`)."""

    def gene_site_ld(self, r2_bins=64, freq_bins=1, site_min_minor=1, gene_min_minor=1, max_sites=4096, max_genes=4096, strong_q=32768,
                     sites=None, genes=None):
        """Population.gene_site_ld() of the run's two matrices: every shard selects and packs its own sites, shard 0 adds the
        genes of its replica, contracts and bins; columns are global (ps_sim_gene_site_ld / ps_multi_gene_site_ld;
        docs/GENE_SITE_ASSOCIATION.md) -> a GeneSiteLd"""
        from .association import _gs_call, _gs_params
        prm = _gs_params(r2_bins, freq_bins, site_min_minor, gene_min_minor, max_sites, max_genes, strong_q)
        return _gs_call(self._entry("gene_site_ld"), prm, sites, genes, self._h)

    def gene_site_ld_timing(self):
        """device ms of (counts and selection, packing, the contraction, the pair statistics) of the last gene_site_ld()"""
        return self._timed.core_genome.gene_site_ld_timing()


class _Profiles:
    """The read-outs that cut the core matrix into loci, written once for both forms of a run as `_Readouts` writes the others
    (it resolves them through the same `_entry`)."""

    def allele_profiles(self, n_loci, bounds=None, dist_bins=None, complex_max=0, want_profiles=True, key_seed=0, key_bits=64):
        """Population.allele_profiles() of the run's core matrix, all sites: every shard fingerprints the sites it holds, shard 0
        adds the tables, numbers the alleles and runs the pairs (ps_sim_allele_profiles / ps_multi_allele_profiles;
        docs/ALLELE_PROFILES.md) -> an AlleleProfiles"""
        from .mlst import _mlst_device_call
        return _mlst_device_call(self._entry("allele_profiles"), self._h, self.params.pop_size, n_loci, bounds, dist_bins, complex_max,
                                 want_profiles, key_seed, key_bits)

    def allele_profiles_timing(self):
        """device ms of (the fingerprints, the allele numbers, the verification, the pairs, the label rounds) of the last
        allele_profiles()"""
        return self._timed.core_genome.allele_profiles_timing()


class _Samples:
    """Isolate samples of a run, written once for both of its forms as `_Readouts` writes the read-outs (it resolves them through
    the same `_entry`)."""

    def subset(self, rows=None):
        """the rows `rows` (output rows as every read-out numbers them; they may repeat; None = all) of the run's two matrices as
        two new, owned Populations on the device -> (core, acc), to which every read-out of Population applies; the core sample
        of a sharded run holds all sites, on shard 0's device (ps_sim_subset / ps_multi_subset; docs/ISOLATE_SAMPLES.md).  The
        run is not synchronised and continues bit for bit."""
        from .samples import _run_subset
        return _run_subset(self._entry("subset"), self, rows)


class _Joining:
    """The neighbour-joining tree of a run, written once for both of its forms as `_Readouts` writes the other trees (it resolves
    the entry through the same `_entry`)."""

    def neighbour_joining(self, metric="core"):
        """Population.neighbour_joining() of the run's two matrices (ps_sim_neighbour_joining / ps_multi_neighbour_joining;
        docs/NEIGHBOUR_JOINING.md) -> a NeighbourJoiningTree"""
        from .joining import _nj_call
        from .population import _tree_params
        return _nj_call(self._entry("neighbour_joining"), _tree_params(metric), self.params.pop_size, self._h)

    def neighbour_joining_timing(self):
        """device ms of (the count kernels, the store kernels and the row sums, the joins) of the last neighbour_joining()"""
        return self._timed.core_genome.neighbour_joining_timing()


class _Bootstrap:
    """Bootstrap support of a run's trees, written once for both of its forms as `_Joining` writes the neighbour-joining tree."""

    def bootstrap_support(self, method="nj", replicates=100, seed=0, draws=None, sites=None):
        """Population.bootstrap_support() of the run's two matrices (ps_sim_bootstrap_support / ps_multi_bootstrap_support;
        docs/BOOTSTRAP_SUPPORT.md) -> a BootstrapSupport"""
        from .bootstrap import _boot_call, _method
        _method(method)                 # (a ValueError before the library is asked for anything)
        return _boot_call(self._entry("bootstrap_support"), self.params.pop_size, method, replicates, seed, draws, sites, self._h)

    def bootstrap_support_timing(self):
        """device ms of (the site lists, the operands, the trees) of the last bootstrap_support(), summed over its replicates"""
        return self._timed.core_genome.bootstrap_support_timing()


class _Search:
    """The parsimony tree search of a run, written once for both of its forms as `_Bootstrap` writes the bootstrap."""

    def tree_nni(self, left, right, max_rounds=1000, moves_per_round=0):
        """Population.tree_nni() of the run's core matrix (ps_sim_tree_nni / ps_multi_tree_nni; docs/PARSIMONY_SEARCH.md) -> a
        ParsimonySearch"""
        from .search import _nni_call
        return _nni_call(self._entry("tree_nni"), left, right, self.params.pop_size, max_rounds, moves_per_round, self._h)

    def tree_nni_timing(self):
        """device ms of (the uploads of the schedules, the kernels) of the last tree_nni(), summed over its passes"""
        return self._timed.core_genome.tree_nni_timing()


class _Likelihood:
    """The Jukes-Cantor likelihood of a tree of a run in both of its forms (Simulation: ps_sim_, MultiSimulation: ps_multi_)."""

    def tree_likelihood(self, left, right, lengths, per_site=False, derivatives=False):
        """Population.tree_likelihood() of the run's core matrix (ps_sim_tree_likelihood / ps_multi_tree_likelihood;
        docs/TREE_LIKELIHOOD.md) -> a TreeLikelihood"""
        from .likelihood import _lik_call
        return _lik_call(self._entry("tree_likelihood"), left, right, lengths, self.params.pop_size, self._core_width, per_site,
                         derivatives, self._h)

    def tree_ml_lengths(self, left, right, lengths=None, max_rounds=50, eps_lnl=1e-3):
        """Population.tree_ml_lengths() of the run's core matrix (ps_sim_tree_ml_lengths / ps_multi_tree_ml_lengths) -> an
        MlLengths; without `lengths` the start is the Jukes-Cantor correction of the run's tree_parsimony() on the same tree"""
        from .likelihood import _ml_call, _start_lengths
        if lengths is None:
            lengths = _start_lengths(self, left, right)
        return _ml_call(self._entry("tree_ml_lengths"), left, right, lengths, self.params.pop_size, max_rounds, eps_lnl, self._h)

    def tree_likelihood_timing(self):
        """device ms of (the uploads, the kernels, the sums of the rows) of the last tree_likelihood() or tree_ml_lengths()"""
        return self._timed.core_genome.tree_likelihood_timing()

    def tree_model_likelihood(self, left, right, lengths, model, per_site=False, derivatives=False):
        """Population.tree_model_likelihood() of the run's core matrix (ps_sim_tree_model_likelihood /
        ps_multi_tree_model_likelihood; docs/TREE_MODEL.md) -> a ModelLikelihood.  `model.site_class`: one entry per core site of
        the whole run."""
        from .models import _model_call
        return _model_call(self._entry("tree_model_likelihood"), left, right, lengths, model, self.params.pop_size, self._core_width, per_site,
                           derivatives, self._h)

    def tree_model_ml_lengths(self, left, right, model, lengths=None, max_rounds=50, eps_lnl=1e-3):
        """Population.tree_model_ml_lengths() of the run's core matrix (ps_sim_tree_model_ml_lengths /
        ps_multi_tree_model_ml_lengths) -> a ModelMlLengths; without `lengths` the start is the F81 correction of the run's
        tree_parsimony() on the same tree"""
        from .models import _model_ml_call, _model_start_lengths
        if lengths is None:
            lengths = _model_start_lengths(self, left, right, model)
        return _model_ml_call(self._entry("tree_model_ml_lengths"), left, right, lengths, model, self.params.pop_size, max_rounds, eps_lnl, self._h)

    def model_nni_deltas(self, left, right, lengths, model):
        """Population.model_nni_deltas() of the run's core matrix (ps_sim_tree_model_nni_deltas / ps_multi_tree_model_nni_deltas;
        docs/LIKELIHOOD_SEARCH.md) -> a ModelNniDeltas"""
        from .ml_search import _deltas_call
        return _deltas_call(self._entry("tree_model_nni_deltas"), left, right, lengths, model, self.params.pop_size, self._h)

    def tree_model_nni(self, left, right, model, lengths=None, max_rounds=1000, moves_per_round=0, length_rounds=5, eps_gain=1e-3):
        """Population.tree_model_nni() of the run's core matrix (ps_sim_tree_model_nni / ps_multi_tree_model_nni) -> a
        LikelihoodSearch; without `lengths` the start is the F81 correction of the run's parsimony changes"""
        from .ml_search import _search_call
        from .models import _model_start_lengths
        if lengths is None:
            lengths = _model_start_lengths(self, left, right, model)
        return _search_call(self._entry("tree_model_nni"), left, right, lengths, model, self.params.pop_size, max_rounds, moves_per_round,
                            length_rounds, eps_gain, self._h)

    def tree_model_nni_timing(self):
        """device ms of (the uploads, the kernels, the products of the rows) of the search passes of the last tree_model_nni() or
        model_nni_deltas()"""
        return self._timed.core_genome.tree_model_nni_timing()

    def tree_model_timing(self):
        """device ms of (the uploads, the kernels, the sums of the rows) of the last tree_model_likelihood() or tree_model_ml_lengths()"""
        return self._timed.core_genome.tree_model_timing()

    def ancestral_states(self, left, right, lengths, model, min_posterior=0.0, states=True):
        """Population.ancestral_states() of the run's core matrix (ps_sim_tree_ancestral_states / ps_multi_tree_ancestral_states;
        docs/ANCESTRAL_STATES.md) -> an AncestralStates; a sharded run returns one whole Population on shard 0's device.
        `model.site_class`: one entry per core site of the whole run."""
        from .ancestral import _device_call
        return _device_call(self._entry("tree_ancestral_states"), self._timed.core_genome, self._core_width, left, right, lengths, model,
                            self.params.pop_size, min_posterior, states, self._h)

    def ancestral_states_timing(self):
        """device ms of (the uploads, the kernel with its stores, the sums of the rows) of the last ancestral_states()"""
        return self._timed.core_genome.ancestral_states_timing()


class Simulation(_Readouts, _Associations, _Profiles, _Samples, _Joining, _Bootstrap, _Search, _Likelihood, _GeneReadouts):
    """State of main() between main.rs:259 and :553 for one process (one GPU)."""
    _prefix = "ps_sim_"
    _core_width = property(lambda self: self.core_genome.ncols)       # the shard's columns when it is a shard
    _timed = property(lambda self: self)

    def __init__(self, params=None, _handle=None, **kw):
        self._lib = _lib.load()
        self.params = params if params is not None else make_params(**kw)
        self.derived = derive(self.params)
        self._owned = _handle is None
        self._h = C.c_void_p(_handle) if _handle is not None else C.c_void_p()
        if self._owned:
            check(self._lib.ps_sim_create(C.byref(self.params), C.byref(self._h)))
        p, d = self.params, self.derived
        sb = p.core_size * p.shard_rank // p.shard_count
        se = p.core_size * (p.shard_rank + 1) // p.shard_count
        self.core_genome = Population(p.pop_size, se - sb, 4, True, 0.0, p.seed, p.core_genes,
                                      global_cols=p.core_size, _handle=self._lib.ps_sim_core(self._h),
                                      _owned=False)
        self.pan_genome = Population(p.pop_size, d.pan_size, 2, False, d.avg_gene_freq_adj, p.seed,
                                     p.core_genes, _handle=self._lib.ps_sim_acc(self._h), _owned=False)
        P = p.max_distances
        self.range1 = np.ctypeslib.as_array(self._lib.ps_sim_range1(self._h), (P,)).copy()
        self.range2 = np.ctypeslib.as_array(self._lib.ps_sim_range2(self._h), (P,)).copy()
        G = d.pan_size
        self.selection_weights = (np.ctypeslib.as_array(self._lib.ps_sim_selection(self._h), (G,)).copy()
                                  if G else np.zeros(0))
        self.generation = 0

    def close(self):
        # core_genome / pan_genome borrow handles owned by the ps_sim: they die with it
        for name in ("core_genome", "pan_genome"):
            pop = getattr(self, name, None)
            if pop is not None:
                pop._h = C.c_void_p()
        if getattr(self, "_h", None) and self._h.value and self._owned:
            self._lib.ps_sim_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state files (ps_sim_save / ps_sim_load; docs/STATE_FORMAT.md) -----------------
    def save(self, path, per_gen=None):
        """write the state after the last queued generation (waits for it; the run may go on, unperturbed).  `per_gen`:
        (generations_done, 4) doubles kept for the caller (the CLI's _per_gen.tsv rows), or None.  Per-site weights are
        not stored: call set_site_weights again after load()."""
        rows = None
        if per_gen is not None:
            rows = np.ascontiguousarray(per_gen, np.float64).reshape(-1)
            if rows.size != 4 * self.generations_done:
                raise ValueError("per_gen must hold 4 values for each of the %d generations done" % self.generations_done)
            if rows.size == 0:
                rows = np.zeros(1)
        check(self._lib.ps_sim_save(self._h, os.fsencode(path), rows.ctypes.data if rows is not None else None))

    @classmethod
    def load(cls, path, params=None):
        """a Simulation from a state file.  params None: the saved parameters -- run(count) continues the saved run bit
        for bit (self.generation starts at the file's generations_done).  Otherwise a branch: the sizes and the shard
        must be the file's, everything else (seed included) is `params`'."""
        lib = _lib.load()
        h = C.c_void_p()
        check(lib.ps_sim_load(os.fsencode(path), C.byref(params) if params is not None else None, C.byref(h)))
        try:
            if params is None:
                params = SimParams()
                check(lib.ps_state_info(os.fsencode(path), C.byref(params), None, None, 0))
                params.device = -1
            sim = cls(params, _handle=h.value)
        except Exception:
            lib.ps_sim_destroy(h)
            raise
        sim._owned = True
        sim.generation = sim.generations_done
        return sim

    @property
    def generations_done(self):
        """generations_done of the file a loaded run came from; first + count of the last run()"""
        return int(self._lib.ps_sim_generations_done(self._h))

    def last_parents(self):
        out = np.zeros(self.params.pop_size, np.uint32)
        check(self._lib.ps_sim_last_parents(self._h, out))
        return out

    def set_exchange(self, fn, ctx=None):
        """shard the HGT donors over the site shards of this run; `fn` (an _lib.EXCHANGE_FN object, or the address of a
        native ps_exchange_fn such as ps_exchange_rccl with its handle as `ctx`) ORs the shards' delta buffers once per
        generation (ps_sim_set_exchange).  Every shard of the run must install one."""
        self._exchange_fn = fn          # keep the ctypes thunk alive
        check(self._lib.ps_sim_set_exchange(self._h, C.cast(fn, C.c_void_p), ctx))

    def set_site_weights(self, core_weights=None, pan_mutation_weights=None, pan_recombination_weights=None):
        """run the loop with per-site weights (ps_sim_set_site_weights): `core_weights` core_size values;
        the accessory pair (n_comp, pan_size) each, n_comp = derived.n_comp; the rates stay those of the parameters"""
        from .population import _ptr, _weights
        p, d = self.params, self.derived
        wc = _weights(core_weights, 1, p.core_size, "core")
        wm = _weights(pan_mutation_weights, d.n_comp, d.pan_size, "accessory mutation")
        wr = _weights(pan_recombination_weights, d.n_comp, d.pan_size, "accessory recombination")
        check(self._lib.ps_sim_set_site_weights(self._h, _ptr(wc), _ptr(wm), _ptr(wr)))

    def emulate_exchange(self, n_shards):
        """bench.py --emulate-shard: shard 0 of n_shards, exchange stood in for by device-local copies (timing only)"""
        check(self._lib.ps_sim_emulate_exchange(self._h, int(n_shards)))

    def emulated_link_time(self, reset=True):
        """(modelled microseconds of link time charged by the emulated exchange since the last reset, GB/s per link, latency us)"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        check(self._lib.ps_sim_emulated_link_time(self._h, int(reset), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def exchange_stats(self, reset=True):
        """(exchange calls, bytes sent + received by this shard in them) since the last reset -- library providers only"""
        n, b = C.c_uint64(), C.c_uint64()
        check(self._lib.ps_sim_exchange_stats(self._h, int(reset), C.byref(n), C.byref(b)))
        return n.value, b.value

    def enable_timing(self, on=True):
        check(self._lib.ps_sim_enable_timing(self._h, int(on)))

    def sweep_timing(self, reset=True):
        n, ms, b = C.c_uint64(), C.c_double(), C.c_double()
        check(self._lib.ps_sim_sweep_timing(self._h, int(reset), C.byref(n), C.byref(ms), C.byref(b)))
        return n.value, ms.value, b.value

    def host_timing(self, reset=True):
        """(generations, ms waiting for the device half, ms in the softmaxes, ms in the parent draw) since the last reset"""
        n, a, b, c = C.c_uint64(), C.c_double(), C.c_double(), C.c_double()
        check(self._lib.ps_sim_host_timing(self._h, int(reset), C.byref(n), C.byref(a), C.byref(b), C.byref(c)))
        return n.value, a.value, b.value, c.value

    def distance_timing(self):
        """device ms of the core / accessory distance kernels of the last final_distances() call"""
        a, b = C.c_double(), C.c_double()
        check(self._lib.ps_sim_distance_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def write_outputs(self, outpref):
        core, acc = self.final_distances()
        with open(outpref + ".tsv", "w") as f:                       # main.rs:474-482
            f.writelines("%s\t%s\n" % (fmt_f64(c), fmt_f64(a)) for c, a in zip(core, acc))
        with open(outpref + "_freqs.txt", "w") as f:                 # main.rs:487-497
            f.writelines("%s\n" % fmt_f64(x) for x in self.pan_genome.gene_frequencies())
        if self.params.print_matrices:                               # main.rs:550-553
            self.core_genome.write(outpref)
            self.pan_genome.write(outpref)


class MultiSimulation(_Readouts, _Associations, _Profiles, _Samples, _Joining, _Bootstrap, _Search, _Likelihood, _GeneReadouts):
    """The run sharded by core site inside ONE process (ps_multi): shard k on HIP device devices[k]
    (ordinals may repeat), one host thread per shard inside each call; results equal the unsharded run."""
    _prefix = "ps_multi_"
    _core_width = property(lambda self: self.params.core_size)
    _timed = property(lambda self: self.shards[0])

    def __init__(self, params, n_shards, devices=None):
        self._lib = _lib.load()
        self.params = params
        self._h = C.c_void_p()
        dev = None
        if devices is not None:
            dev = (C.c_int * int(n_shards))(*[int(x) for x in devices])
        check(self._lib.ps_multi_create(C.byref(params), int(n_shards), dev, C.byref(self._h)))
        self.n_shards = self._lib.ps_multi_shards(self._h)
        self.shards = []
        for k in range(self.n_shards):
            q = make_params(**{f: getattr(params, f) for f, _ in params._fields_})
            q.shard_rank, q.shard_count = k, self.n_shards
            self.shards.append(Simulation(q, _handle=self._lib.ps_multi_shard(self._h, k)))
        self.range1, self.range2 = self.shards[0].range1, self.shards[0].range2
        self.pan_genome = self.shards[0].pan_genome
        self.generation = 0

    def close(self):
        # the shard wrappers borrow handles owned by the ps_multi: null them first, so that a later use raises
        # a PansimError (null handle) instead of touching freed memory
        for s in getattr(self, "shards", []):
            for pop in (s.core_genome, s.pan_genome):
                pop._h = C.c_void_p()
            s._h = C.c_void_p()
        if getattr(self, "_h", None) and self._h.value:
            self._lib.ps_multi_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def pairwise_counts(self):
        out = np.zeros(self.params.max_distances, np.uint32)
        check(self._lib.ps_multi_pairwise_counts(self._h, out))
        return out

    def average_distance(self, core=True):
        """population.rs:753-784 of the run's core matrix (the shards' counts summed) or of its accessory matrix"""
        out = np.zeros(self.params.pop_size, np.float64)
        check(self._lib.ps_multi_average_distance(self._h, int(bool(core)), out))
        return out

    def site_allele_counts(self):
        """(core_size, 4) uint32: the shards' Population.site_allele_counts() concatenated"""
        from .population import _ptr
        out = np.zeros((self.params.core_size, 4), np.uint32)
        check(self._lib.ps_multi_site_allele_counts(self._h, _ptr(out)))
        return out

    def core_diversity(self, spectrum=False):
        """Population.core_diversity() of the whole core matrix: the shards' integers and spectra added"""
        from .population import _diversity_call
        return _diversity_call(self._lib.ps_multi_core_diversity, self.params.pop_size, spectrum, self._h)

    def write(self, outpref):
        check(self._lib.ps_multi_write(self._h, str(outpref).encode()))


__all__ = ["Simulation", "MultiSimulation", "make_params", "state_info", "validate", "derive", "selection_coefficients", "sample_pairs",
           "DEFAULTS", "standard_deviation"]
