/*
 * pansim_hip.h -- C ABI of libpansim_hip.so, the MI355X (gfx950) drop-in for the
 * per-generation hot path of bacpop/Pansim.
 *
 * The reference has no FFI layer; its library seam is `pub mod population`
 * (pansim/src/lib.rs:4) consumed by main() (pansim/src/main.rs:8).  Every entry
 * point below replaces one item of that seam and cites it.  A Rust host binds
 * this header with `extern "C"` declarations (INTEGRATION.md shows the stub).
 *
 * Conventions
 *  - every function returns 0 on success and a negative ps_status on failure;
 *    ps_last_error() returns the message of the calling thread's last failure.
 *    Nothing aborts or throws across the boundary (the reference panics:
 *    population.rs:440, :484, :562, :584).
 *  - the caller owns every buffer it passes; the library never keeps a caller
 *    pointer after the call returns.  A handle owns its HBM state.
 *  - handles are not thread-safe: one host thread per handle, as all reference
 *    methods take `&mut self`.
 *  - matrices cross the boundary in the reference's layout: one row per
 *    individual, row-major u8 (`Array2<u8>` (N, ncols), population.rs:164-178).
 *    In HBM the core matrix is site-major u8 and the accessory matrix is
 *    bit-packed.
 *  - there is no CPU fallback: without a HIP device every compute call fails
 *    with PS_ERR_NO_DEVICE.
 */
#ifndef PANSIM_HIP_H
#define PANSIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PS_OK = 0,
    PS_ERR_INVALID = -1,    /* bad argument (reference: unwrap()/assert panic) */
    PS_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime failure */
    PS_ERR_OOM = -3,
    PS_ERR_WEIGHTS = -4,    /* WeightedIndex::new would panic (population.rs:440) */
    PS_ERR_IO = -5,
    PS_ERR_STATE = -6       /* call sequence invalid (e.g. rates not set) */
} ps_status;

const char *ps_last_error(void);
/* library ABI version (bumped on any signature change) */
int ps_abi_version(void);
/* number of visible HIP devices, <0 on runtime failure.  Does not create a context. */
int ps_device_count(void);

/* ------------------------------------------------------------------------ */
/* struct Population (population.rs:164-170)                                 */
/* ------------------------------------------------------------------------ */
typedef struct ps_population ps_population;

typedef struct {
    uint64_t pop_size;     /* N: `size` of Population::new (population.rs:182) */
    uint64_t ncols;        /* `allele_count` held by THIS handle (a site shard for core) */
    uint64_t global_cols;  /* full core_size / pan_size (== ncols when not sharded) */
    uint64_t col_offset;   /* global index of local column 0 (site sharding) */
    uint64_t core_genes;   /* population.rs:188 */
    uint64_t seed;         /* --seed (main.rs:180); Philox key */
    int32_t core;          /* population.rs:185: 1 = core alleles, 0 = accessory */
    int32_t device;        /* HIP device ordinal, -1 = current device */
} ps_config;

/* Population::new (population.rs:181-242).  The reference draws ONE random
 * vector and copies it to every individual (clonal start, :206-229); here the
 * caller passes that vector (`init_vec`, ncols bytes; core: 1/2/4/8, accessory:
 * 0/1).  ps_init_vector() below draws it from the build's seeded host stream. */
int ps_population_create(const ps_config *cfg, const uint8_t *init_vec, ps_population **out);
void ps_population_destroy(ps_population *p);

/* Draw the clonal start vector of Population::new (population.rs:199-219):
 * core: 1 << uniform{0..3}; accessory: uniform() < avg_gene_freq.  Columns
 * [col_offset, col_offset+ncols) of the global vector are returned. */
int ps_init_vector(uint64_t seed, int core, uint64_t col_offset, uint64_t ncols,
                   double avg_gene_freq, uint8_t *out);

/* Replace / read the whole matrix, individual-major u8 (N x ncols).  The
 * reference has no such call (its field is private); tests use it to run the
 * deterministic operators on identical state. */
int ps_load_matrix(ps_population *p, const uint8_t *rows);
int ps_read_matrix(ps_population *p, uint8_t *rows);

/* The per-compartment rates the reference passes at every call:
 * `mutations_vec` of mutate_alleles (population.rs:469; main.rs:275-276, :348,
 * :361) and `recombinations_vec` of recombine (population.rs:546; main.rs:279,
 * :349-351, :364-366), with the gene range of each compartment's weight mask
 * (main.rs:342-345, :356-359; core: one compartment [0, global_cols)).  They are
 * set once because the keyed dense form decides mutation and recombination of a
 * cell from one random word. */
int ps_set_rates(ps_population *p, int n_comp, const double *lam_mut, const double *lam_rec,
                 const uint64_t *comp_begin, const uint64_t *comp_end);

/* The same rates with the reference's WEIGHT VECTORS instead of ranges: mutate_alleles draws the column of
 * every event from `weighted_dist[c]` (population.rs:467-471, :503, :527), recombine the accessory gene of an HGT event from
 * `locus_weights[c]` restricted to the donor's present genes (:544-549, :636-680).  w_mut / w_rec: n_comp x global_cols f32,
 * row-major, over the GLOBAL columns even on a site shard (normalisation is global: a shard equals its columns of the whole
 * run bit for bit); n_comp 1..PS_MAX_SITE_COMP.  Column s mutates at rate sum_c lam_mut[c] w_mut[c][s] / W_c (overlapping
 * compartments add); the gene of an HGT event of compartment c is drawn in proportion to w_rec[c][g] among the donor's
 * present genes, weights quantised to 16 bits of the compartment's largest, a gene of weight 0 never, no event if none
 * qualifies (:672); at most 65536 genes.  Core handles: w_rec = NULL -- the reference draws the site of a core HR event
 * uniformly whatever the weights say (:687-689) -- and the lam_rec of the compartments add.  Negative or non-finite weights,
 * and an all-zero vector under a non-zero rate (WeightedIndex::new would panic), fail with PS_ERR_INVALID and a message.
 * When every vector is the 0/1 mask of one contiguous range, w_mut[c] == w_rec[c], the ranges disjoint and n_comp <= 2
 * (core: one compartment, every site 1), this call IS ps_set_rates with those ranges: same plan, same bits.  Rates and
 * weights are state of the handle, set together, for the reason given above; ps_set_rates switches back. */
#define PS_MAX_SITE_COMP 8
int ps_set_site_rates(ps_population *p, int n_comp, const double *lam_mut, const double *lam_rec,
                      const float *w_mut, const float *w_rec);
/* The tables ps_set_site_rates hands to the kernels, computed on the host alone (no device is touched).  plan_out[5]:
 * core k, R, cshift, has_events (accessory: 0), then 1 if the vectors are ranges (the ps_set_rates path).  thr_out: core
 * 7 x global_cols level-2 thresholds (site-major), accessory global_cols flip thresholds.  wq_out (accessory only):
 * n_comp x global_cols quantised HGT weights.  Any output may be NULL. */
int ps_site_tables(int core, uint64_t global_cols, int n_comp, const double *lam_mut, const double *lam_rec,
                   const float *w_mut, const float *w_rec, uint32_t *plan_out, uint32_t *thr_out, uint16_t *wq_out);

/* Population::next_generation(&sample) (population.rs:450-465) */
int ps_next_generation(ps_population *p, const uint32_t *sample);
/* Population::mutate_alleles (population.rs:467-542), generation = loop index j of main.rs:429 */
int ps_mutate_alleles(ps_population *p, uint32_t generation);
/* Population::recombine (population.rs:544-751) */
int ps_recombine(ps_population *p, uint32_t generation);
/* HGT donors sharded over the ranks / shards of one run (the exchange step of the path).  Events are
 * keyed per donor and the recipient's bit is ORed (population.rs:632: the value is always 1), so any partition of the
 * donors gives the unsharded result: this handle generates the events of donors [N r / K, N (r + 1) / K) into a delta
 * buffer of `n_words` u64 (the individual-major bit matrix, zero padded), calls `fn` -- which must leave the bitwise
 * OR of all shards' buffers in every shard's buffer, ordered on `hip_stream` (hipStream_t) -- and ORs the result into
 * its replica of the matrix.  Providers: ps_multi (device-to-device reads between the shards of one process),
 * pansim_amd/distributed.py (torch.distributed: all-to-all + all-gather over RCCL), or any host's own transport.
 * fn == NULL applies the own donors' events only; shard_count == 1 switches sharding off. */
typedef int (*ps_exchange_fn)(void *ctx, void *d_words, uint64_t n_words, void *hip_stream);
int ps_set_donor_shard(ps_population *acc, uint32_t shard_rank, uint32_t shard_count, ps_exchange_fn fn, void *ctx);
/* Fused next_generation + mutate_alleles + recombine in one pass over HBM
 * (main.rs:445-464 for one matrix); bit-identical to the three calls in order.
 * do_recombine mirrors the `HR_rate > 0.0` / `HGT_rate > 0.0` guards (main.rs:459-464). */
int ps_step(ps_population *p, uint32_t generation, const uint32_t *sample, int do_recombine);

/* Population::sample_indices (population.rs:270-448) on the accessory matrix.
 * avg_pairwise_dists: N values (main.rs:435-440).  out_idx: N parent indices. */
int ps_sample_indices(ps_population *acc, uint32_t generation, int32_t avg_gene_num,
                      const double *avg_pairwise_dists, const double *selection_coefficients,
                      int verbose, int no_control_genome_size, double genome_size_penalty,
                      double competition_strength, uint32_t *out_idx);
/* The device half of sample_indices: num_genes (population.rs:282-291) and the
 * per-row log-fitness with the -inf reset (population.rs:299-322). */
int ps_fitness_terms(ps_population *acc, const double *selection_coefficients,
                     int32_t *num_genes, double *logw);
/* The host half: weights (population.rs:293-437), then draws (:440-443). */
int ps_sample_weights(const int32_t *num_genes, const double *logw, uint64_t n, uint64_t n_genes,
                      int32_t avg_gene_num, const double *avg_pairwise_dists,
                      int no_control_genome_size, double genome_size_penalty,
                      double competition_strength, double *weights);
int ps_draw_parents(const double *weights, uint64_t n, uint64_t seed, uint32_t generation,
                    uint32_t *out_idx);

/* Population::average_distance (population.rs:753-784), for both matrices.  Core: population.rs:132-137 over all sites, in
 * output order; a site-shard handle (ncols != global_cols) cannot finish the sum and fails with
 * PS_ERR_INVALID -- ps_multi_average_distance sums the shards. */
int ps_average_distance(ps_population *p, double *out);
/* Rows [first, first + count) of average_distance (count values): what one rank of a row-sharded D-avg computes -- every
 * individual's mean is a sum over ALL others in ascending order (:770), so the rows are independent and a run splits
 * them over its ranks and all-gathers the N doubles. */
int ps_average_distance_rows(ps_population *p, uint64_t first, uint64_t count, double *out);
/* Population::pairwise_distances (population.rs:787-837) */
int ps_pairwise_distances(ps_population *p, uint64_t max_distances, const uint32_t *range1,
                          const uint32_t *range2, double *out);
/* Integer numerators of pairwise_distances for this handle's columns: core:
 * out_a = sum popcount(x^y) (distances.rs:22-52, before the /2 of
 * population.rs:817); accessory: out_a = intersection, out_b = union
 * (distances.rs:55-77).  out_is_device != 0: out_a/out_b are device pointers
 * (site-sharded runs all-reduce them over RCCL). */
int ps_pairwise_counts(ps_population *p, uint64_t max_distances, const uint32_t *range1,
                       const uint32_t *range2, uint32_t *out_a, uint32_t *out_b,
                       int out_is_device);
/* Which kernel form the last core pair-count call of this handle ran in (bench.py prices the distance phase
 * against the roofline of that form): */
enum {
    PS_PAIR_FORM_NONE = 0,
    PS_PAIR_FORM_TILED2 = 1,     /* sampled pairs compared from LDS tiles of the 2-bit packed matrix (VALU bound) */
    PS_PAIR_FORM_ALLPAIRS = 2,   /* all-pairs register tiles, xor + popcount on nibble strings (VALU bound), then lookup */
    PS_PAIR_FORM_TILED4 = 3,     /* sampled pairs from LDS tiles of nibble strings */
    PS_PAIR_FORM_ROWS = 4,       /* matrix transposed once to bit strings, two strings streamed per pair (HBM bound) */
    PS_PAIR_FORM_SIMPLE = 5,     /* one thread per pair on the byte matrix (matrices with bytes above 15) */
    PS_PAIR_FORM_ALLPAIRS_MFMA = 6, /* all-pairs one-hot X X^T on the i8 matrix cores (exact i32 counts), then lookup */
    PS_PAIR_FORM_ALLPAIRS_MFMA_FP4 = 7, /* the same on the block-scaled FP4 path (E2M1 {0, 1}, scales 2^0; exact f32 counts) */
    PS_PAIR_FORM_ALLPAIRS_MFMA_SIGNED = 8 /* FP4 path, three +-1 features per site instead of four {0, 1}: S = 4 matches - sites */
};
int ps_last_pair_form(ps_population *p);
/* Which kernel the last core sweep of this handle (ps_step, ps_next_generation, ps_mutate_alleles, ps_recombine, a
 * generation of ps_sim_run) was launched as -- the library chooses by population width, rates, parent order and the room
 * for a second buffer; bench.py labels and prices its roofline line from this: */
enum {
    PS_SWEEP_FORM_NONE = 0,
    PS_SWEEP_FORM_WAVE = 1,        /* core_sweep_wave_kernel, one wave per site row (N <= 1024) */
    /* 2: a former build of the wave sweep (rounds 3-5); never reported now */
    PS_SWEEP_FORM_WINDOW = 3,      /* core_sweep_window_kernel: N > 1024, children in ascending parent order, out of place */
    PS_SWEEP_FORM_BLOCK = 4,       /* core_sweep_block_kernel: N > 1024, whole rows in workgroup-shared LDS, in place */
    PS_SWEEP_FORM_INLINE = 5       /* core_sweep_inline_kernel: the queue-free form for any rates */
};
int ps_last_sweep_form(ps_population *p);
/* Population::gene_frequencies (population.rs:840-863): ncols + core_genes values */
int ps_gene_frequencies(ps_population *p, double *out);
/* Core allele counts and diversity (docs/CORE_DIVERSITY.md).  The reference has no such function: these are the core
 * counterparts of Population::gene_frequencies (population.rs:840-863), which answers for the accessory matrix only.  One
 * streaming pass over the site-major matrix, ordered on the handle's stream behind every queued generation; column sums do
 * not depend on the row order, so the calls are valid on a simulation's handle at any point.  The classes of a site are A, C,
 * G, T (bytes 1, 2, 4, 8) and `other` (any other byte: only after ps_load_matrix of arbitrary bytes), which counts in no
 * column.  An accessory handle fails with PS_ERR_INVALID (use ps_gene_frequencies).  A site-shard handle (ncols !=
 * global_cols) answers for its own columns, sites = ncols: every field except the double adds across shards. */
typedef struct {
    uint64_t pop_size, sites;          /* N; columns this result covers */
    uint64_t other_cells;              /* cells that are not 1/2/4/8 */
    uint64_t segregating_sites;        /* sites where at least two of the five classes are non-empty */
    uint64_t pair_differences;         /* sum over i<j of differing sites = sum over sites of (N^2 - sum_c n_c^2) / 2 */
    uint64_t base_cells[4];            /* A, C, G, T totals */
    double   mean_pairwise_distance;   /* (double)pair_differences / (double)(N*(N-1)/2) / (double)sites, 0.0 if N < 2 or sites == 0 */
} ps_core_diversity_t;
/* Core counterpart of Population::gene_frequencies (population.rs:840-863; the reference has no such function): counts[4 s + a]
 * = cells of local site s that equal 1 << a, as integers (a frequency is count / pop_size).  counts: ncols x 4. */
int ps_site_allele_counts(ps_population *core, uint32_t *counts);
/* The summary of the same pass without writing the counts (core counterpart of population.rs:840-863; the reference has no such
 * function).  spectrum: pop_size + 1 bins, or NULL -- spectrum[m] = sites whose minor count N - max_c n_c is m. */
int ps_core_diversity(ps_population *core, ps_core_diversity_t *out, uint64_t *spectrum);
/* The same summary from a counts table, on the host alone (no device is touched, as ps_site_tables; the reference has no such
 * function; core counterpart of population.rs:840-863 for tables read back or assembled elsewhere).  counts: sites x 4; a site
 * whose counts exceed pop_size fails with PS_ERR_INVALID. */
int ps_diversity_from_counts(const uint32_t *counts, uint64_t sites, uint64_t pop_size, ps_core_diversity_t *out,
                             uint64_t *spectrum);
/* device time of the counts kernel of the last ps_site_allele_counts / ps_core_diversity call on this handle (HIP events
 * around the launch; no reference counterpart) */
int ps_core_diversity_timing(ps_population *core, double *kernel_ms);
/* Population::calc_gene_freq (population.rs:244-268) */
int ps_calc_gene_freq(ps_population *p, double *out);
/* Population::write (population.rs:865-897): <outpref>_core_genome.csv / _pangenome.csv */
int ps_write(ps_population *p, const char *outpref);
/* wait for all queued device work of this handle */
int ps_sync(ps_population *p);
/* Launch tuning / test hooks (no reference counterpart).  A refused value leaves the switch as it was (PS_ERR_INVALID).  The keys,
 * one per line, in the order of ps_tuning_key:
 *   "sweep_blocks_per_cu"     wave-per-row sweep: resident 256-thread blocks per CU, 1..8
 *   "sweep_rows"              2..4; accepted and ignored since round 6: a wave of that sweep takes the 4 sites of one level-1 block group per iteration
 *   "sweep_out_of_place"      core sweeps: -1 = choose, 0 = update the matrix in place, 1 = write the new generation to a second buffer that then swaps roles with the first, 2 = the same with nontemporal row loads and stores; results are identical
 *   "hgt_apply_threads"       binned HGT: threads per workgroup of the LDS-image pass, 256 / 512 / 1024
 *   "window_blocks_per_cu"    window sweep: workgroups per CU, 0 = choose, 1..8
 *   "davg_form"               average_distance: 0 = choose, 1 = LDS-tile popcount kernels, 2 = intersections on the matrix cores in one kernel -- the choice above pop_size 53248 --, 3 = the same in two phases, u16 counts then division + ordered fold -- the choice for row shards and for 8192 < pop_size <= 53248
 *   "core_davg_form"          average_distance of the core matrix: 0 = choose, 1 = whole matrix -- FP4 all-pairs triangle, then the fold --, 2 = banded -- FP4 rectangle of a band of rows, then the fold --, 3 = generic; matrices that are not one-hot always take 3
 *   "ld_band"                 ps_locus_ld / ps_gene_site_ld: rows of loci per band (rounded up to 64), 0 = choose..65536
 *   "mlst_band"               ps_allele_profiles: loci per band of the fingerprint table, 0 = choose..65535
 *   "gene_team"               gene gain / loss model: threads of a team, 0 = choose, 64 or 256
 *   "gather_form"             isolate samples, on the source: 0 = choose, 1 = source rows staged in LDS, 2 = bytes loaded from global memory
 *   "core_davg_band"          core D-avg, banded forms: rows per band, rounded up to a multiple of 256; 0 = choose
 *   "davg_plain_division"     0/1: matrix-core D-avg: the compiler's f64 division in the epilogue
 *   "davg_ib"                 two-phase D-avg: individuals per workgroup of the division + fold phase, 0 = choose, 16 or 32
 *   "davg_nb"                 matrix-core D-avg: 32-individual fragments per wave, 0 = choose, 1, 2, or -- two-phase form only; the one-kernel form then chooses by itself -- 4
 *   "hgt_mode"                accessory recombination: 0 = choose, 1 = one atomic per event, 2 = two passes: bin by recipient partition, OR in LDS images
 *   "pair_mode"               core distances: 0 = choose by cost, 1 = sampled-pair kernel, 2 = all-pairs tiles + lookup, 3 = sampled-pair kernel in its nibble form even for one-hot matrices, 4 = transposed bit strings streamed per pair -- the sampled form of populations too wide for an LDS tile, 5 = all-pairs xor + popcount tiles even for one-hot matrices, 6 = all pairs on the i8 matrix cores, 7 = all pairs on the FP4 path with three +-1 features per site; one-hot matrices go to the matrix cores in modes 0 and 2 (FP4 form on one-hot nibbles), 6 and 7
 *   "pair_ranges"             site ranges of the tiled sampled-pair kernels, 0 = choose..65535; the 16-bit counter cap still applies
 *   "force_block_sweep"       0/1: use the block sweep even when a row fits one wavefront
 *   "force_inline_sweep"      0/1: use the queue-free inline block sweep
 *   "hgt_slices"              binned HGT: event slices, 0 = choose..4096
 *   "block_batch"             block sweep: segments per wave batch, 0 = choose, 2 or 4
 *   "hgt_bin_cap"             tests: the bins of the binned HGT hold at most this many events, the rest take the overflow image; 0 = sized by the rates
 *   "hgt_events_per_thread"   light HGT kernel inside the generation loop: events a thread handles in sequence -- the launch is that narrow; 0 = whole chip; ps_sim sets it from the estimated sweep time
 *   "window_sweep"            window sweep for pop_size > 1024: -1 = choose, 0 = never (block sweep), 1 = wherever the parents are sorted
 *   "sweep_generations"       core handle of a ps_sim: generations one launch of the wave sweep applies in ps_sim_run, 0 = choose, 1 or 2; only where the wave sweep takes the loop's step -- pop_size <= 1024 -- and only for runs of at least that many generations, everything else keeps one generation per launch; results are identical
 *   "sweep_queue_cap"         tests: the sweeps treat their candidate queues and HR lists as this short, so that the queue-free redo of a batch / row group -- what a full queue falls back to -- runs; 0 = real size
 *   "hgt_list_in_global"      0/1: light HGT: donor gene lists in global scratch instead of LDS
 *   "hgt_bin_list_in_global"  0/1: the same for the bin pass of the binned HGT
 *   "no_block_preload"        0/1: block sweep: parent indices re-read per batch
 *   "block_waves"             block sweep: waves per workgroup, 0 = choose, 4, 8 or 16
 *   "lds_limit"               bytes of LDS a workgroup may use, 1 KiB..160 KiB
 *   "free_cus_per_xcd"        read only (ps_set_tuning does not know it; PANSIM_SWEEP_FREE_CUS at creation): CUs per XCD that the core stream's CU mask leaves to other streams, 0..8
 *   "hgt_bin_prio"            read only (PANSIM_HGT_BIN_PRIO at creation): s_setprio level of the binned HGT's bin pass beside the sweep, 0..3
 * The PANSIM_* environment variables that set a switch when a handle is created are listed in pansim_amd/csrc/tuning.h. */
int ps_set_tuning(ps_population *p, const char *key, int64_t value);
/* The value of a switch as it is now.  An accepted-and-ignored key ("sweep_rows") reads as what the library does whatever was
 * set, 4, not as the last accepted value.  An unknown key: PS_ERR_INVALID. */
int ps_get_tuning(ps_population *p, const char *key, int64_t *value);
/* The key of switch `index` in the order above, NULL past the end.  No handle, no device. */
const char *ps_tuning_key(uint32_t index);

/* ------------------------------------------------------------------------ */
/* free functions of the seam                                                */
/* ------------------------------------------------------------------------ */
/* distances.rs:22-52 and :55-77, computed on the device from host slices */
int ps_hamming_bitwise_fast(const uint8_t *x, const uint8_t *y, size_t n, uint32_t *out);
int ps_jaccard_distance_fast(const uint8_t *x, const uint8_t *y, size_t n, uint32_t *inter,
                             uint32_t *uni);
/* population.rs:87-94: returns (std, mean), population sigma */
int ps_standard_deviation(const double *values, uint64_t n, double *std_out, double *mean_out);
/* population.rs:154-162 */
char ps_int_to_base(uint8_t n);
/* Rust `{}` Display of f64 as used by every writer (main.rs:328, :481, :496, :546) */
int ps_fmt_f64(double v, char *buf, size_t cap);
/* The Poisson sampler behind the per-donor HGT event counts (population.rs:562, :599 use statrs'
 * Poisson; only the distribution is contractual): thr[j] = floor(P(K <= kmin + j) * 2^32) over
 * lambda +- (12 sigma + 12); a 32-bit uniform u gives kmin + #{j : thr[j] <= u}.  Returns the
 * table length, 0 if lambda <= 0 or cap is too small. */
uint32_t ps_poisson_table(double lambda, uint32_t *kmin_out, uint32_t *thr, uint32_t cap);

/* ------------------------------------------------------------------------ */
/* main() as a library: parameter derivation and the generation loop         */
/* ------------------------------------------------------------------------ */
typedef struct {
    uint64_t pop_size, core_size, pan_genes, core_genes;      /* main.rs:155-162 */
    double avg_gene_freq, HR_rate, HGT_rate;                   /* :163-165 */
    int32_t n_gen;                                             /* :166-167 */
    uint64_t max_distances;                                    /* :169 */
    double core_mu, rate_genes1, rate_genes2, prop_genes2;     /* :170-173 */
    double prop_positive, pos_lambda, neg_lambda;              /* :174-176 */
    uint64_t seed;                                             /* :180 */
    int32_t print_dist, print_matrices, print_selection, verbose; /* :178-183 */
    int32_t no_control_genome_size;                            /* :184 */
    double genome_size_penalty, competition_strength;          /* :185-186 */
    /* site sharding: this process holds core sites
     * [core_size*shard_rank/shard_count, core_size*(shard_rank+1)/shard_count) */
    int32_t shard_rank, shard_count;
    int32_t device;                                            /* HIP device, -1 = current */
    /* opt-in, UNPINNED: draw what precedes sample_beta -- the selection coefficients, main.rs:289-319 --
     * from the reference's own seeded stream (rand 0.8.5 StdRng = ChaCha12 after seed_from_u64, rand's Uniform,
     * statrs' ziggurat Exp) instead of the build's Philox stream.  Everything from main.rs:370 on keeps the build's streams. */
    int32_t reference_seed_stream;
} ps_sim_params;

typedef struct {
    uint64_t pan_size;                  /* main.rs:259 */
    double avg_gene_freq_adj;           /* :263-268 */
    int32_t avg_gene_num;               /* :272 */
    double n_core_mutations;            /* :275-276 */
    double n_recombinations_core;       /* :279 */
    double n_recombinations_pan_total;  /* :280 */
    int32_t n_comp;                     /* :341, :355 */
    uint64_t comp_begin[2], comp_end[2];
    double n_pan_mutations[2];          /* :348, :361 */
    double n_recombinations_pan[2];     /* :349-351, :364-366 */
} ps_derived;

void ps_sim_default_params(ps_sim_params *p);                  /* defaults of main.rs:21-151 */
/* main.rs:195-247: 0 if valid; otherwise the reference's stdout text is written to msg */
int ps_sim_validate(const ps_sim_params *p, char *msg, size_t cap);
int ps_sim_derive(const ps_sim_params *p, ps_derived *d);      /* main.rs:259-367 */
/* main.rs:287-319 (build's seeded host stream) */
int ps_selection_coefficients(uint64_t seed, uint64_t n_genes, double prop_positive,
                              double pos_lambda, double neg_lambda, double *out);
/* The same draws from the reference's own seeded stream (ChaCha12 StdRng; see ps_sim_params.reference_seed_stream).
 * Restated from the published algorithms of rand 0.8.5 / rand_chacha 0.3 / statrs 0.16, which are not available here:
 * UNPINNED. */
int ps_reference_selection_coefficients(uint64_t seed, uint64_t n_genes, double prop_positive,
                                        double pos_lambda, double neg_lambda, double *out);
/* the ChaCha block function behind it (rounds = 12 for StdRng; 20 reproduces the RFC 7539 vectors): 16 output words */
void ps_chacha_block(const uint32_t key[8], uint64_t counter, uint64_t stream, int rounds, uint32_t out[16]);
/* main.rs:413-427 */
int ps_sample_pairs(uint64_t seed, uint64_t pop_size, uint64_t max_distances, uint32_t *range1,
                    uint32_t *range2);

typedef struct ps_sim ps_sim;
/* main.rs:259-427: derive, draw selection coefficients, build both populations and the pair list */
int ps_sim_create(const ps_sim_params *p, ps_sim **out);
void ps_sim_destroy(ps_sim *s);
/* main.rs:429-464 for generations [first, first+count): select, gather x2,
 * mutate x2, HR, HGT.  Asynchronous on the device; ps_sim_sync() waits.
 * Row order.  INSIDE, the loop stores the children of a generation in ascending parent order (a stable sort of the N draws
 * of sample_indices, population.rs:440-443: what lets populations wider than one wavefront gather from a ~1 KB window of the
 * parent row).  AT THE BOUNDARY every output of the simulation comes in the reference's order: row k of
 * ps_read_matrix / ps_write / ps_multi_write on the simulation's handles is the child of draw k (main.rs:445-447), the pair
 * list (main.rs:413-427) and ps_pairwise_counts / _distances on those handles name individuals by that row,
 * ps_fitness_terms / ps_average_distance return their vectors in it, ps_sim_last_parents returns the draws in draw order.
 * A direct ps_load_matrix / ps_next_generation / ps_step on a simulation's handle makes the internal order the output order
 * until the simulation's next generation. */
int ps_sim_run(ps_sim *s, uint32_t first_generation, uint32_t count);
int ps_sim_sync(ps_sim *s);
/* Run the loop with per-site weights (ps_set_site_rates on both handles; the rates stay those of the parameters).  w_core:
 * core_size values; w_acc_mut / w_acc_rec: n_comp x pan_size (n_comp of ps_sim_derive), given together.  NULL leaves that
 * matrix as it is.  Call it between runs; it waits for queued generations. */
int ps_sim_set_site_weights(ps_sim *s, const float *w_core, const float *w_acc_mut, const float *w_acc_rec);
/* Shard the HGT donors over the site shards of this run (shard_rank / shard_count of the parameters) and exchange the
 * deltas through `fn` once per generation (ps_set_donor_shard).  Every shard of the run must do the same. */
int ps_sim_set_exchange(ps_sim *s, ps_exchange_fn fn, void *ctx);
/* bench.py --emulate-shard K: play shard 0 of K with the exchange stood in for by device-local copies of the same
 * volume plus a kernel that holds the stream for the time the two collectives would take on one xGMI link each
 * (latency + (K - 1) / K x bytes / link rate per collective; timing only: the other shards' events never arrive). */
int ps_sim_emulate_exchange(ps_sim *s, int n_shards);
/* what the emulation charged: modelled link time (microseconds, accumulated since the last reset) and its parameters */
int ps_sim_emulated_link_time(ps_sim *s, int reset, double *modelled_us, double *link_gbps, double *latency_us);
/* exchange calls and bytes this shard sent + received in them since the last reset */
int ps_sim_exchange_stats(ps_sim *s, int reset, uint64_t *calls, uint64_t *bytes);
/* The native provider of ps_exchange_fn for one process per GPU: the OR over RCCL (all-to-all of the K row slices with
 * ncclSend / ncclRecv, a local OR, ncclAllGather of the merged slices -- RCCL has no OR reduction).  librccl.so is
 * opened with dlopen at the first call; without it these calls fail with PS_ERR_NO_DEVICE (ps_rccl_available() = 0)
 * and nothing else of the library is affected.  Rank 0 draws the id, the host carries its 128 bytes to the other ranks
 * (MPI, a file, a socket), every rank creates its handle (collective: ncclCommInitRank) and installs
 *     ps_sim_set_exchange(sim, ps_exchange_rccl, handle).
 * The reference has no counterpart (one process, rayon threads: main.rs:249-257). */
#define PS_RCCL_ID_BYTES 128
typedef struct ps_rccl_exchange ps_rccl_exchange;
int ps_rccl_available(void);
int ps_rccl_unique_id(uint8_t *id_out /* PS_RCCL_ID_BYTES */);
int ps_rccl_exchange_create(const uint8_t *id, int rank, int world, int device, ps_rccl_exchange **out);
void ps_rccl_exchange_destroy(ps_rccl_exchange *x);
/* a ps_exchange_fn: ctx = the ps_rccl_exchange of this rank */
int ps_exchange_rccl(void *ctx, void *d_words, uint64_t n_words, void *hip_stream);
/* calls and bytes this rank sent + received in them since the last reset */
int ps_rccl_exchange_stats(ps_rccl_exchange *x, int reset, uint64_t *calls, uint64_t *bytes);
ps_population *ps_sim_core(ps_sim *s);
ps_population *ps_sim_acc(ps_sim *s);
const double *ps_sim_selection(ps_sim *s);                     /* pan_size values */
const uint32_t *ps_sim_range1(ps_sim *s);
const uint32_t *ps_sim_range2(ps_sim *s);
/* the draws of the most recent generation in draw order (population.rs:443): out_idx[k] = the output row, in the generation
 * before, of the parent of this generation's output row k */
int ps_sim_last_parents(ps_sim *s, uint32_t *out_idx);
/* Device timing of the core sweep kernel, measured with HIP events on the
 * stream it is launched on, accumulated since the last reset: launches, total
 * milliseconds, and algorithmic bytes per launch (2*N*L_local).  A launch of the
 * wave sweep may carry several generations ("sweep_generations"): it still reads
 * and writes the matrix once, so bytes per launch stay 2*N*L_local and `launches`
 * is smaller than the number of generations (ps_sim_host_timing counts those). */
int ps_sim_sweep_timing(ps_sim *s, int reset, uint64_t *launches, double *total_ms,
                        double *bytes_per_launch);
int ps_sim_enable_timing(ps_sim *s, int on);
/* main.rs:467-470: pairwise_distances of both matrices for the run's pair list (P values each), the two
 * kernel chains enqueued together on their own streams.  With site shards the core distances of this call
 * cover this shard's columns only (ps_multi_pairwise_distances sums the shards' numerators first). */
int ps_sim_pairwise_distances(ps_sim *s, double *core_out, double *acc_out);
/* device time of the distance kernels of the last ps_sim_pairwise_distances call, per matrix (HIP events) */
int ps_sim_distance_timing(ps_sim *s, double *core_ms, double *acc_ms);
/* Host half of sample_indices inside ps_sim_run, accumulated since the last reset: generations, milliseconds
 * spent waiting for the device half (gene counts / log-fitness of the previous accessory chain), in the three
 * softmaxes (population.rs:325-393, libm on the host) and in the parent draw (:440-443: the cumulative table on
 * the host; the N draws on the device for pop_size >= 4096, on the host below). */
int ps_sim_host_timing(ps_sim *s, int reset, uint64_t *generations, double *wait_ms, double *weights_ms,
                       double *draw_ms);

/* ------------------------------------------------------------------------ */
/* state files: save a run, continue it bit for bit, or branch off it        */
/* ------------------------------------------------------------------------ */
/* The reference has no counterpart (a run lives and dies with main()).  Every random decision here is a function of (seed,
 * stream, generation, site, internal row), so the state of a run is its two matrices in INTERNAL row order, the
 * generation number and the row maps of DESIGN.md 3.5; docs/STATE_FORMAT.md specifies the file, DESIGN.md 3.7 the semantics.
 * The core matrix of a simulated population is one-hot and is stored at 2 bits per cell (PS_STATE_PACKED2; packed and
 * unpacked by kernels, in chunks through pinned buffers: no N x L host copy); a matrix that is not one-hot -- bytes loaded with
 * ps_load_matrix -- is stored as it is (PS_STATE_RAW8).  NOT stored: selection coefficients, pair list, plans and tables
 * (functions of the parameters), tuning keys, and the per-site weight vectors, which are state of the handles: call
 * ps_sim_set_site_weights again after ps_sim_load.  One file per ps_sim; a ps_multi run is saved shard by shard,
 * ps_sim_save(ps_multi_shard(m, k), ...), and loaded as one ps_sim per shard. */
enum { PS_STATE_PACKED2 = 1, PS_STATE_RAW8 = 2 };
typedef struct {
    uint32_t version, core_encoding;         /* format version (1); PS_STATE_PACKED2 / PS_STATE_RAW8 */
    uint64_t generations_done;               /* g0: generations [0, g0) have been applied */
    uint64_t pan_size, site_begin, site_end; /* accessory genes; this shard's core sites [site_begin, site_end) */
    uint64_t pitch;                          /* cells per stored core row (pop_size rounded up to 128) */
    uint64_t core_offset, core_bytes, acc_offset, acc_bytes, maps_offset, maps_bytes, per_gen_offset, per_gen_bytes;
    int32_t has_row_maps;                    /* 0: internal order == output order, no last parents (no generation yet) */
    int32_t core_rows_overridden, acc_rows_overridden;   /* a direct ps_load_matrix / ps_step made that handle's orders coincide */
    int32_t has_per_gen;                     /* a per-generation section (4 doubles per generation) is present */
} ps_state_header;
/* Write the state of the run after its last queued generation (waits for it; the run may go on afterwards, unperturbed).
 * per_gen: 4 x generations_done doubles kept for the caller (the CLI's _per_gen.tsv rows), or NULL. */
int ps_sim_save(ps_sim *s, const char *path, const double *per_gen);
/* A new ps_sim from a file.  params == NULL: the saved parameters (on the current device) -- ps_sim_run(s, g0, count) then
 * continues the saved run bit for bit.  params != NULL: a BRANCH -- pop_size, core_size, pan_genes, core_genes (hence
 * pan_size), shard_rank and shard_count must equal the file's (else PS_ERR_INVALID, the message names the field);
 * everything else, the seed included, is the caller's: selection coefficients, pair list, rates and plans are derived from
 * `params`.  Unreadable / short file, bad magic or version, checksum mismatch: PS_ERR_IO, the message names the section.
 * A failed load leaves no handle and no device memory behind. */
int ps_sim_load(const char *path, const ps_sim_params *params, ps_sim **out);
/* g0 of a loaded run; first + count of the last ps_sim_run */
uint32_t ps_sim_generations_done(ps_sim *s);
/* The header of a file, no device touched (as ps_site_tables): saved parameters, generations_done, encoding, section sizes.
 * per_gen_out (cap doubles; may be NULL): the per-generation section, checksum verified.  Any output may be NULL. */
int ps_state_info(const char *path, ps_sim_params *params_out, ps_state_header *hdr_out, double *per_gen_out, uint64_t cap);

/* ------------------------------------------------------------------------ */
/* one process, several devices: the run sharded by core site  */
/* ------------------------------------------------------------------------ */
/* main() of the reference is one process (main.rs:429-553).  ps_multi holds one ps_sim per site shard,
 * shard k on HIP device devices[k] (null: k modulo the visible devices; ordinals may repeat, i.e. several
 * shards on one GPU), each driven by its own host thread inside a call.  A generation needs no exchange
 * between the shards; the distance phase sums the shards' integer Hamming numerators on shard 0's device
 * (device-to-device copies).  All results equal those of the unsharded run bit for bit. */
typedef struct ps_multi ps_multi;
int ps_multi_create(const ps_sim_params *p, int n_shards, const int *devices, ps_multi **out);
void ps_multi_destroy(ps_multi *m);
int ps_multi_shards(ps_multi *m);
/* borrowed, for reading: selection coefficients, pair list, matrices, timings.  A shard's generations and its HGT take
 * part in exchanges between ALL shards (parent weights, HGT deltas): ps_sim_run / ps_recombine on a borrowed shard fail
 * with PS_ERR_STATE -- drive the shards through ps_multi_run. */
ps_sim *ps_multi_shard(ps_multi *m, int k);
/* main.rs:429-464 for generations [first, first+count) on every shard */
int ps_multi_run(ps_multi *m, uint32_t first_generation, uint32_t count);
int ps_multi_sync(ps_multi *m);
/* population.rs:787-837 for the run's pair list: core numerators summed over the shards (out_core: P values) */
int ps_multi_pairwise_counts(ps_multi *m, uint32_t *out_core);
/* main.rs:467-470: core and accessory distances of the run's pair list (P values each) */
int ps_multi_pairwise_distances(ps_multi *m, double *core_out, double *acc_out);
/* population.rs:753-784 of the run's core matrix (core != 0: every shard counts its sites, shard 0 adds and folds; the tuning
 * keys of shard 0's core handle apply) or of its accessory matrix (core == 0: shard 0's replica).  out: pop_size values. */
int ps_multi_average_distance(ps_multi *m, int core, double *out);
/* ps_site_allele_counts / ps_core_diversity of the run's core matrix (core counterparts of population.rs:840-863; the reference
 * has no such function): the shards' counts concatenated (counts: core_size x 4), their integers and spectra added, the
 * double formed once over core_size. */
int ps_multi_site_allele_counts(ps_multi *m, uint32_t *counts);
int ps_multi_core_diversity(ps_multi *m, ps_core_diversity_t *out, uint64_t *spectrum);
/* ps_sim_set_site_weights for a ps_multi run is NOT plumbed yet: always PS_ERR_INVALID, with a message that says what to do
 * instead (one ps_sim per shard). */
int ps_multi_set_site_weights(ps_multi *m, const float *w_core, const float *w_acc_mut, const float *w_acc_rec);
/* main.rs:550-553: <outpref>_core_genome.csv (lines assembled from the shards' columns) and _pangenome.csv */
int ps_multi_write(ps_multi *m, const char *outpref);

/* Joint core x accessory distance histogram over ALL N (N - 1) / 2 unordered pairs (docs/DISTANCE_HISTOGRAM.md).  The reference
 * has no such function: it writes a SAMPLE of pairs as text (population.rs:787-837) and bins the text afterwards
 * (scripts/plot_distances.R).  Per pair i < j, in integers: core d = h / 2 (h as ps_pairwise_counts returns it),
 * bin_c = min(core_bins - 1, floor(d core_bins / core_span)), a pair with d >= core_span counted in core_clamped; accessory
 * a = U - I, b = U + core_genes, bin_a = min(acc_bins - 1, floor(a acc_bins / b)), a pair with b == 0 (the reference's NaN)
 * in no bin and counted in undefined_pairs.  joint[bin_c * acc_bins + bin_a] (core_bins x acc_bins values); the moments
 * cover all pairs, undefined ones included.  1 <= core_bins, acc_bins; core_bins x acc_bins <= 16384; pop_size >= 2; at most
 * 65535 accessory genes: anything else is PS_ERR_INVALID.  Results do not depend on the launch geometry. */
typedef struct {
    uint32_t core_bins, acc_bins;
    uint64_t core_span;                /* S >= 1 in units of d; 0 = automatic: core_d_max + 1 (a first pass without binning) */
} ps_pair_hist_params;
typedef struct {
    uint64_t pop_size, pairs, core_sites, core_genes;      /* pop_size is 0 from ps_histogram_from_counts */
    uint32_t core_bins, acc_bins;
    uint64_t core_span;                /* the span used */
    uint64_t undefined_pairs, core_clamped;
    uint64_t core_d_min, core_d_max, core_d_sum, core_d_sqsum_lo, core_d_sqsum_hi;      /* sum of d^2 = hi 2^64 + lo */
    double   mean_core_distance;       /* (double)core_d_sum / (double)pairs / (double)core_sites, 0.0 if core_sites == 0 */
} ps_pair_hist_t;
/* All pairs of two handles of equal pop_size on one device (the reference has no such function; replaces population.rs:787-837 +
 * scripts/plot_distances.R): `core` a core handle that holds all sites, `acc` an accessory handle.  Ordered behind all queued
 * work of BOTH handles; changes no state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible. */
int ps_distance_histogram(ps_population *core, ps_population *acc, const ps_pair_hist_params *prm, ps_pair_hist_t *out,
                          uint64_t *joint);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:787-837 +
 * scripts/plot_distances.R); a site shard fails with a message that points to ps_multi_distance_histogram */
int ps_sim_distance_histogram(ps_sim *s, const ps_pair_hist_params *prm, ps_pair_hist_t *out, uint64_t *joint);
/* The same for a sharded run (the reference has no such function; population.rs:787-837 + scripts/plot_distances.R): every
 * shard counts its own sites band by band, shard 0 adds, halves and bins against its accessory replica */
int ps_multi_distance_histogram(ps_multi *m, const ps_pair_hist_params *prm, ps_pair_hist_t *out, uint64_t *joint);
/* The same integer rules on the host alone (no device is touched, as ps_diversity_from_counts; the reference has no such
 * function; population.rs:787-837 + scripts/plot_distances.R): bins any list of pair numerators, e.g. ps_pairwise_counts'.
 * n_pairs >= 1; an intersection above its union is PS_ERR_INVALID. */
int ps_histogram_from_counts(const uint32_t *core_h, const uint32_t *acc_inter, const uint32_t *acc_union, uint64_t n_pairs,
                             uint64_t core_sites, uint64_t core_genes, const ps_pair_hist_params *prm, ps_pair_hist_t *out,
                             uint64_t *joint);
/* device ms of the last ps_distance_histogram on this core handle (HIP events; no reference counterpart): the count kernels
 * of both matrices, and the binning kernel (with the moments pass of an automatic span) */
int ps_distance_histogram_timing(ps_population *core, double *counts_ms, double *binning_ms);

/* Strain clusters: the connected components of the graph over ALL N individuals whose edges are the pairs closer than a
 * threshold (docs/STRAIN_CLUSTERS.md).  The reference has no such function: it writes a SAMPLE of pairs as text
 * (population.rs:787-837) and the clusters are read off the plotted cloud (scripts/plot_distances.R).  Per pair i < j, in
 * integers, with the numerators of the distance histogram: core criterion d = h / 2 <= core_max_d; accessory criterion
 * a = U - I, b = U + core_genes, b != 0 and a acc_den <= acc_num b (a pair with b == 0, the reference's NaN, is never an edge
 * and is counted in undefined_pairs).  Equality is an edge.  A pair is an edge iff every active criterion holds; at least one
 * must be active and acc_num <= acc_den <= 2^24, else PS_ERR_INVALID.  labels[k] (pop_size values, the reference's row order) =
 * the smallest row of k's cluster.  Results do not depend on the launch geometry. */
typedef struct {
    uint64_t core_max_d;               /* in units of d; UINT64_MAX = no core criterion */
    uint32_t acc_num, acc_den;         /* distance a / b <= acc_num / acc_den; acc_den == 0 = no accessory criterion */
} ps_cluster_params;
typedef struct {
    uint64_t pop_size, pairs, core_sites, core_genes;      /* pairs: all N (N - 1) / 2, or the list's length from ps_clusters_from_counts */
    uint64_t edges, clusters, singletons, largest_cluster;
    uint64_t within_pairs;             /* sum over the clusters of size (size - 1) / 2 */
    uint64_t undefined_pairs;          /* pairs with b == 0; counted only while the accessory criterion is active */
    uint64_t rounds;                   /* label rounds taken on the device (informational; 0 from ps_clusters_from_counts) */
} ps_cluster_t;
/* All pairs of two handles of equal pop_size >= 2 on one device (the reference has no such function; replaces
 * population.rs:787-837 + scripts/plot_distances.R): `core` a core handle that holds all sites, `acc` an accessory handle of at
 * most 65535 genes (required; without an accessory criterion none of its kernels is launched).  Ordered behind all queued work
 * of BOTH handles; changes no state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible. */
int ps_strain_clusters(ps_population *core, ps_population *acc, const ps_cluster_params *prm, ps_cluster_t *out, uint32_t *labels);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:787-837 +
 * scripts/plot_distances.R); a site shard fails with a message that points to ps_multi_strain_clusters */
int ps_sim_strain_clusters(ps_sim *s, const ps_cluster_params *prm, ps_cluster_t *out, uint32_t *labels);
/* The same for a sharded run (the reference has no such function; population.rs:787-837 + scripts/plot_distances.R): every
 * shard counts its own sites band by band, shard 0 adds them and computes edges and labels against its accessory replica */
int ps_multi_strain_clusters(ps_multi *m, const ps_cluster_params *prm, ps_cluster_t *out, uint32_t *labels);
/* The same integer rule on the host alone (no device is touched, as ps_histogram_from_counts; the reference has no such
 * function; population.rs:787-837 + scripts/plot_distances.R): union-find over any list of pairs (r1[k], r2[k]) with their
 * numerators (those of an inactive criterion may be NULL), labels in the list's own index space.  An intersection above its
 * union, an index >= pop_size or r1[k] == r2[k] is PS_ERR_INVALID. */
int ps_clusters_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter,
                            const uint32_t *acc_union, uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites, uint64_t core_genes,
                            const ps_cluster_params *prm, ps_cluster_t *out, uint32_t *labels);
/* device ms of the last ps_strain_clusters on this core handle (HIP events; the reference has no such function;
 * population.rs:787-837 + scripts/plot_distances.R): the count kernels of both matrices, the edge kernel, the label rounds
 * (host round trips included).  PS_ERR_STATE before any call. */
int ps_strain_clusters_timing(ps_population *core, double *counts_ms, double *edges_ms, double *labels_ms);

/* Single-linkage tree: the minimum spanning tree of the complete graph over ALL N individuals under one distance
 * (docs/LINKAGE_TREE.md) -- the single-linkage dendrogram, whose N - 1 sorted edge weights are the merge heights; cutting it at
 * any threshold gives the labels of ps_strain_clusters at that threshold.  The reference has no such function: it writes a
 * SAMPLE of pairs as text (population.rs:787-837), and a sample cannot give a spanning tree.  Per pair i < j, in integers, with
 * the numerators of the distance histogram: core metric num = d = h / 2, den = core sites; accessory metric num = a = U - I,
 * den = b = U + core_genes, a pair with b == 0 (the reference's NaN) reported as 0 / 0, above every defined distance and equal
 * to every other undefined one.  Two distances compare by num1 den2 against num2 den1 in u64 (equal denominators: by the
 * numerators); no floating point.  Edges are ordered by (distance, lo, hi), lo < hi rows of the reference's row order: the order
 * is strict, the tree is unique and does not depend on the launch geometry.  The accessory metric needs at most 65535 accessory
 * genes and core_genes + 65535 < 2^32, else PS_ERR_INVALID. */
#define PS_TREE_CORE 0
#define PS_TREE_ACC 1
typedef struct {
    int32_t metric;                    /* PS_TREE_CORE or PS_TREE_ACC */
} ps_tree_params;
typedef struct {
    uint64_t pop_size, pairs, core_sites, core_genes;      /* pairs: all N (N - 1) / 2, or the list's length from ps_tree_from_counts */
    uint64_t metric;
    uint64_t edges;                    /* pop_size - 1, or fewer from a list that leaves a forest */
    uint64_t undefined_edges;          /* tree edges with den == 0 */
    uint64_t distinct_heights;         /* distinct distances among the edges */
    uint64_t rounds;                   /* Boruvka rounds taken on the device (informational; 0 from ps_tree_from_counts) */
} ps_tree_t;
/* All pairs of two handles of equal pop_size >= 2 on one device (the reference has no such function; population.rs:787-837
 * writes a sample): `core` a core handle that holds all sites, `acc` an accessory handle of at most 65535 genes (required; with
 * the core metric none of its kernels is launched).  lo, hi, num, den: pop_size - 1 values each, in ascending order of
 * (distance, lo, hi).  Ordered behind all queued work of BOTH handles; changes no state.  PS_ERR_NO_DEVICE before anything
 * else when no GPU is visible. */
int ps_linkage_tree(ps_population *core, ps_population *acc, const ps_tree_params *prm, ps_tree_t *out, uint32_t *lo, uint32_t *hi,
                    uint64_t *num, uint64_t *den);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:787-837); a site shard
 * fails with a message that points to ps_multi_linkage_tree */
int ps_sim_linkage_tree(ps_sim *s, const ps_tree_params *prm, ps_tree_t *out, uint32_t *lo, uint32_t *hi, uint64_t *num, uint64_t *den);
/* The same for a sharded run (the reference has no such function; population.rs:787-837): every shard counts its own sites
 * band by band, shard 0 adds them, keeps them and runs the rounds against its accessory replica */
int ps_multi_linkage_tree(ps_multi *m, const ps_tree_params *prm, ps_tree_t *out, uint32_t *lo, uint32_t *hi, uint64_t *num, uint64_t *den);
/* The same order on the host alone (no device is touched, as ps_clusters_from_counts; the reference has no such function;
 * population.rs:787-837): Kruskal over any list of pairs (r1[k], r2[k]) with their numerators (those of the other metric may
 * be NULL), in the list's own index space.  Duplicate pairs are allowed; a list that does not connect all of pop_size gives
 * the minimum spanning forest, out->edges < pop_size - 1 (the arrays still have room for pop_size - 1).  An index >= pop_size,
 * r1[k] == r2[k] or, under the accessory metric, an intersection above its union or a union above 65535 is PS_ERR_INVALID. */
int ps_tree_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter,
                        const uint32_t *acc_union, uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites, uint64_t core_genes,
                        const ps_tree_params *prm, ps_tree_t *out, uint32_t *lo, uint32_t *hi, uint64_t *num, uint64_t *den);
/* device ms of the last ps_linkage_tree on this core handle (HIP events; the reference has no such function;
 * population.rs:787-837): the count kernels of the metric, the store kernels, the rounds (host round trips included).
 * PS_ERR_STATE before any call. */
int ps_linkage_tree_timing(ps_population *core, double *counts_ms, double *store_ms, double *rounds_ms);

/* Average-linkage (UPGMA) tree: the dendrogram of ALL N individuals under one distance in which the distance of two clusters is
 * the average over all their cross pairs (docs/UPGMA_TREE.md) -- under a strict clock the consistent estimator of the genealogy
 * that ps_sim_genealogy records.  The reference has no such function: it writes a SAMPLE of pairs as text
 * (population.rs:787-837), from which no tree can be built.  In integers, with the numerators of the distance histogram and the
 * metrics of the linkage tree (ps_tree_params as it is): a cluster's id is its smallest row; the distance of clusters A, B is
 * num / den with, core metric, num = sum of d = h / 2 over A x B and den = |A| |B| core_sites, accessory metric, num = sum of
 * a = U - I and den = sum of b = U + core_genes (the pooled distance).  Two distances compare by num1 den2 against num2 den1 in 128
 * bits; no floating point.  The tree is the one of the sequential algorithm: N - 1 times, merge the pair of clusters that is
 * smallest under (distance, lo id, hi id); the order is strict, so the tree is unique and does not depend on the launch geometry.
 * Merge k (in the order the sequential algorithm performs them) creates node pop_size + k, the leaves being the rows 0 ..
 * pop_size - 1: left[k], right[k] its children (left: the cluster with the smaller id), size[k] its members, num[k] / den[k]
 * its distance, non-decreasing in k -- scipy's linkage matrix with exact fractions.  Limits, else PS_ERR_INVALID: pop_size <=
 * 16384 (every sum below 2^58); under the accessory metric core_genes >= 1 (no pair is 0 / 0), at most 65535 accessory genes and
 * core_genes + 65535 < 2^32. */
typedef struct {
    uint64_t pop_size, pairs, core_sites, core_genes;      /* pairs: all N (N - 1) / 2 */
    uint64_t metric;
    uint64_t merges;                   /* pop_size - 1 */
    uint64_t distinct_heights;         /* distinct distances among the merges */
    uint64_t root_num, root_den;       /* the distance of the last merge */
    uint64_t rounds;                   /* rounds of mutual nearest neighbours on the device (informational; 0 from ps_upgma_from_counts) */
} ps_upgma_t;
/* All pairs of two handles of equal pop_size >= 2 on one device (the reference has no such function; population.rs:787-837
 * writes a sample): `core` a core handle that holds all sites, `acc` an accessory handle of at most 65535 genes (required; with
 * the core metric none of its kernels is launched).  left, right, size, num, den: pop_size - 1 values each.  Ordered behind all
 * queued work of BOTH handles; changes no state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible. */
int ps_upgma_tree(ps_population *core, ps_population *acc, const ps_tree_params *prm, ps_upgma_t *out, uint32_t *left, uint32_t *right,
                  uint32_t *size, uint64_t *num, uint64_t *den);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:787-837); a site shard
 * fails with a message that points to ps_multi_upgma_tree */
int ps_sim_upgma_tree(ps_sim *s, const ps_tree_params *prm, ps_upgma_t *out, uint32_t *left, uint32_t *right, uint32_t *size, uint64_t *num,
                      uint64_t *den);
/* The same for a sharded run (the reference has no such function; population.rs:787-837): every shard counts its own sites
 * band by band, shard 0 adds them, keeps them and runs the rounds against its accessory replica */
int ps_multi_upgma_tree(ps_multi *m, const ps_tree_params *prm, ps_upgma_t *out, uint32_t *left, uint32_t *right, uint32_t *size,
                        uint64_t *num, uint64_t *den);
/* The sequential algorithm on the host alone (no device is touched; the reference has no such function;
 * population.rs:787-837; O(pop_size^3) at worst): over the COMPLETE list of pairs (r1[k], r2[k]) with their numerators (those of the other
 * metric may be NULL), in any order and orientation.  A missing or duplicate pair (average linkage is undefined on a partial
 * list), an index >= pop_size, r1[k] == r2[k], an intersection above its union and the metric's limits are PS_ERR_INVALID. */
int ps_upgma_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter,
                         const uint32_t *acc_union, uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites, uint64_t core_genes,
                         const ps_tree_params *prm, ps_upgma_t *out, uint32_t *left, uint32_t *right, uint32_t *size, uint64_t *num,
                         uint64_t *den);
/* The tree as one line of Newick text (host only; the reference has no such function; population.rs:787-837): leaves are rows,
 * children left then right, "(child:len,child:len)" up to the closing ";", len = 0.5 * ((double)num / den of the parent - that
 * of the child), a leaf's distance being 0, written with ps_fmt_f64.  `needed` counts the terminating zero; buf == NULL asks for
 * the size alone, a buffer below it is PS_ERR_INVALID. */
int ps_upgma_newick(const uint32_t *left, const uint32_t *right, const uint64_t *num, const uint64_t *den, uint64_t pop_size, char *buf,
                    uint64_t cap, uint64_t *needed);
/* device ms of the last ps_upgma_tree on this core handle (HIP events; the reference has no such function;
 * population.rs:787-837): the count kernels of the metric, the store kernels, the rounds (host round trips included).
 * PS_ERR_STATE before any call. */
int ps_upgma_tree_timing(ps_population *core, double *counts_ms, double *store_ms, double *rounds_ms);

/* Neighbour-joining tree (Saitou & Nei 1987 in the Studier-Keppler form; docs/NEIGHBOUR_JOINING.md): the tree of ALL N individuals
 * from one distance without the assumption of a clock -- it recovers any additive (tree) metric exactly.  The reference has no
 * such function: it writes a SAMPLE of pairs as text (population.rs:787-837), from which no tree can be built.  The metrics are
 * those of the linkage tree (ps_tree_params as it is); every distance is an IEEE-754 binary64: core metric d = (double)(h / 2),
 * an exact integer in differing sites; accessory metric d = (double)a / (double)b with a = U - I and b = U + core_genes, one
 * correctly rounded division.  A node's id is the smallest row among its leaves.  Start: r_i = the sum of d(i, k) over k != i,
 * accumulated from +0.0 in ascending row k.  While n > 2 active nodes are left: over all pairs, lo the node with the smaller
 * id, q = ((double)(n - 2) * d(lo, hi) - r_lo) - r_hi; the pair that is smallest under the strict order (q as a number, id(lo),
 * id(hi)) is joined with the lengths b_lo = 0.5 * d(lo, hi) + (r_lo - r_hi) / (2.0 * (double)(n - 2)) and b_hi = d(lo, hi) -
 * b_lo; for every other active k, duk = 0.5 * ((d(lo, k) + d(hi, k)) - d(lo, hi)), r_k = ((r_k - d(lo, k)) - d(hi, k)) + duk and
 * d(lo, k) = duk; r_lo = 0.5 * ((r_lo + r_hi) - (double)n * d(lo, hi)); the new node takes lo's place and id.  The last two nodes
 * are joined with b_lo = d(lo, hi) and b_hi = 0 (the tree is unrooted; this edge makes the list binary).  Every line is this
 * sequence of binary64 operations in this association, without a fused multiply-add (pansim_amd/csrc/nj_rule.h), so the device,
 * the host form and any restatement that follows it agree bit for bit.  Join k (in the order performed) creates node pop_size +
 * k, the leaves being the rows 0 .. pop_size - 1: left[k] (lo), right[k] (hi) its children, len_left[k], len_right[k] the
 * branches above them, negative ones reported as they are.  (left, right) is a merge list as ps_tree_parsimony takes it.  Limits,
 * else PS_ERR_INVALID: 2 <= pop_size <= 16384 (the matrix holds 2 GB at the cap), fewer than 2^32 core sites; under the
 * accessory metric core_genes >= 1, at most 65535 accessory genes and core_genes + 65535 < 2^32. */
typedef struct {
    uint64_t pop_size, pairs, core_sites, core_genes;      /* pairs: all N (N - 1) / 2 */
    uint64_t metric;
    uint64_t joins;                    /* pop_size - 1 */
    uint64_t negative_branches;        /* lengths below 0.0 among len_left and len_right */
} ps_nj_t;
/* All pairs of two handles of equal pop_size >= 2 on one device (the reference has no such function; population.rs:787-837
 * writes a sample): `core` a core handle that holds all sites, `acc` an accessory handle of at most 65535 genes (required; with
 * the core metric none of its kernels is launched).  left, right, len_left, len_right: pop_size - 1 values each.  Ordered behind
 * all queued work of BOTH handles; changes no state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible; the matrix
 * that cannot be allocated is PS_ERR_OOM with its bytes. */
int ps_neighbour_joining(ps_population *core, ps_population *acc, const ps_tree_params *prm, ps_nj_t *out, uint32_t *left, uint32_t *right,
                         double *len_left, double *len_right);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:787-837); a site shard
 * fails with a message that points to ps_multi_neighbour_joining */
int ps_sim_neighbour_joining(ps_sim *s, const ps_tree_params *prm, ps_nj_t *out, uint32_t *left, uint32_t *right, double *len_left,
                             double *len_right);
/* The same for a sharded run (the reference has no such function; population.rs:787-837): every shard counts its own sites
 * band by band, shard 0 adds them, keeps them as distances and runs the joins against its accessory replica */
int ps_multi_neighbour_joining(ps_multi *m, const ps_tree_params *prm, ps_nj_t *out, uint32_t *left, uint32_t *right, double *len_left,
                               double *len_right);
/* The same rule on the host alone, the plain O(pop_size^3) loop (no device is touched; the reference has no such function;
 * population.rs:787-837): over the COMPLETE list of pairs (r1[k], r2[k]) with their numerators (those of the other metric may be
 * NULL), in any order and orientation.  A missing or duplicate pair (the row sums are undefined on a partial list), an index >=
 * pop_size, r1[k] == r2[k], an intersection above its union and the metric's limits are PS_ERR_INVALID.  It holds pop_size^2
 * doubles and as many bytes on the host (2.3 GB at the cap; PS_ERR_OOM when they cannot be allocated) and takes about pop_size^3 / 6
 * steps: seconds at a few thousand individuals, hours at the cap -- it is the restatement for tests and small samples. */
int ps_nj_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter, const uint32_t *acc_union,
                      uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites, uint64_t core_genes, const ps_tree_params *prm, ps_nj_t *out,
                      uint32_t *left, uint32_t *right, double *len_left, double *len_right);
/* The tree as one line of Newick text in the usual unrooted form, three subtrees at the top (host only;
 * the reference has no such function; population.rs:787-837): the last join is dissolved, its child that is an inner node (the
 * right one if both are) is opened, that node's two children stand at the top level, left then right, and the other child stands
 * beside them with the length of the last edge, len_left + len_right of the last join; pop_size == 2 gives "(0:len,1:0);".
 * Leaves are rows, children left then right, every length written as ps_fmt_f64(len / scale), scale finite and > 0 (core_sites
 * turns the core metric's sites into substitutions per site).  A child that is not an earlier, still free node is
 * PS_ERR_INVALID.  `needed` counts the terminating zero; buf == NULL asks for the size alone, a buffer below it is
 * PS_ERR_INVALID. */
int ps_nj_newick(const uint32_t *left, const uint32_t *right, const double *len_left, const double *len_right, uint64_t pop_size, double scale,
                 char *buf, uint64_t cap, uint64_t *needed);
/* device ms of the last ps_neighbour_joining on this core handle (HIP events; the reference has no such function;
 * population.rs:787-837): the count kernels of the metric, the store kernels and the initial row sums, the joins.
 * PS_ERR_STATE before any call. */
int ps_neighbour_joining_timing(ps_population *core, double *counts_ms, double *store_ms, double *joins_ms);

/* Bootstrap support of the three trees (Felsenstein 1985; docs/BOOTSTRAP_SUPPORT.md): how often the clades of the tree of ALL N
 * individuals come back when the core sites are resampled with replacement.  The reference has no such function: it writes a
 * SAMPLE of pairs as text (population.rs:787-837), from which no tree can be built.  Core metric only.  Replicate b is a
 * multiset of `draws` sites of the L = global core sites (only the multiset matters); its numerator of a pair is the count that
 * ps_pairwise_counts would return on the matrix M[:, sites_b].  Without the caller's lists, draw k of replicate b comes from the
 * Philox4x32-10 block (k >> 1, b, 0, PS_STREAM_BOOTSTRAP = 22) under the key `seed`: the words (x, y) serve draw 2m, (z, w) draw
 * 2m + 1, and site = the high 32 bits of the 96-bit product (x * 2^32 + y) * L, i.e. (x * L + ((y * L) >> 32)) >> 32 in 64-bit
 * arithmetic.  The reference tree is the method's tree of the matrix itself, its merge list (left, right) what the method's own
 * entry returns (PS_BOOT_LINKAGE: ps_merges_from_tree of ps_linkage_tree's edges); the replicates' trees come from the same
 * device code with the same tie rules and row ids.  With S_k the leaves below merge k of the reference tree (node pop_size + k),
 * support[k] = the replicates whose tree has a merge with exactly that leaf set (the two rooted methods), or a merge whose
 * split of the leaves -- its set or the complement -- is that of S_k (PS_BOOT_NJ; a split with fewer than two leaves on one side
 * is in every tree and always found).  Sets only: equal heights are not collapsed.  shared[b] = the reference merges found in
 * replicate b, the last merge (all leaves) always among them. */
#define PS_BOOT_LINKAGE 0
#define PS_BOOT_UPGMA 1
#define PS_BOOT_NJ 2
typedef struct {
    int32_t method;                    /* PS_BOOT_LINKAGE, PS_BOOT_UPGMA or PS_BOOT_NJ */
    uint32_t replicates;               /* 1 .. 65535 */
    uint64_t draws;                    /* sites drawn per replicate, 1 .. 2^31 - 1; 0: the core sites */
    uint64_t seed;                     /* the key of the draw (not read with the caller's lists) */
} ps_bootstrap_params;
typedef struct {
    uint64_t pop_size, pairs, core_sites, core_genes;      /* pairs: all N (N - 1) / 2 */
    uint64_t method, replicates, draws;
    uint64_t merges;                   /* pop_size - 1 */
    uint64_t support_sum;              /* the sum of support[] over all merges */
    uint64_t supported_50, supported_70, supported_95;     /* merges other than the last with support * 100 >= p * replicates */
} ps_bootstrap_t;
/* All pairs of two handles of equal pop_size >= 2 on one device (the reference has no such function; population.rs:787-837
 * writes a sample): `core` a core handle that holds all sites, one-hot (every byte 1, 2, 4 or 8; core_davg_form not 3), `acc`
 * its accessory handle (required as by the trees; none of its kernels is launched).  sites: NULL for the keyed draw, else
 * replicates x draws global site indices, replicate-major (block bootstraps, jackknives); an index >= L is PS_ERR_INVALID with
 * its replicate and position.  left, right, support: pop_size - 1 values each; shared: `replicates` values.  Limits, else
 * PS_ERR_INVALID before anything is queued: those of the method (pop_size <= 16384 for PS_BOOT_UPGMA and PS_BOOT_NJ), 1 <=
 * replicates <= 65535, 1 <= draws < 2^31, 1 <= L < 2^32, one-hot matrices.  Ordered behind all queued work of BOTH handles;
 * changes no state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible. */
int ps_bootstrap_support(ps_population *core, ps_population *acc, const ps_bootstrap_params *prm, const uint32_t *sites, ps_bootstrap_t *out,
                         uint32_t *left, uint32_t *right, uint32_t *support, uint32_t *shared);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:787-837); a site shard
 * fails with a message that points to ps_multi_bootstrap_support */
int ps_sim_bootstrap_support(ps_sim *s, const ps_bootstrap_params *prm, const uint32_t *sites, ps_bootstrap_t *out, uint32_t *left, uint32_t *right,
                             uint32_t *support, uint32_t *shared);
/* The same for a sharded run (the reference has no such function; population.rs:787-837): every shard draws all sites of a
 * replicate, keeps its own and counts them band by band; shard 0 adds the counts and runs the trees */
int ps_multi_bootstrap_support(ps_multi *m, const ps_bootstrap_params *prm, const uint32_t *sites, ps_bootstrap_t *out, uint32_t *left,
                               uint32_t *right, uint32_t *support, uint32_t *shared);
/* The draw rule on the host alone (no device is touched; the reference has no such function; population.rs:787-837): the
 * draws [first, first + count) of replicate `replicate` over core_sites sites (1 .. 2^32 - 1), of `draws` (1 .. 2^31 - 1) */
int ps_bootstrap_sites(uint64_t seed, uint32_t replicate, uint64_t core_sites, uint64_t draws, uint64_t first, uint64_t count,
                       uint32_t *out_sites);
/* The counting on the host alone (no device is touched; the reference has no such function; population.rs:787-837):
 * support and shared as above from the reference tree's merge list and those of `replicates` trees (rep_left, rep_right:
 * replicates x (pop_size - 1), replicate-major), compared as rooted clades (unrooted == 0) or as splits.  Every list is checked
 * as by ps_nj_newick: a child that is not an earlier, still free node is PS_ERR_INVALID.  O(pop_size) per replicate, exact. */
int ps_bootstrap_from_merges(const uint32_t *ref_left, const uint32_t *ref_right, const uint32_t *rep_left, const uint32_t *rep_right,
                             uint64_t replicates, uint64_t pop_size, int unrooted, uint32_t *support, uint32_t *shared);
/* device ms of the last ps_bootstrap_support on this core handle (HIP events; the reference has no such function;
 * population.rs:787-837), summed over the replicates: the site lists (draw, count, scan, expand), the operands (pack, counts,
 * store), the trees.  PS_ERR_STATE before any call. */
int ps_bootstrap_timing(ps_population *core, double *lists_ms, double *operands_ms, double *trees_ms);

/* Nearest neighbours: for every individual its k closest OTHER individuals among ALL N under one distance, and the lineages that
 * follow from them (docs/NEAREST_NEIGHBOURS.md) -- the sparse form of the distance matrix, N k entries, and the graph of
 * PopPUNK's lineage model.  The reference has no such function: it writes a SAMPLE of pairs as text (population.rs:787-837), and
 * a sample holds almost none of an individual's nearest neighbours.  The metrics, their numerators, the undefined distance 0 / 0
 * and the integer comparison are those of the linkage tree above (PS_KNN_CORE = PS_TREE_CORE, PS_KNN_ACC = PS_TREE_ACC).  The
 * neighbours of individual i are ordered by (distance, neighbour's row), rows of the reference's row order: the order is strict,
 * the lists are unique and do not depend on the launch geometry, the bands or the sharding; for the edges at one vertex it is
 * the tree's order (distance, lo, hi).  Limits: 1 <= k <= min(pop_size - 1, PS_KNN_MAX_K); under the accessory metric at most
 * 65535 accessory genes and core_genes + 65535 < 2^32; else PS_ERR_INVALID. */
#define PS_KNN_CORE 0
#define PS_KNN_ACC 1
#define PS_KNN_MAX_K 128u
typedef struct {
    int32_t metric;                    /* PS_KNN_CORE or PS_KNN_ACC */
    uint32_t k;                        /* neighbours per individual */
} ps_knn_params;
typedef struct {
    uint64_t pop_size, pairs, core_sites, core_genes;      /* pairs: all N (N - 1) / 2, or the list's length from ps_neighbours_from_counts */
    uint64_t metric, k;
    uint64_t undefined_neighbours;     /* listed entries with den == 0 */
    uint64_t graph_edges;              /* distinct unordered pairs (i, j) with j in i's list or i in j's */
    uint64_t mutual_edges;             /* unordered pairs where both hold; graph_edges + mutual_edges = the listed entries (N k) */
} ps_knn_t;
typedef struct {
    uint64_t pop_size, rank;
    uint64_t edges;                    /* distinct unordered pairs (i, nbr[i k + q]), q < rank */
    uint64_t lineages, largest_lineage;
    uint64_t within_pairs;             /* pairs of individuals inside one lineage */
} ps_lineage_t;
/* All pairs of two handles of equal pop_size >= 2 on one device (the reference has no such function; population.rs:787-837
 * writes a sample): `core` a core handle that holds all sites, `acc` an accessory handle of at most 65535 genes (required; with
 * the core metric none of its kernels is launched).  nbr, num, den: pop_size * k values each; entry i k + r is the r-th nearest
 * other individual of row i of the reference's row order, its distance num / den (0 / 0: undefined).  Every list is full.  Needs
 * no N x N scratch: O(N k) beside the band of the count kernels.  Ordered behind all queued work of BOTH handles; changes no
 * state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible. */
int ps_nearest_neighbours(ps_population *core, ps_population *acc, const ps_knn_params *prm, ps_knn_t *out, uint32_t *nbr, uint64_t *num,
                          uint64_t *den);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:787-837); a site shard
 * fails with a message that points to ps_multi_nearest_neighbours */
int ps_sim_nearest_neighbours(ps_sim *s, const ps_knn_params *prm, ps_knn_t *out, uint32_t *nbr, uint64_t *num, uint64_t *den);
/* The same for a sharded run (the reference has no such function; population.rs:787-837): every shard counts its own sites
 * band by band, shard 0 adds them and selects against its accessory replica */
int ps_multi_nearest_neighbours(ps_multi *m, const ps_knn_params *prm, ps_knn_t *out, uint32_t *nbr, uint64_t *num, uint64_t *den);
/* The same order on the host alone (no device is touched, as ps_tree_from_counts; the reference has no such function;
 * population.rs:787-837): any list of pairs (r1[k], r2[k]) with their numerators (those of the other metric may be NULL), in
 * the list's own index space; every pair is a candidate of both its ends.  An individual with fewer than k listed partners gets
 * UINT32_MAX, 0, 0 in the unfilled slots (the limits on k are the same).  Of several copies of a pair the nearest (at equal
 * distance the earliest) is listed, once.  The other PS_ERR_INVALID cases are those of
 * ps_tree_from_counts. */
int ps_neighbours_from_counts(const uint32_t *r1, const uint32_t *r2, const uint32_t *core_h, const uint32_t *acc_inter,
                              const uint32_t *acc_union, uint64_t n_pairs, uint64_t pop_size, uint64_t core_sites, uint64_t core_genes,
                              const ps_knn_params *prm, ps_knn_t *out, uint32_t *nbr, uint64_t *num, uint64_t *den);
/* Lineages at rank 1 <= rank <= k (host only; the reference has no such function; population.rs:787-837): the connected
 * components of the graph with the edges {i, nbr[i k + q]}, q < rank.  labels[i] = the smallest row of i's component, as in
 * ps_strain_clusters.  UINT32_MAX entries are skipped; any other index >= pop_size, or a rank outside 1 .. k, is
 * PS_ERR_INVALID. */
int ps_lineages_from_neighbours(const uint32_t *nbr, uint64_t pop_size, uint32_t k, uint32_t rank, ps_lineage_t *out, uint32_t *labels);
/* device ms of the last ps_nearest_neighbours on this core handle (HIP events; the reference has no such function;
 * population.rs:787-837): the count kernels of the metric, the select kernels.  PS_ERR_STATE before any call. */
int ps_nearest_neighbours_timing(ps_population *core, double *counts_ms, double *select_ms);

/* True genealogy of a run (docs/GENEALOGY.md): the parent draws of the generations loop recorded on the device, and from them
 * the relatedness that actually happened -- what the read-outs above infer from distances.  The reference has no such function:
 * its parent draws (population.rs:443) are dropped after every generation.
 * ps_sim_record_ancestry keeps the draws of the last `capacity` generations in a device ring of capacity x pop_size u32 (one
 * stream-ordered copy per generation; the matrices of the run do not change by a bit).  capacity 0 switches the recording off
 * and frees the ring; any call starts an empty record.  The record also starts again (depth 0) at a generation that follows a
 * direct ps_load_matrix / ps_step / ps_next_generation on a handle of the run, and at a ps_sim_run whose first_generation is not
 * the one after the last.  It is not written to state files: ps_sim_load returns a run that records nothing.
 * capacity x pop_size x 4 must stay below 2^64 (PS_ERR_INVALID); an allocation that fails is PS_ERR_OOM. */
#define PS_GEN_BEYOND 0xffffffffu
typedef struct {
    uint64_t pop_size, generation;     /* generation: the generations done (ps_sim_generations_done) */
    uint64_t capacity, depth;          /* depth = min(generations recorded since the record began, capacity) */
    uint64_t roots;                    /* 1 + the entries of coal that are PS_GEN_BEYOND */
    uint64_t tmrca;                    /* max of coal when roots == 1, else 0 */
} ps_genealogy_t;
typedef struct {
    uint64_t clusters, largest, within_pairs;      /* within_pairs: sum over the clusters of size (size - 1) / 2 */
} ps_gen_clusters_t;
int ps_sim_record_ancestry(ps_sim *s, uint32_t capacity);
/* The same for a sharded run (the reference has no such function; population.rs:443): every shard draws the same parents,
 * shard 0 records alone */
int ps_multi_record_ancestry(ps_multi *m, uint32_t capacity);
/* The comb of the present population (the reference has no such function; population.rs:443): order[r], r < pop_size, is the
 * row of the reference's row order (row k = the child of draw k) stored at internal row r; coal[r], r < pop_size - 1, is the
 * smallest t in 1 .. depth at which the ancestors t generations back of internal rows r and r + 1 are one individual, or
 * PS_GEN_BEYOND.  Children are stored in ascending parent order, so the time of ANY two internal rows i < j is
 * max(coal[i .. j - 1]).  Behind all queued work of the run; changes no state.  PS_ERR_NO_DEVICE before anything else when no
 * GPU is visible; PS_ERR_STATE while nothing is recorded (the message names ps_sim_record_ancestry). */
int ps_sim_genealogy(ps_sim *s, ps_genealogy_t *out, uint32_t *order, uint32_t *coal);
int ps_multi_genealogy(ps_multi *m, ps_genealogy_t *out, uint32_t *order, uint32_t *coal);
/* Host-only read-outs of a comb (no device is touched; the reference has no such function; population.rs:443).  order must be
 * a permutation of 0 .. pop_size - 1, rows are rows of the reference's row order.
 * _pair: the time to the most recent common ancestor of rows i and j (0 for i == j; PS_GEN_BEYOND dominates); _pairs: the
 * same for a list. */
int ps_genealogy_pair(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, uint32_t i, uint32_t j, uint32_t *t);
int ps_genealogy_pairs(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, const uint32_t *r1, const uint32_t *r2,
                       uint64_t n_pairs, uint32_t *t);
/* The true clusters at look-back t <= depth (host only; the reference has no such function; population.rs:443): labels[i] =
 * the smallest row among those that share row i's ancestor t generations back, as ps_strain_clusters labels.  t above `depth`
 * (the depth of the comb's ps_genealogy_t) is PS_ERR_INVALID. */
int ps_genealogy_clusters(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, uint32_t depth, uint32_t t, uint32_t *labels,
                          ps_gen_clusters_t *out);
/* The trees of the comb in Newick form (host only; the reference has no such function; population.rs:443): one tree per root,
 * one line each, ending in ";".  Leaves are rows; a segment of the comb splits at EVERY position of its largest time (equal
 * times: a multifurcation), children in comb order as (child:len,...) with whole-number lengths.  *needed = the bytes of the text
 * with its terminating zero; buf == NULL asks for the size alone, a buffer below it is PS_ERR_INVALID. */
int ps_genealogy_newick(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, char *buf, uint64_t cap, uint64_t *needed);

/* Clock histogram: ALL N (N - 1) / 2 pairs binned by (divergence time, distance) -- whether distance tracks time under the
 * run's recombination (docs/GENEALOGY.md).  The reference has no such function (population.rs:443, :787-837).  metric and its
 * numerators as ps_nearest_neighbours; the distance axis by the integer rules of ps_distance_histogram with dist_bins bins
 * (core: span core_span, 0 = automatic; accessory: a pair with b == 0 is in no bin and counted in undefined_pairs).  Time axis
 * with St = time_span (0 = depth): a pair that coalesced t generations back is in row min(time_bins - 1, floor((t - 1)
 * time_bins / St)), a pair beyond the record in the extra row time_bins.  joint[row * dist_bins + bin]: (time_bins + 1) x
 * dist_bins values; per_time[3 row + 0, 1, 2]: the binned pairs of the row, their sum of num and of den (core: num = d = h / 2,
 * den = core sites; accessory: num = a, den = b).  Limits: time_bins, dist_bins >= 1, time_bins <= 1024, (time_bins + 1) x
 * dist_bins <= 16384, time_span < 2^32, the accessory limits of ps_nearest_neighbours; else PS_ERR_INVALID.  Results do not
 * depend on the launch geometry, the bands or the sharding. */
typedef struct {
    int32_t metric;                    /* PS_KNN_CORE or PS_KNN_ACC */
    uint32_t time_bins, dist_bins;
    uint64_t time_span;                /* St >= 1 in generations; 0 = the record's depth */
    uint64_t core_span;                /* as ps_pair_hist_params; not used by the accessory metric */
} ps_clock_params;
typedef struct {
    uint64_t pop_size, pairs, core_sites, core_genes;      /* pop_size is 0 from ps_clock_from_counts */
    uint64_t metric, time_bins, dist_bins;
    uint64_t time_span, core_span;     /* the spans used (core_span 0 under the accessory metric) */
    uint64_t depth;
    uint64_t undefined_pairs, core_clamped;
    uint64_t beyond_pairs;             /* the binned pairs of row time_bins */
    uint64_t binned_pairs;             /* the sum of joint = pairs - undefined_pairs */
    uint64_t num_sum, den_sum;         /* over the binned pairs */
} ps_clock_t;
/* The two matrices of a recording simulation against its own record.  Behind all queued work of the run; changes no state.
 * PS_ERR_NO_DEVICE before anything else when no GPU is visible; PS_ERR_STATE while nothing is recorded (the message names
 * ps_sim_record_ancestry); a site shard fails with a message that points to ps_multi_clock_histogram */
int ps_sim_clock_histogram(ps_sim *s, const ps_clock_params *prm, ps_clock_t *out, uint64_t *joint, uint64_t *per_time);
/* The same for a sharded run (the reference has no such function; population.rs:443, :787-837): every shard counts its own
 * sites band by band, shard 0 adds them and bins against its own record and accessory replica */
int ps_multi_clock_histogram(ps_multi *m, const ps_clock_params *prm, ps_clock_t *out, uint64_t *joint, uint64_t *per_time);
/* The same rules on the host alone (no device is touched, as ps_histogram_from_counts; the reference has no such function;
 * population.rs:443, :787-837): any list of pairs with their divergence times (1 .. depth or PS_GEN_BEYOND, e.g. from
 * ps_genealogy_pairs) and numerators (those of the other metric may be NULL).  n_pairs >= 1, 1 <= depth < 2^32 - 1. */
int ps_clock_from_counts(const uint32_t *tmrca, const uint32_t *core_h, const uint32_t *acc_inter, const uint32_t *acc_union,
                         uint64_t n_pairs, uint64_t depth, uint64_t core_sites, uint64_t core_genes, const ps_clock_params *prm,
                         ps_clock_t *out, uint64_t *joint, uint64_t *per_time);
/* device ms of the last clock histogram on this core handle (HIP events; the reference has no such function;
 * population.rs:787-837): the count kernels of the metric; the comb, the table and the binning.  PS_ERR_STATE before any call. */
int ps_clock_histogram_timing(ps_population *core, double *counts_ms, double *binning_ms);

/* Linkage disequilibrium between LOCI (docs/LINKAGE_DISEQUILIBRIUM.md) -- the other axis of the two matrices: r^2 and the
 * four-gamete test over all pairs of the selected columns, binned by r^2 and by the distance between the columns.  The reference
 * has no such function (the signature of its recombination is read off population.rs:544-751, the counts are those of :840-863).
 * A locus is a column: a core site (indicator: the cell equals the site's major base -- the most frequent of the bytes 1, 2, 4, 8,
 * ties to the lowest byte; any other cell is 0) or an accessory gene (indicator: presence).  c = the ones of a locus over the N =
 * pop_size individuals; c == 0 or c == N is monomorphic.  Selection: an explicit strictly ascending list (monomorphic entries
 * kept), or automatically the C columns with min(c, N - c) >= min_minor in column order, all of them if C <= max_loci, else
 * entry j = the candidate of rank floor(j C / max_loci).  Per pair a < b of the list, columns s_a < s_b, n11 = the individuals
 * with both indicators set: a pair with a monomorphic locus is counted in undefined_pairs and nowhere else; otherwise
 * D = N n11 - c_a c_b, den = c_a (N - c_a) c_b (N - c_b), q = floor(2^16 D^2 / den) in [0, 65536], r^2 bin = min(r2_bins - 1,
 * (q r2_bins) >> 16), lag bin = min(lag_bins - 1, floor(log2(s_b - s_a))), hist[lag * r2_bins + r2] += 1, lag_sum_q[lag] += q.
 * Every result but mean_r2 is an integer: nothing depends on the launch geometry, the bands, the sharding or the order of the
 * individuals.  Limits: pop_size <= 65536, max_loci (or n_loci) <= 65536, min_minor >= 1, r2_bins >= 1, 1 <= lag_bins <= 32,
 * r2_bins x lag_bins <= 16384; else PS_ERR_INVALID.  Fewer than two loci is not an error: no pairs. */
#define PS_LD_CORE 0
#define PS_LD_ACC 1
#define PS_LD_MAX_LOCI 65536u
typedef struct {
    uint32_t r2_bins, lag_bins;
    uint32_t min_minor;                /* automatic selection: candidates have min(c, N - c) >= min_minor */
    uint32_t max_loci;                 /* automatic selection: at most this many loci */
} ps_ld_params;
typedef struct {
    uint64_t pop_size, columns;
    uint64_t candidates;               /* C of the automatic selection; the polymorphic entries of an explicit list */
    uint64_t loci;                     /* M */
    uint64_t pairs, defined_pairs, undefined_pairs;        /* pairs = M (M - 1) / 2 = defined + undefined */
    uint64_t four_gamete_pairs;        /* all four combinations present */
    uint64_t complete_pairs;           /* q == 65536 */
    uint64_t positive_pairs, negative_pairs;               /* D > 0, D < 0 */
    uint64_t sum_q;
    double mean_r2;                    /* (double)sum_q / 65536.0 / (double)defined_pairs; 0.0 without defined pairs */
    uint64_t r2_bins, lag_bins, min_minor, max_loci;
} ps_ld_t;
/* One handle, core or accessory by its kind (the reference has no such function; population.rs:544-751, :840-863).  loci ==
 * NULL: automatic selection; else n_loci column indices.  locus_index, locus_count (either may be NULL): max_loci entries
 * (n_loci when explicit), the first out->loci written.  hist: lag_bins x r2_bins values; lag_sum_q: lag_bins.  Ordered behind
 * all queued work of the handle (a two-generation sweep launch included); changes no state.  PS_ERR_NO_DEVICE before anything
 * else when no GPU is visible; a site shard fails with a message that points to ps_multi_locus_ld. */
int ps_locus_ld(ps_population *p, const ps_ld_params *prm, const uint32_t *loci, uint32_t n_loci, ps_ld_t *out, uint32_t *locus_index,
                uint32_t *locus_count, uint64_t *hist, uint64_t *lag_sum_q);
/* The same for one matrix of a simulation, metric PS_LD_CORE or PS_LD_ACC (the reference has no such function;
 * population.rs:544-751, :840-863) */
int ps_sim_locus_ld(ps_sim *s, int32_t metric, const ps_ld_params *prm, const uint32_t *loci, uint32_t n_loci, ps_ld_t *out,
                    uint32_t *locus_index, uint32_t *locus_count, uint64_t *hist, uint64_t *lag_sum_q);
/* The same for a sharded run (the reference has no such function; population.rs:544-751, :840-863).  Core: every shard counts
 * and packs its own selected sites (candidate ranks offset by the shards before it), the bit rows travel to shard 0, which
 * contracts and bins; column indices are global.  Accessory: shard 0's replica. */
int ps_multi_locus_ld(ps_multi *m, int32_t metric, const ps_ld_params *prm, const uint32_t *loci, uint32_t n_loci, ps_ld_t *out,
                      uint32_t *locus_index, uint32_t *locus_count, uint64_t *hist, uint64_t *lag_sum_q);
/* The automatic selection on the host alone (no device is touched, as ps_histogram_from_counts; the reference has no such
 * function; population.rs:840-863): ones[col] = c of every column; index has room for max_loci entries. */
int ps_ld_select_loci(const uint32_t *ones, uint64_t columns, uint64_t pop_size, uint32_t min_minor, uint32_t max_loci, uint32_t *index,
                      uint64_t *n_loci, uint64_t *candidates);
/* The per-pair rules on the host alone (no device is touched; the reference has no such function; population.rs:544-751,
 * :840-863): n_loci loci with strictly ascending locus_index and their counts, n11 of the n_loci (n_loci - 1) / 2 pairs (a, b),
 * a < b, row-major (NULL when n_loci < 2).  A count above pop_size, or an n11 that the two counts do not allow, is
 * PS_ERR_INVALID.  out->columns and out->candidates are 0. */
int ps_ld_from_counts(const uint32_t *locus_index, const uint32_t *locus_count, const uint32_t *n11, uint64_t n_loci, uint64_t pop_size,
                      const ps_ld_params *prm, ps_ld_t *out, uint64_t *hist, uint64_t *lag_sum_q);
/* device ms of the last ps_locus_ld on this handle (shard 0's core handle after ps_multi_locus_ld; HIP events; the reference has
 * no such function; population.rs:544-751): counts and selection, packing, the contraction, the pair statistics.  PS_ERR_STATE
 * before any call. */
int ps_locus_ld_timing(ps_population *p, double *select_ms, double *pack_ms, double *counts_ms, double *stats_ms);

/* Gene-site association (docs/GENE_SITE_ASSOCIATION.md) -- the cross block ps_locus_ld leaves out: r^2 over all pairs (accessory
 * gene g, core site s) of two selected lists.  The reference has no such function (the signature of its recombination is read off
 * population.rs:544-751, the counts are those of :840-863).  Indicators, c and "monomorphic" are those of ps_locus_ld.  The
 * selection rule of ps_locus_ld runs on each side on its own: sites with site_min_minor / max_sites or the strictly ascending
 * list `sites`, genes with gene_min_minor / max_genes or `genes`; Ms sites, Mg genes, either may be 0 (no pairs).  Per pair, n11 =
 * the individuals with both indicators set: a pair with a monomorphic locus is counted in undefined_pairs and nowhere else;
 * otherwise q, the sign of D, the four-gamete flag and `complete` are those of ps_locus_ld, r^2 bin = min(r2_bins - 1,
 * (q r2_bins) >> 16), frequency bin of the gene = min(freq_bins - 1, floor(2 m freq_bins / N)) with m = min(c_g, N - c_g),
 * hist[freq * r2_bins + r2] += 1, freq_sum_q[freq] += q, and the pair is strong when q >= strong_q.  Best tag of a gene: over its
 * defined pairs the site with the largest q, ties to the lowest column (a gene whose every q is 0 reports its lowest defined
 * site; one without a defined pair PS_GS_NONE, q 0, sign 0); of a site: the gene, likewise.  Every result but mean_r2 is an
 * integer sum or a maximum under a strict order: nothing depends on the launch geometry, the bands, the sharding or the order of
 * the individuals.  Limits: pop_size <= 65536, max_sites (or n_sites) + max_genes (or n_genes) <= 65536, each automatic cap and
 * both minors >= 1, r2_bins >= 1, freq_bins >= 1, r2_bins x freq_bins <= 16384, 1 <= strong_q <= 65536; else PS_ERR_INVALID. */
#define PS_GS_NONE 0xFFFFFFFFu
typedef struct {
    uint32_t r2_bins, freq_bins;
    uint32_t site_min_minor, gene_min_minor;   /* automatic selection of a side: candidates have min(c, N - c) >= this */
    uint32_t max_sites, max_genes;             /* automatic selection of a side: at most this many */
    uint32_t strong_q;                         /* a pair with q >= strong_q is strong (32768: r^2 >= 0.5) */
} ps_gs_params;
typedef struct {
    uint64_t pop_size, site_columns, gene_columns;
    uint64_t site_candidates, gene_candidates;             /* C of an automatic side; the polymorphic entries of an explicit list */
    uint64_t sites, genes;                                 /* Ms, Mg */
    uint64_t pairs, defined_pairs, undefined_pairs;        /* pairs = Ms Mg = defined + undefined */
    uint64_t four_gamete_pairs, complete_pairs, positive_pairs, negative_pairs;
    uint64_t strong_pairs;                                 /* q >= strong_q */
    uint64_t genes_tagged, sites_tagging;                  /* genes / sites whose best q >= strong_q */
    uint64_t sum_q;
    double mean_r2;                                        /* (double)sum_q / 65536.0 / (double)defined_pairs; 0.0 without defined pairs */
    uint64_t r2_bins, freq_bins, site_min_minor, gene_min_minor, max_sites, max_genes, strong_q;
} ps_gs_t;
/* The per-locus arrays of one side, each NULL or with room for the side's cap (its n_ when explicit); the first Ms (Mg) entries
 * are written: the column, its ones, the best partner's column (or PS_GS_NONE), its q, the locus' strong pairs, the sign of D
 * with the best partner (-1 / 0 / +1). */
typedef struct {
    uint32_t *index, *count, *best, *best_q, *strong;
    int32_t *best_sign;
} ps_gs_side;
/* The core handle and the accessory handle of the same individuals on one device (the reference has no such function;
 * population.rs:544-751, :840-863).  sites == NULL / genes == NULL: that side is selected automatically.  site_out, gene_out: NULL
 * or the arrays wanted.  hist: freq_bins x r2_bins values; freq_sum_q: freq_bins.  Genes are packed on the accessory handle's
 * stream and sites on the core handle's, each behind its handle's queued work (a two-generation sweep launch included); changes
 * no state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible; a site shard fails with a message that points to
 * ps_multi_gene_site_ld. */
int ps_gene_site_ld(ps_population *core, ps_population *acc, const ps_gs_params *prm, const uint32_t *sites, uint32_t n_sites,
                    const uint32_t *genes, uint32_t n_genes, ps_gs_t *out, const ps_gs_side *site_out, const ps_gs_side *gene_out,
                    uint64_t *hist, uint64_t *freq_sum_q);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:544-751, :840-863) */
int ps_sim_gene_site_ld(ps_sim *s, const ps_gs_params *prm, const uint32_t *sites, uint32_t n_sites, const uint32_t *genes,
                        uint32_t n_genes, ps_gs_t *out, const ps_gs_side *site_out, const ps_gs_side *gene_out, uint64_t *hist,
                        uint64_t *freq_sum_q);
/* The same for a sharded run (the reference has no such function; population.rs:544-751, :840-863): every shard counts, selects
 * and packs its own sites, the bit rows travel to shard 0, whose accessory replica provides the genes and which contracts and
 * bins; column indices are global. */
int ps_multi_gene_site_ld(ps_multi *m, const ps_gs_params *prm, const uint32_t *sites, uint32_t n_sites, const uint32_t *genes,
                          uint32_t n_genes, ps_gs_t *out, const ps_gs_side *site_out, const ps_gs_side *gene_out, uint64_t *hist,
                          uint64_t *freq_sum_q);
/* The per-pair rules and the best tags on the host alone (no device is touched; the reference has no such function;
 * population.rs:544-751, :840-863): the two lists with strictly ascending columns and their counts, n11 of the n_genes x n_sites
 * pairs, row-major (NULL without pairs).  The index and count members of the two sides are not written.  A count above pop_size,
 * or an n11 that the two counts do not allow, is PS_ERR_INVALID.  The columns and the candidates of `out` are 0. */
int ps_gene_site_from_counts(const uint32_t *site_index, const uint32_t *site_count, uint64_t n_sites, const uint32_t *gene_index,
                             const uint32_t *gene_count, uint64_t n_genes, const uint32_t *n11, uint64_t pop_size,
                             const ps_gs_params *prm, ps_gs_t *out, const ps_gs_side *site_out, const ps_gs_side *gene_out,
                             uint64_t *hist, uint64_t *freq_sum_q);
/* device ms of the last ps_gene_site_ld on this core handle (shard 0's after ps_multi_gene_site_ld; HIP events; the reference has
 * no such function; population.rs:544-751): counts and selection of both sides, packing, the contraction, the pair statistics.
 * PS_ERR_STATE before any call. */
int ps_gene_site_ld_timing(ps_population *core, double *select_ms, double *pack_ms, double *counts_ms, double *stats_ms);

/* Core allele profiles, cgMLST (docs/ALLELE_PROFILES.md).  The reference has no such function (the sequences are the rows of the
 * core matrix, population.rs:164-170).  The L core sites are cut into n_loci loci: without `bounds` locus g is the sites
 * [floor(g L / n_loci), floor((g + 1) L / n_loci)) (n_loci <= L); with `bounds` (n_loci + 1 values, strictly ascending, the last
 * <= L) locus g is [bounds[g], bounds[g + 1]) and the sites outside belong to no locus.  Two individuals carry the same allele of
 * a locus iff their bytes agree at every site of it (bytes outside 1 / 2 / 4 / 8 are just other values); the alleles of a locus
 * are numbered 0 .. A_g - 1 by first appearance in output row order (the reference's row order, as the labels of
 * ps_strain_clusters).  locus_alleles[g] = A_g, locus_same_pairs[g] = the pairs of individuals with the same allele.  Per pair
 * i < j, d = the loci at which the numbers differ: hist[floor(d dist_bins / (n_loci + 1))] += 1, sum_d, min_d, max_d,
 * identical_pairs (d = 0), edges (d <= complex_max).  st[k]: the smallest output row with the profile of k (the sequence type);
 * complex_of[k]: the smallest output row of k's connected component of the graph d <= complex_max (single linkage).  The device
 * compares 128-bit keyed fingerprints of the loci (key_seed; key_bits < 64 shortens the keys, for tests) and then verifies every
 * class byte for byte: a fingerprint collision ends the call with PS_ERR_STATE and changes no result.  Every result but
 * mean_distance is an exact integer and depends on the sequences and the row order only.  Limits, else PS_ERR_INVALID: 2 <=
 * pop_size <= 65536, 1 <= n_loci <= 65535, n_loci x pop_size <= 2^30, 1 <= dist_bins <= 16384, complex_max <= n_loci, 1 <=
 * key_bits <= 64. */
typedef struct {
    uint32_t n_loci, dist_bins, complex_max, key_bits;
    uint64_t key_seed;
} ps_mlst_params;
typedef struct {
    uint64_t pop_size, pairs, core_sites;
    uint64_t loci, sites_covered;                              /* sites_covered: the sites inside a locus */
    uint64_t alleles_total, max_alleles, monomorphic_loci;     /* the sum and the maximum of A_g; the loci with A_g = 1 */
    uint64_t sequence_types, singleton_sts, largest_st;
    uint64_t identical_pairs;                                  /* = the sum over sequence types of size (size - 1) / 2 */
    uint64_t complexes, largest_complex;
    uint64_t edges;
    uint64_t sum_d, min_d, max_d;                              /* sum_d = the sum over loci of (pairs - locus_same_pairs) */
    double mean_distance;                                      /* (double)sum_d / (double)pairs / (double)loci */
    uint64_t dist_bins, complex_max;
    uint64_t rounds;                                           /* label rounds taken on the device (0 from the host form) */
} ps_mlst_t;
/* A core handle that holds all sites (the reference has no such function; population.rs:164-170).  bounds: NULL or n_loci + 1
 * values.  locus_alleles: n_loci u32; locus_same_pairs: n_loci u64; st, complex_of: pop_size u32; hist: dist_bins u64; profiles:
 * NULL or pop_size x n_loci u16, individual-major.  Runs on the handle's stream behind its queued work (a two-generation sweep
 * launch included); changes no state; the tuning key "mlst_band" forces the loci per band of the fingerprint table.
 * PS_ERR_NO_DEVICE before anything else when no GPU is visible; a site shard fails with a message that points to
 * ps_multi_allele_profiles. */
int ps_allele_profiles(ps_population *core, const ps_mlst_params *prm, const uint64_t *bounds, ps_mlst_t *out, uint32_t *locus_alleles,
                       uint64_t *locus_same_pairs, uint32_t *st, uint32_t *complex_of, uint64_t *hist, uint16_t *profiles);
/* The same for the core matrix of a simulation (the reference has no such function; population.rs:164-170); the run is not
 * synchronised. */
int ps_sim_allele_profiles(ps_sim *s, const ps_mlst_params *prm, const uint64_t *bounds, ps_mlst_t *out, uint32_t *locus_alleles,
                           uint64_t *locus_same_pairs, uint32_t *st, uint32_t *complex_of, uint64_t *hist, uint16_t *profiles);
/* The same for a sharded run (the reference has no such function; population.rs:164-170): every shard fingerprints the sites it
 * holds (a locus may straddle shards), the tables add on shard 0, which numbers the alleles and runs the pairs; every shard
 * verifies its own sites. */
int ps_multi_allele_profiles(ps_multi *m, const ps_mlst_params *prm, const uint64_t *bounds, ps_mlst_t *out, uint32_t *locus_alleles,
                             uint64_t *locus_same_pairs, uint32_t *st, uint32_t *complex_of, uint64_t *hist, uint16_t *profiles);
/* Everything above from any table of allele ids on the host alone (no device is touched; the reference has no such function;
 * population.rs:164-170): alleles = pop_size x n_loci u32, individual-major, in output row order; the ids of a locus need not be
 * dense and are renumbered by first appearance.  core_sites and sites_covered of `out` are 0; key_bits and key_seed are not
 * used (key_bits is still checked). */
int ps_profiles_from_alleles(const uint32_t *alleles, uint64_t pop_size, const ps_mlst_params *prm, ps_mlst_t *out, uint32_t *locus_alleles,
                             uint64_t *locus_same_pairs, uint32_t *st, uint32_t *complex_of, uint64_t *hist, uint16_t *profiles);
/* device ms of the last ps_allele_profiles on this core handle (shard 0's after ps_multi_allele_profiles; HIP events; the
 * reference has no such function; population.rs:164-170): the fingerprints, the allele numbers, the verification, the pairs, the
 * label rounds.  PS_ERR_STATE before any call. */
int ps_allele_profiles_timing(ps_population *core, double *fingerprint_ms, double *canon_ms, double *verify_ms, double *pairs_ms,
                              double *labels_ms);

/* Isolate samples (docs/ISOLATE_SAMPLES.md): some rows of one or more populations as a NEW handle on the device, so that every
 * read-out of this header answers for a sample (a few hundred isolates, a bootstrap replicate, serial samples pooled over time) as
 * it answers for a population.  The reference has no such function (its only sample is the random pairs of main.rs:413-427; the
 * rows are those of population.rs:164-170).  The new handle is a full, independent ps_population on the device of parts[0] with a
 * stream of its own, made as ps_population_create makes one: cfg of parts[0] with pop_size = the sum of n_rows, no rates set,
 * output row order = internal order, row j = the j-th requested row; nibble / one-hot safety = the AND over the parts; the pad
 * bytes of the core rows and the pad bits of the accessory rows are zero.  It is destroyed with ps_population_destroy, in any
 * order relative to its sources.  A source is read on its own stream behind whatever is queued there (a two-generation sweep
 * launch included) and never written: its matrix, edit epoch, cached pair lists and read-out scratch do not change, and a run
 * continues bit for bit.  The call returns with the gathers complete.  PS_ERR_INVALID, naming the field or index, `*out` null: a
 * null argument, n_parts = 0, the sum of n_rows = 0 or beyond what ps_population_create accepts, a row >= its part's pop_size,
 * parts that are not all core or all accessory, that differ in ncols, col_offset, global_cols or core_genes, or that are on
 * different devices.  The core matrix is gathered within every site row by core_gather_rows_kernel, which stages the source row in
 * LDS or, for source rows beyond 64 KiB and for 48 n < pitch, loads the bytes from global memory; the tuning key "gather_form"
 * of the SOURCE handle forces the form (0 = choose, 1 = LDS, 2 = direct). */
/* rows of parts[k] (rows == NULL or rows[k] == NULL: all of them, n_rows[k] = that part's pop_size), in that handle's OUTPUT row
 * order as every read-out numbers rows; rows may repeat (the reference has no such function; population.rs:164-170) */
int ps_population_pool(ps_population *const *parts, const uint32_t *const *rows, const uint64_t *n_rows, uint32_t n_parts,
                       ps_population **out);
/* = the pool of one part (the reference has no such function; population.rs:164-170) */
int ps_population_subset(ps_population *src, const uint32_t *rows, uint64_t n_rows, ps_population **out);
/* the core and the accessory sample of a run from the same rows; either out pointer may be NULL; the run is not synchronised
 * (the reference has no such function; population.rs:164-170) */
int ps_sim_subset(ps_sim *s, const uint32_t *rows, uint64_t n_rows, ps_population **core_out, ps_population **acc_out);
/* the same for a sharded run (the reference has no such function; population.rs:164-170): the core sample is a WHOLE handle
 * (col_offset 0, ncols = global_cols) on shard 0's device -- every shard gathers the sites it holds, whose block lands
 * contiguously at col_offset x pitch, directly on shard 0's device and through a peer copy from another; the accessory sample
 * comes from shard 0's replica */
int ps_multi_subset(ps_multi *m, const uint32_t *rows, uint64_t n_rows, ps_population **core_out, ps_population **acc_out);
/* device ms of the gather(s) that filled `made` (HIP events on the sources' streams, the peer copies of shards included; the
 * reference has no such function; population.rs:164-170).  PS_ERR_STATE on a handle that none of the calls above made. */
int ps_population_subset_timing(ps_population *made, double *gather_ms);
/* Host only, no device: the comb of ps_sim_genealogy (docs/GENEALOGY.md) restricted to `rows` (n_rows >= 1 output rows below n;
 * they may repeat).  The reference has no such function (the parents are the draws of population.rs:443).  The positions are
 * walked in ascending order and those whose row is in `rows` kept; a row asked for several times gives several entries at its
 * position, in the order of their indices in `rows`, with coalescence time 0 between them.  order_out (n_rows u32): the INDEX IN
 * `rows` of every kept entry, which is its row in the handle ps_sim_subset makes from the same rows; coal_out (n_rows - 1 u32):
 * the maximum of coal between two neighbouring kept entries (PS_GEN_BEYOND is the largest value).  So for all a, b:
 * pair(restricted, a, b) == pair(full, rows[a], rows[b]). */
int ps_genealogy_restrict(const uint32_t *order, const uint32_t *coal, uint64_t n, const uint32_t *rows, uint64_t n_rows,
                          uint32_t *order_out, uint32_t *coal_out);

/* Group differentiation (docs/GROUP_DIFFERENTIATION.md): what the labels of strain_clusters, the trees' clusters_at, the
 * lineages and the genealogy's clusters say about the matrices.  The reference has no such function (the counts are the grouped
 * form of population.rs:840-863).  Groups: a distinct label value with at least min_size members is a candidate, candidates are
 * ranked by (size descending, label ascending), the first max_groups (1 .. PS_GROUPS_MAX) are groups 0 .. K - 1; everyone else
 * is unassigned (group_of = UINT32_MAX) and takes part in nothing.  K = 0 is PS_ERR_INVALID.  With n_g the group sizes, N_a
 * their sum and c_{s,g,c} the cells of site s in group g of class c (A, C, G, T, other: the five classes of
 * docs/CORE_DIVERSITY.md):
 *   counts[(s K + g) 4 + a]  cells of site s in group g whose byte is 1 << a
 *   between[g K + h]         sum_s (n_g n_h - sum_c c_{s,g,c} c_{s,h,c}), the (pair, site) differences; g == h: sum_s (n_g^2 -
 *                            sum_c c^2) / 2; symmetric
 *   fixed[g K + h]           sites where g and h share no class; g == h: sites where g is monomorphic
 *   site_within[s]           sum_g (n_g^2 - sum_c c_{s,g,c}^2) / 2
 *   site_total[s]            (N_a^2 - sum_c (sum_g c_{s,g,c})^2) / 2
 *   gene_counts[y K + g]     members of g that carry accessory gene y
 *   acc_between[g K + h]     sum_y (c_g (n_h - c_h) + (n_g - c_g) c_h), presence / absence differences over pairs; g == h: sum_y
 *                            c_g (n_g - c_g)
 *   gene_fixed[g K + h]      genes present in every member of g and absent from every member of h
 *   gene_private[g]          genes with c_g > 0 and c_h = 0 for every other group h
 * Every integer is exact over ALL pairs and independent of the launch geometry, the sharding and the order of the individuals;
 * the doubles are formed once from the integers. */
#define PS_GROUPS_MAX 16
typedef struct {
    uint32_t max_groups;               /* 1 .. PS_GROUPS_MAX */
    uint32_t min_size;                 /* >= 1 */
} ps_diff_params;
typedef struct {
    uint64_t pop_size, sites, genes;   /* N; core sites this result covers; accessory genes (0 without the accessory handle) */
    uint64_t groups, assigned, unassigned;                 /* K, N_a, N - N_a */
    uint64_t other_cells;              /* cells of the assigned that are not 1/2/4/8 */
    uint64_t within_pairs, between_pairs;                  /* sum_g n_g (n_g - 1) / 2; sum_{g<h} n_g n_h */
    uint64_t within_differences, between_differences;      /* sum_g between[g][g]; sum_{g<h} between[g][h] */
    double pi_within, pi_between;      /* differences / pairs / sites, 0.0 when a denominator is 0 */
    double fst;                        /* Hudson: 1 - pi_within / pi_between, 0.0 when pi_between is 0 */
} ps_diff_t;
/* The group rules on the host alone (no device is touched; the reference has no such function; population.rs:840-863 grouped):
 * labels and group_of hold pop_size values, group_label and group_size max_groups (the first *groups written). */
int ps_groups_from_labels(const uint32_t *labels, uint64_t pop_size, uint32_t max_groups, uint32_t min_size, uint32_t *group_of,
                          uint32_t *group_label, uint32_t *group_size, uint32_t *groups);
/* One core handle and, or NULL, the accessory handle of the same individuals on the same device (the reference has no such
 * function; population.rs:840-863 grouped).  labels: pop_size values in the reference's row order.  group_of: pop_size;
 * group_label, group_size: max_groups; between, fixed, acc_between, gene_fixed: max_groups^2 (K x K values are written,
 * densely); gene_private: max_groups; site_within, site_total: ncols; counts: ncols x max_groups x 4 (ncols x K x 4 written);
 * gene_counts: genes x max_groups.  site_within .. gene_private may each be NULL, and what is not asked for launches no work of
 * its own; the gene outputs need `acc`.  pop_size <= 65536.  A site-shard core handle answers for its own sites, without an
 * accessory handle (with one: ps_multi_group_differentiation).  Ordered behind all queued work of both handles; changes no
 * state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible. */
int ps_group_differentiation(ps_population *core, ps_population *acc, const uint32_t *labels, const ps_diff_params *prm, ps_diff_t *out,
                             uint32_t *group_of, uint32_t *group_label, uint32_t *group_size, uint64_t *between, uint64_t *fixed,
                             uint32_t *site_within, uint32_t *site_total, uint32_t *counts, uint32_t *gene_counts, uint64_t *acc_between,
                             uint64_t *gene_fixed, uint64_t *gene_private);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:840-863 grouped) */
int ps_sim_group_differentiation(ps_sim *s, const uint32_t *labels, const ps_diff_params *prm, ps_diff_t *out, uint32_t *group_of,
                                 uint32_t *group_label, uint32_t *group_size, uint64_t *between, uint64_t *fixed, uint32_t *site_within,
                                 uint32_t *site_total, uint32_t *counts, uint32_t *gene_counts, uint64_t *acc_between,
                                 uint64_t *gene_fixed, uint64_t *gene_private);
/* The same for a sharded run (the reference has no such function; population.rs:840-863 grouped): every shard answers for its
 * own sites, the u64 matrices and the summary integers add, the per-site arrays and the counts concatenate in site order
 * (core_size sites), the doubles are formed once; the genes from shard 0's accessory replica. */
int ps_multi_group_differentiation(ps_multi *m, const uint32_t *labels, const ps_diff_params *prm, ps_diff_t *out, uint32_t *group_of,
                                   uint32_t *group_label, uint32_t *group_size, uint64_t *between, uint64_t *fixed, uint32_t *site_within,
                                   uint32_t *site_total, uint32_t *counts, uint32_t *gene_counts, uint64_t *acc_between,
                                   uint64_t *gene_fixed, uint64_t *gene_private);
/* The core results from a counts table, on the host alone (no device is touched, as ps_diversity_from_counts; the reference has
 * no such function; population.rs:840-863 grouped).  counts: sites x groups x 4; group_size: groups values that add up to at
 * most 65536; between, fixed: groups^2; site_within, site_total: sites, or NULL.  out->pop_size = out->assigned = the sum of the
 * sizes, out->genes = 0.  Counts of a (site, group) that add up to more than the group's size are PS_ERR_INVALID. */
int ps_differentiation_from_counts(const uint32_t *counts, uint64_t sites, uint32_t groups, const uint32_t *group_size, ps_diff_t *out,
                                   uint64_t *between, uint64_t *fixed, uint32_t *site_within, uint32_t *site_total);
/* device ms of the last ps_group_differentiation on this core handle (each shard's own after the ps_multi form; HIP events; the
 * reference has no such function; population.rs:840-863 grouped): the membership tables, the core pass, the gene pass (0.0
 * without one).  PS_ERR_STATE before any call. */
int ps_group_differentiation_timing(ps_population *core, double *members_ms, double *core_ms, double *genes_ms);

/* Parsimony of the two matrices on a tree (docs/TREE_PARSIMONY.md): Fitch parsimony of every core site and accessory gene on a
 * given binary tree -- how often each column changed, which sites changed more often than their alleles require (homoplasy),
 * and how many sites changed and genes were gained or lost on every branch.  The reference has no such function (its trees are
 * implicit in the parent draws of population.rs:443; the columns are those of population.rs:840-863).
 * Tree: merges `left[k]`, `right[k]`, k < merges, of node ids in scipy's numbering as ps_upgma_tree returns them: nodes 0 ..
 * pop_size - 1 are the leaves (rows of the reference's row order), merge k creates node pop_size + k.  2 <= pop_size <=
 * PS_PARS_MAX_POP, 1 <= merges <= pop_size - 1, every child id < pop_size + k, left[k] != right[k], no node a child twice; else
 * PS_ERR_INVALID, found on the host before any device work.  merges < pop_size - 1 is a forest; a node that is nobody's child is
 * a root, a leaf that is one is uncovered.
 * States: the class bit of a core cell is its byte if that is 1, 2, 4 or 8, else 16 (`other`, a fifth state); of a gene 1
 * (absent) or 2 (present).  Up pass: S(leaf) = its class bit, S(node) = S(l) & S(r) if not empty, else S(l) | S(r);
 * changes[s] = the merges with an empty intersection at column s, the minimum number of changes of the column on the tree.
 * Down pass (only when a branch, gain or loss output is asked for): X(root) = the lowest bit of S(root); X(c) = X(v) if
 * X(v) & S(c) is not empty, else the lowest bit of S(c); the branch above c changes at s iff X(c) != X(v), for a gene 1 -> 2 is
 * a gain and 2 -> 1 a loss.  Over all branches the changing branches of a column are changes[s].
 *   site_changes[s]                    changes of core site s
 *   site_hist[PS_PARS_BINS]            sites by their changes, the last bin >= PS_PARS_BINS - 1
 *   branch_changes[node]               core sites that change on the branch above the node (pop_size + merges values; roots 0)
 *   gene_changes / _gains / _losses[y] per accessory gene; gains + losses = changes
 *   branch_gains / branch_losses[node] genes gained / lost on the branch above the node
 * Every integer is exact and independent of the launch geometry, the sharding and the order of the individuals; ci is formed
 * once from the integers. */
#define PS_PARS_BINS 64
#define PS_PARS_MAX_POP 16384u
typedef struct {
    uint64_t pop_size, sites, genes;   /* N; core sites this result covers; accessory genes (0 without a gene output) */
    uint64_t merges, trees;            /* M; internal roots */
    uint64_t covered_leaves;           /* leaves that are somebody's child */
    uint64_t spanning;                 /* 1 iff merges == pop_size - 1 */
    uint64_t total_changes, changed_sites, max_changes;    /* sum, number of non-zero entries and maximum of site_changes */
    uint64_t gene_total_changes, gene_total_gains, gene_total_losses;  /* gains and losses 0 when no down pass ran on the genes */
    /* only when spanning, else 0: min_changes = sum_s (classes_s - 1) with classes_s the distinct class bits among all leaves;
     * excess_changes = total_changes - min_changes; homoplasic_sites = the sites with changes[s] > classes_s - 1 */
    uint64_t min_changes, excess_changes, homoplasic_sites;
    double ci;                         /* consistency index min_changes / total_changes; 0.0 when not spanning or no changes */
} ps_parsimony_t;
/* One core handle and, or NULL, the accessory handle of the same individuals on the same device (the reference has no such
 * function; population.rs:443, :840-863).  site_changes: ncols; site_hist: PS_PARS_BINS; branch_*: pop_size + merges;
 * gene_*: the accessory handle's genes.  Every output but `out` may be NULL, and what is not asked for launches no work of its
 * own; the gene outputs and the branch gains / losses need `acc`.  Leaves are mapped through each handle's own row order.  A
 * site-shard core handle answers for its own sites, without an accessory handle (with one: ps_multi_tree_parsimony).  Ordered
 * behind all queued work of both handles; changes no state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible. */
int ps_tree_parsimony(ps_population *core, ps_population *acc, const uint32_t *left, const uint32_t *right, uint64_t merges,
                      ps_parsimony_t *out, uint32_t *site_changes, uint64_t *site_hist, uint64_t *branch_changes, uint32_t *gene_changes,
                      uint32_t *gene_gains, uint32_t *gene_losses, uint64_t *branch_gains, uint64_t *branch_losses);
/* The same for the two matrices of a simulation (the reference has no such function; population.rs:443, :840-863) */
int ps_sim_tree_parsimony(ps_sim *s, const uint32_t *left, const uint32_t *right, uint64_t merges, ps_parsimony_t *out,
                          uint32_t *site_changes, uint64_t *site_hist, uint64_t *branch_changes, uint32_t *gene_changes,
                          uint32_t *gene_gains, uint32_t *gene_losses, uint64_t *branch_gains, uint64_t *branch_losses);
/* The same for a sharded run (the reference has no such function; population.rs:443, :840-863): every shard answers for its own
 * sites, the u64 arrays and the summary integers add (max_changes: the largest), site_changes concatenates in site order
 * (core_size sites), ci is formed once; the genes from shard 0's accessory replica. */
int ps_multi_tree_parsimony(ps_multi *m, const uint32_t *left, const uint32_t *right, uint64_t merges, ps_parsimony_t *out,
                            uint32_t *site_changes, uint64_t *site_hist, uint64_t *branch_changes, uint32_t *gene_changes,
                            uint32_t *gene_gains, uint32_t *gene_losses, uint64_t *branch_gains, uint64_t *branch_losses);
/* device ms of the last ps_tree_parsimony on this core handle (each shard's own after the ps_multi form; HIP events; the
 * reference has no such function; population.rs:443): the upload of the schedule, the core pass, the gene pass (0.0 without
 * one).  PS_ERR_STATE before any call. */
int ps_tree_parsimony_timing(ps_population *core, double *schedule_ms, double *core_ms, double *gene_ms);
/* The merge list of a linkage tree (host only, no device is touched; the reference has no such function; population.rs:787-837):
 * Kruskal over the edges (lo[k], hi[k]) of ps_linkage_tree in their given order; merge k joins the clusters of edge k, left the
 * one with the smaller smallest row (ps_upgma_tree's convention).  left, right: room for `edges` values.  An edge inside one
 * cluster, a row >= pop_size or more than pop_size - 1 edges is PS_ERR_INVALID. */
int ps_merges_from_tree(const uint32_t *lo, const uint32_t *hi, uint64_t edges, uint64_t pop_size, uint32_t *left, uint32_t *right,
                        uint64_t *merges);
/* The merge list of a comb (host only; the reference has no such function; population.rs:443): the positions r with coal[r] !=
 * PS_GEN_BEYOND in (coal ascending, r ascending) order; merge k joins the two contiguous intervals of internal rows that meet
 * between r and r + 1, left the left interval; leaves are order[r]; height[k] (may be NULL) = coal[r].  Equal times, which
 * ps_genealogy_newick prints as one multifurcation, are resolved left to right in comb order.  left, right, height: room for
 * pop_size - 1 values.  order must be a permutation of 0 .. pop_size - 1. */
int ps_merges_from_genealogy(const uint32_t *order, const uint32_t *coal, uint64_t pop_size, uint32_t *left, uint32_t *right,
                             uint32_t *height, uint64_t *merges);
/* The schedule the kernel runs by (host only; the reference has no such function; population.rs:443): level_of[k] of merge k =
 * 1 + the larger of its children's levels, leaves at 0; *levels = the largest.  The tree rules above apply. */
int ps_parsimony_schedule(const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, uint32_t *level_of,
                          uint32_t *levels);
/* The plain sequential restatement on the host (no device is touched, as ps_diversity_from_counts; the reference has no such
 * function; population.rs:443, :840-863), through the same per-node functions as the kernel.  rows: individual-major pop_size x
 * cols bytes, row k = leaf k.  genes == 0: the bytes are core cells and site_changes, site_hist, branch_changes are filled (the
 * gene outputs must be NULL); genes == 1: a byte is the presence (non-zero) of a gene and gene_changes .. branch_losses are
 * filled (the core outputs must be NULL).  Any output may be NULL. */
int ps_parsimony_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, int genes, const uint32_t *left, const uint32_t *right,
                           uint64_t merges, ps_parsimony_t *out, uint32_t *site_changes, uint64_t *site_hist, uint64_t *branch_changes,
                           uint32_t *gene_changes, uint32_t *gene_gains, uint32_t *gene_losses, uint64_t *branch_gains,
                           uint64_t *branch_losses);

/* Comparison of two trees over the same leaves (docs/TREE_COMPARISON.md): how well one tree -- an inferred one -- recovers another
 * -- the recorded genealogy: the cophenetic agreement over ALL pairs of leaves, the rooted triplets both resolve alike, the clades
 * they share.  The reference has no such function (its trees are implicit in the parent draws of population.rs:443).
 * Tree: a merge list as ps_tree_parsimony takes it (the rules above apply; forests are accepted, leaves are rows of the
 * reference's row order), with a value per merge: 1 <= val[k] <= 262143 (2^18 - 1) and val[parent] >= val[child], else
 * PS_ERR_INVALID; val == NULL means val[k] = k + 1, the merge rank.  Equal values on a parent and its child are one
 * multifurcating node.
 * v_T(i, j) = the value of the lowest common ancestor of leaves i, j in T; i, j in different trees of a forest are "not joined".
 * The clade C_T(i, j) of a joined pair = the leaves below the highest ancestor of that merge with the same value (its tie-top).
 *   joined_*            the pairs i < j by the trees that join them
 *   sum_a .. sum_ab     over the pairs joined in both: sums of v_A, v_B, v_A^2, v_B^2, v_A v_B
 *   joint[(bins_a + 1)(bins_b + 1)]   pairs by (bin of v_A, bin of v_B), bin = ps_clock_time_bin's min(B - 1, floor((v - 1) B / S)),
 *                       S the span (0: the tree's largest value); row bins_a / column bins_b: not joined in A / in B
 *   cophenetic_r        (n sum_ab - sum_a sum_b) / sqrt((n sum_aa - sum_a^2)(n sum_bb - sum_b^2)), n = joined_both, the integer
 *                       terms exact in 128 bits; 0.0 when n = 0 or a variance term is 0
 *   triplets != 0:      {i, j, k} is resolved as ij|k in T iff i, j are joined and v(i, j) < v(i, k) (another tree of the forest:
 *                       infinitely far).  resolved_a = sum over the pairs joined in A of N - |C_A(i, j)|, resolved_b alike;
 *                       shared_triplets = sum over the pairs joined in both of N - |C_A u C_B|: every triple both trees resolve
 *                       alike, once; triples = C(N, 3); triplet_recall = shared / resolved_a, triplet_precision = shared /
 *                       resolved_b (0.0 on a zero denominator).  triplets == 0: the fields are 0.
 *   clades_a, clades_b  the tie-top merges of each tree; shared_clades those with equal leaf sets; rf_distance = clades_a +
 *                       clades_b - 2 shared; clade_recall = shared / clades_a, clade_precision = shared / clades_b
 *   in_b[merges_a]      (may be NULL) 1 iff merge k of A is a tie-top whose leaf set is a clade of B; in_a[merges_b] the same swapped
 * Every integer is exact and independent of the launch geometry; the doubles are formed once from the integers.
 * PS_ERR_INVALID: a null required argument, a bad tree or value, bins < 1 or > 1024, (bins_a + 1)(bins_b + 1) > 16384, a span >= 2^32. */
typedef struct {
    uint32_t bins_a, bins_b;           /* value bins per tree */
    uint64_t span_a, span_b;           /* 0: the tree's largest value */
    int32_t triplets;                  /* != 0: the triplet sums as well (a rank table of (N + 1)^2 u16 on the device) */
} ps_tree_compare_params;
typedef struct {
    uint64_t pop_size, merges_a, merges_b, pairs;      /* N, M_A, M_B, N (N - 1) / 2 */
    uint64_t joined_both, joined_a_only, joined_b_only, joined_neither;
    uint64_t sum_a, sum_b, sum_aa, sum_bb, sum_ab;
    uint64_t triples, resolved_a, resolved_b, shared_triplets;
    uint64_t clades_a, clades_b, shared_clades, rf_distance;
    uint64_t bins_a, bins_b, span_a, span_b;           /* the spans as used */
    double cophenetic_r, triplet_recall, triplet_precision, clade_recall, clade_precision;
} ps_tree_compare_t;
/* Two trees over the pop_size leaves of `any` (the reference has no such function; population.rs:443): any handle -- it supplies
 * the device, the stream and the scratch, and only its pop_size is read.  One kernel over all pairs behind two sparse tables
 * (and the rank table).  Ordered behind the handle's queued work; changes no state.  PS_ERR_OOM names the bytes it could not
 * allocate.  PS_ERR_NO_DEVICE before anything else when no GPU is visible. */
int ps_tree_compare(ps_population *any, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a, uint64_t merges_a,
                    const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b, uint64_t merges_b,
                    const ps_tree_compare_params *prm, ps_tree_compare_t *out, uint64_t *joint, uint8_t *in_b, uint8_t *in_a);
/* The same on the core handle of a simulation (the reference has no such function; population.rs:443) */
int ps_sim_tree_compare(ps_sim *s, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a, uint64_t merges_a,
                        const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b, uint64_t merges_b,
                        const ps_tree_compare_params *prm, ps_tree_compare_t *out, uint64_t *joint, uint8_t *in_b, uint8_t *in_a);
/* The same on shard 0's core handle of a sharded run: trees are global (the reference has no such function; population.rs:443) */
int ps_multi_tree_compare(ps_multi *m, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a, uint64_t merges_a,
                          const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b, uint64_t merges_b,
                          const ps_tree_compare_params *prm, ps_tree_compare_t *out, uint64_t *joint, uint8_t *in_b, uint8_t *in_a);
/* The plain sequential restatement over all pairs on the host (no device is touched, as ps_parsimony_from_rows; the reference
 * has no such function; population.rs:443), through the same checks, leaf orders, clades and finish as the device path.  With
 * triplets it holds (pop_size + 1)^2 u16 on the host. */
int ps_tree_compare_from_merges(uint64_t pop_size, const uint32_t *left_a, const uint32_t *right_a, const uint32_t *val_a,
                                uint64_t merges_a, const uint32_t *left_b, const uint32_t *right_b, const uint32_t *val_b,
                                uint64_t merges_b, const ps_tree_compare_params *prm, ps_tree_compare_t *out, uint64_t *joint,
                                uint8_t *in_b, uint8_t *in_a);
/* Values for ps_tree_compare from the heights of ps_upgma_tree or the sorted edges of ps_linkage_tree (host only; the reference
 * has no such function; population.rs:787-837): the heights num[k] / den[k] must not decrease in k under the linkage tree's
 * comparison (num1 den2 against num2 den1, here in 128 bits; den == 0 is undefined: above every defined height and equal to
 * itself), else PS_ERR_INVALID.  levels[0] = 1, plus 1 at every strict increase (dense ranks); *distinct (may be NULL) = the last. */
int ps_levels_from_heights(const uint64_t *num, const uint64_t *den, uint64_t merges, uint32_t *levels, uint64_t *distinct);
/* device ms of the last ps_tree_compare on this handle (HIP events; the reference has no such function; population.rs:443): the
 * uploads and the tables, the pass over all pairs.  PS_ERR_STATE before any call. */
int ps_tree_compare_timing(ps_population *any, double *tables_ms, double *pairs_ms);

/* Parsimony tree search (docs/PARSIMONY_SEARCH.md): nearest-neighbour interchanges (NNI) of any spanning tree towards a local
 * optimum of its Fitch length over the core sites.  The reference has no such function (its trees are implicit in the parent
 * draws of population.rs:443; the columns are those of population.rs:840-863).
 * Tree: a merge list as ps_tree_parsimony takes it (the rules above apply), SPANNING: merges == pop_size - 1, and 2 <= pop_size
 * <= PS_NNI_MAX_POP (two LDS dwords per node); else PS_ERR_INVALID.  States: the five class bits of a core cell.
 * Candidates of merge k, node c = pop_size + k with children a = left[k], b = right[k], parent v and sibling s: none when c is
 * the root; below an inner node v kind 0 swaps b with s and kind 1 swaps a with s; below the root only its LEFT child beside an
 * internal s = (p, q) has them, kind 0 swaps b with p and kind 1 swaps b with q (the root stays on its edge).
 *   delta[2 k + kind]   total changes of the neighbour tree minus total changes of this tree over the handle's sites, exact;
 *                       PS_NNI_NONE where there is no candidate
 * Canonical form: internal nodes in (level as ps_parsimony_schedule defines it, smallest leaf of the clade) order, the k-th as
 * node pop_size + k, left the child whose clade has the smaller smallest leaf: one list per rooted topology.
 * Search: from the canonical form of the start tree, per round one pass (T and all deltas), the improving candidates in (delta,
 * node, kind) order taken greedily while the nodes they touch ({v, c, a, b, s}; {root, l, r, a, b, p, q} on the root's edge)
 * are unmarked, at most moves_per_round (0: no cap); a batch of several whose tree is longer than T + the best delta is
 * discarded (a rollback) and the best candidate applied alone.  It ends at a tree without an improving candidate
 * (local_optimum = 1) or after max_rounds rounds.  passes = rounds + rollbacks + 1.  Every integer is exact and independent of
 * the launch geometry, the sharding and the order of the individuals. */
#define PS_NNI_MAX_POP 8192u
#define PS_NNI_NONE INT64_MAX
typedef struct {
    uint32_t max_rounds;               /* >= 1 */
    uint32_t moves_per_round;          /* 0 = no cap */
} ps_nni_params;
typedef struct {
    uint64_t pop_size, sites, merges;  /* N; core sites this result covers; N - 1 */
    uint64_t rounds, passes, rollbacks;
    uint64_t moves;                    /* interchanges applied in all rounds (the move arrays hold the first move_cap) */
    uint64_t local_optimum;            /* 1 iff the returned tree has no improving candidate */
    uint64_t start_changes, total_changes;     /* T of the start tree and of the returned tree */
    uint64_t min_changes;              /* sum_s (classes_s - 1), as ps_parsimony_t */
    uint64_t candidates_last;          /* improving candidates of the last pass (0 at a local optimum) */
} ps_nni_t;
/* One pass on the list as given, not canonicalised (the reference has no such function; population.rs:443, :840-863): *total
 * = T, delta: 2 merges values.  A site-shard core handle answers for its own sites.  Ordered behind the handle's queued work;
 * changes no state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible. */
int ps_tree_nni_deltas(ps_population *core, const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t *total, int64_t *delta);
/* The search on one core handle (the reference has no such function; population.rs:443, :840-863).  out_left, out_right: the
 * returned tree, canonical, merges values each; round_changes: max_rounds + 1 values, [0] = T of the start tree, [r] = T after
 * round r; move_*: move_cap values each, move i of round move_round[i] (from 1) is candidate (move_node[i], move_kind[i]) of
 * that round's canonical tree with move_delta[i].  Every array may be NULL (the move arrays with move_cap = 0).  A pass reads
 * back 16 merges bytes; selection and surgery run on the host.  Ordered behind the handle's queued work; changes no state. */
int ps_tree_nni(ps_population *core, const uint32_t *left, const uint32_t *right, uint64_t merges, const ps_nni_params *prm, ps_nni_t *out,
                uint32_t *out_left, uint32_t *out_right, uint64_t *round_changes, uint32_t *move_round, uint32_t *move_node,
                uint32_t *move_kind, int64_t *move_delta, uint64_t move_cap);
/* The same on the core matrix of a simulation (the reference has no such function; population.rs:443, :840-863) */
int ps_sim_tree_nni(ps_sim *s, const uint32_t *left, const uint32_t *right, uint64_t merges, const ps_nni_params *prm, ps_nni_t *out,
                    uint32_t *out_left, uint32_t *out_right, uint64_t *round_changes, uint32_t *move_round, uint32_t *move_node,
                    uint32_t *move_kind, int64_t *move_delta, uint64_t move_cap);
/* The same for a sharded run (the reference has no such function; population.rs:443, :840-863): every shard passes over its own
 * sites, T and the deltas add on the host, one selection. */
int ps_multi_tree_nni(ps_multi *m, const uint32_t *left, const uint32_t *right, uint64_t merges, const ps_nni_params *prm, ps_nni_t *out,
                      uint32_t *out_left, uint32_t *out_right, uint64_t *round_changes, uint32_t *move_round, uint32_t *move_node,
                      uint32_t *move_kind, int64_t *move_delta, uint64_t move_cap);
/* device ms of the last ps_tree_nni or ps_tree_nni_deltas on this core handle, summed over its passes (each shard's own after
 * the ps_multi form; HIP events; the reference has no such function; population.rs:443): the uploads of the schedules, the
 * kernels.  PS_ERR_STATE before any call. */
int ps_tree_nni_timing(ps_population *core, double *schedule_ms, double *pass_ms);
/* One pass on the host (no device is touched, as ps_parsimony_from_rows; the reference has no such function; population.rs:443,
 * :840-863), through the same per-node functions as the kernel.  rows: individual-major pop_size x cols bytes, row k = leaf k. */
int ps_nni_deltas_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                            uint64_t merges, uint64_t *total, int64_t *delta);
/* The search on the host (no device is touched; the reference has no such function; population.rs:443, :840-863): the same loop,
 * selection and surgery as ps_tree_nni over host passes. */
int ps_nni_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right, uint64_t merges,
                     const ps_nni_params *prm, ps_nni_t *out, uint32_t *out_left, uint32_t *out_right, uint64_t *round_changes,
                     uint32_t *move_round, uint32_t *move_node, uint32_t *move_kind, int64_t *move_delta, uint64_t move_cap);
/* The canonical form of a spanning merge list (host only; the reference has no such function; population.rs:443).  A parent's id
 * is above its children's, so the list needs no values in ps_tree_compare.  out_left, out_right: merges values each. */
int ps_merges_canonical(const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, uint32_t *out_left,
                        uint32_t *out_right);
/* Candidate (node, kind) of the list as given applied, the result in canonical form (host only; the reference has no such
 * function; population.rs:443).  A node without candidates or kind > 1 is PS_ERR_INVALID. */
int ps_nni_apply(const uint32_t *left, const uint32_t *right, uint64_t merges, uint64_t pop_size, uint32_t node, uint32_t kind,
                 uint32_t *out_left, uint32_t *out_right);

/* Likelihood of a tree under the Jukes-Cantor model (docs/TREE_LIKELIHOOD.md): lnL of a spanning tree with branch lengths over
 * the core sites, every site's likelihood, the derivative sums of every branch, and maximum-likelihood branch lengths.  The
 * reference has no such function (its trees are implicit in the parent draws of population.rs:443; the columns are those of
 * population.rs:840-863, the substitution of a base by another base is population.rs:514-540).
 * Tree: a spanning merge list as ps_tree_nni takes it, 2 <= pop_size <= PS_LIK_MAX_POP (36 LDS bytes per node and 16 per branch);
 * else PS_ERR_INVALID.  length[pop_size + merges]: binary64, expected substitutions per site on the branch above every node, the
 * root's entry ignored, each used as min(max(t, PS_LIK_MIN_LENGTH), PS_LIK_MAX_LENGTH); NaN or infinity is PS_ERR_INVALID.
 * States: bytes 1, 2, 4, 8 are the bases; ANY other byte is missing data (partial (1, 1, 1, 1)) -- not a fifth state as in the
 * parsimony entries.
 *   site likelihood   mant * 2^exp, mant = the root's rescaled partial summed / 4; ln = log(mant) + exp ln 2
 *   branch_g[c]       sum over sites of r = B / (A + x_c B), the site likelihood being A + x_c B in x_c = exp(-4 t_c / 3)
 *   branch_h[c]       sum over sites of r r:  dlnL/dt_c = -(4 x / 3) g,  d2lnL/dt_c2 = (16 x x / 9)(-h) + (16 x / 9) g
 * Every site's (mant, exp) and r are the same bits on host and device (pansim_amd/csrc/jc_rule.h); the sums over sites are taken
 * in a fixed order per device (a repeated call returns the same bits) and differ from the host's by their rounding only. */
#define PS_LIK_MAX_POP 2048u
#define PS_LIK_MIN_LENGTH 1e-8
#define PS_LIK_MAX_LENGTH 10.0
typedef struct {
    uint32_t max_rounds;               /* >= 1 */
    double eps_lnl;                    /* > 0: an accepted round that gains less ends the optimisation */
} ps_ml_params;
typedef struct {
    uint64_t pop_size, sites, merges;  /* N; core sites this result covers; N - 1 */
    uint64_t clamped_lengths;          /* entries of the lengths given that the bounds changed */
    uint64_t missing_cells;            /* cells that are none of 1 / 2 / 4 / 8 */
    uint64_t rounds, passes, rollbacks;/* ps_tree_ml_lengths: accepted rounds, passes, halvings of the step; else 0, 1, 0 */
    uint64_t converged;                /* 1 iff the last accepted round gained less than eps_lnl */
    double lnl, start_lnl;             /* lnL with the returned (given) lengths, and with the start lengths */
    double tree_length;                /* sum of the used lengths */
} ps_likelihood_t;
/* One pass on one core handle (the reference has no such function; population.rs:443, :840-863).  site_mant: sites f64,
 * site_exp: sites i32, branch_g, branch_h: pop_size + merges f64 (the root's 0); each may be NULL and then costs nothing -- no
 * down pass runs unless branch_g or branch_h is asked for.  A site-shard core handle answers for its own sites.  Ordered behind
 * the handle's queued work; changes no state.  PS_ERR_NO_DEVICE before anything else when no GPU is visible; PS_ERR_OOM names
 * the bytes. */
int ps_tree_likelihood(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                       ps_likelihood_t *out, double *site_mant, int32_t *site_exp, double *branch_g, double *branch_h);
/* The same on the core matrix of a simulation (the reference has no such function; population.rs:443, :840-863) */
int ps_sim_tree_likelihood(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                           ps_likelihood_t *out, double *site_mant, int32_t *site_exp, double *branch_g, double *branch_h);
/* The same for a sharded run (the reference has no such function; population.rs:443, :840-863): every shard passes over its own
 * sites, the per-site arrays are concatenated, lnL, g and h add on the host in shard order. */
int ps_multi_tree_likelihood(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                             ps_likelihood_t *out, double *site_mant, int32_t *site_exp, double *branch_g, double *branch_h);
/* Maximum-likelihood branch lengths of the tree from the start lengths length_in (the reference has no such function;
 * population.rs:443, :840-863).  The right root child's length is added to the left's and held at PS_LIK_MIN_LENGTH; a round is
 * one pass with derivatives and one damped Newton step on every other branch at once (delta = -g_t / h_t where h_t < 0, else
 * sign(g_t) t; limited to [-t / 2, max(t, 1e-3)]; t' = clamp(t + lambda delta)); a pass that gives a lower lnL restores the
 * lengths, halves lambda and counts as a rollback, an accepted round sets lambda back to 1.  It ends when an accepted round
 * gains less than eps_lnl (converged = 1; a pass that gains exactly nothing ends it the same way without a round), after
 * max_rounds rounds, or when lambda < 2^-20.  length_out: pop_size + merges values (the root's 0); round_lnl: round_cap >=
 * max_rounds + 1 values, [0] = lnL at the start lengths, [r] = after round r, strictly increasing; either may be NULL. */
int ps_tree_ml_lengths(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                       const ps_ml_params *prm, ps_likelihood_t *out, double *length_out, double *round_lnl, uint64_t round_cap);
/* The same on the core matrix of a simulation (the reference has no such function; population.rs:443, :840-863) */
int ps_sim_tree_ml_lengths(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                           const ps_ml_params *prm, ps_likelihood_t *out, double *length_out, double *round_lnl, uint64_t round_cap);
/* The same for a sharded run (the reference has no such function; population.rs:443, :840-863): one Newton step on the sums of
 * the shards. */
int ps_multi_tree_ml_lengths(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                             const ps_ml_params *prm, ps_likelihood_t *out, double *length_out, double *round_lnl, uint64_t round_cap);
/* device ms of the last ps_tree_likelihood or ps_tree_ml_lengths on this core handle, summed over its passes (each shard's own
 * after the ps_multi form; HIP events; the reference has no such function; population.rs:443): the uploads of the schedule and
 * of x, the kernel, the sum of the workgroups' rows.  PS_ERR_STATE before any call. */
int ps_tree_likelihood_timing(ps_population *core, double *schedule_ms, double *pass_ms, double *reduce_ms);
/* One pass on the host (no device is touched; the reference has no such function; population.rs:443, :840-863), through the same
 * jc_rule.h functions as the kernel, the sites summed in ascending order.  rows: individual-major pop_size x cols bytes, row k =
 * leaf k. */
int ps_likelihood_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                            const double *length, uint64_t merges, ps_likelihood_t *out, double *site_mant, int32_t *site_exp,
                            double *branch_g, double *branch_h);
/* The optimiser on the host (no device is touched; the reference has no such function; population.rs:443, :840-863): the same loop
 * as ps_tree_ml_lengths over host passes. */
int ps_ml_lengths_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                            const double *length_in, uint64_t merges, const ps_ml_params *prm, ps_likelihood_t *out, double *length_out,
                            double *round_lnl, uint64_t round_cap);
/* Start lengths from the branch_changes of ps_tree_parsimony over `sites` sites (host only; the reference has no such function;
 * population.rs:514-540): with p = changes / sites, -3/4 ln(1 - 4 p / 3); PS_LIK_MAX_LENGTH from p = 0.74 on. */
int ps_jc_lengths_from_changes(const uint64_t *branch_changes, uint64_t nodes, uint64_t sites, double *length);

/* Likelihood of a tree under the simulator's own substitution process (docs/TREE_MODEL.md): F81 with base frequencies pi, a root
 * distribution rho and up to 8 rate categories per site.  The reference has no such function; the process is its core mutation,
 * which redraws a hit cell from {2, 4, 8} whatever the old allele was (population.rs:531: pi = (0, 1/3, 1/3, 1/3)), from a
 * founding genome uniform over {1, 2, 4, 8} (population.rs:201-203: rho = 1/4 each, not stationary).
 * P(t) = x I + (1 - x) 1 pi^T with x = exp(-(r t) / beta), beta = 1 - sum pi_a^2: lengths are expected substitutions per site at
 * rate 1 under pi, t / beta events per site; the tree, the lengths, their clamp and the missing-data rule are ps_tree_likelihood's.
 *   freq      pi: entries >= 0, at most one of them 0, summing to 1 within 1e-12
 *   root      rho: entries > 0 summing to 1 within 1e-12; equal to freq bit for bit = reversible (the root rule of ps_tree_ml_lengths)
 *   rate      r_k, finite and >= 0 (0: an invariant class); weight: w_k > 0 summing to 1 within 1e-12; categories: 1 <= K <= 8
 *   site_class  NULL: every site is a mixture of the K categories; else one u8 < K per core site -- of the handle in
 *             ps_tree_model_likelihood and the host entries, of the whole run (the global site index) in the ps_sim_ and ps_multi_
 *             forms -- and site_classes = their count: the site's likelihood is its class's alone
 * Anything else is PS_ERR_INVALID with a message that names the field.
 *   site likelihood   assigned: the class's (mant, exp); mixture: e = the largest exponent of a category of non-zero mantissa,
 *                     mant = sum_k w_k ldexp(mant_k, e_k - e), not renormalised; posterior post_k = w_k ldexp(..) / mant
 *   site_rate         sum_k post_k r_k (assigned: r of the class)
 *   branch_g[c]       sum_s D_sc, D_sc = sum_k post_sk ((r_k x_ck) ratio_sck), ratio = (D - A) / ((1 - x) A + x D)
 *   branch_h[c]       sum_s D_sc^2;   branch_q[c] = sum_s sum_k post_sk r_k ((r_k x_ck) ratio_sck)
 *                     dlnL/dt_c = -g / beta,  d2lnL/dt_c2 = (q - h) / beta^2
 * With pi = rho = 1/4, K = 1, r = w = 1 every site's (mant, exp) is the same bits as ps_tree_likelihood's.  Every site's values
 * are the same bits on host and device (pansim_amd/csrc/subst_rule.h); sums over sites are taken in a fixed order per device.
 * With derivatives pop_size <= PS_MODEL_MAX_POP_DERIV (32 LDS bytes per branch instead of 16), else PS_LIK_MAX_POP. */
#define PS_MODEL_MAX_CATEGORIES 8u
#define PS_MODEL_MAX_POP_DERIV 1536u
typedef struct {
    double freq[4], root[4];
    uint32_t categories;
    double rate[8], weight[8];
    const uint8_t *site_class;         /* NULL: mixture */
    uint64_t site_classes;
} ps_subst_model;
typedef struct {
    uint64_t pop_size, sites, merges;  /* as ps_likelihood_t */
    uint64_t clamped_lengths, missing_cells;
    uint64_t rounds, passes, rollbacks, converged;
    uint64_t categories, classed;      /* K; 1 iff site_class was given */
    double lnl, start_lnl, tree_length;
    double beta, mean_rate;            /* 1 - sum pi_a^2; sum_k w_k r_k (reported, not enforced) */
} ps_model_likelihood_t;
/* One pass on one core handle (the reference has no such function; population.rs:531, :201-203).  site_mant, site_rate: sites
 * f64, site_exp: sites i32, branch_g, branch_h, branch_q: pop_size + merges f64 (the root's 0); each may be NULL and then costs
 * nothing -- no down pass (and no second phase of a mixture site) runs unless a branch output is asked for.  A site-shard core
 * handle answers for its own sites.  Ordered behind the handle's queued work; changes no state.  PS_ERR_NO_DEVICE before
 * anything else when no GPU is visible; PS_ERR_OOM names the bytes. */
int ps_tree_model_likelihood(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                             const ps_subst_model *model, ps_model_likelihood_t *out, double *site_mant, int32_t *site_exp,
                             double *site_rate, double *branch_g, double *branch_h, double *branch_q);
/* The same on the core matrix of a simulation (the reference has no such function; population.rs:531, :201-203) */
int ps_sim_tree_model_likelihood(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                 const ps_subst_model *model, ps_model_likelihood_t *out, double *site_mant, int32_t *site_exp,
                                 double *site_rate, double *branch_g, double *branch_h, double *branch_q);
/* The same for a sharded run (the reference has no such function; population.rs:531, :201-203): every shard passes over its own
 * sites with its slice of site_class, the per-site arrays are concatenated, lnL, g, h and q add on the host in shard order. */
int ps_multi_tree_model_likelihood(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                   const ps_subst_model *model, ps_model_likelihood_t *out, double *site_mant, int32_t *site_exp,
                                   double *site_rate, double *branch_g, double *branch_h, double *branch_q);
/* Maximum-likelihood branch lengths under the model (the reference has no such function; population.rs:531, :201-203): the loop,
 * the step limits, the rollback and the stopping rules of ps_tree_ml_lengths, fed with (dlnL/dt, d2lnL/dt2) of the model.  A
 * reversible model (root == freq bit for bit) folds the right root child's length into the left's and holds it at
 * PS_LIK_MIN_LENGTH; otherwise both root branches are optimised. */
int ps_tree_model_ml_lengths(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                             const ps_subst_model *model, const ps_ml_params *prm, ps_model_likelihood_t *out, double *length_out,
                             double *round_lnl, uint64_t round_cap);
/* The same on the core matrix of a simulation (the reference has no such function; population.rs:531, :201-203) */
int ps_sim_tree_model_ml_lengths(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                 const ps_subst_model *model, const ps_ml_params *prm, ps_model_likelihood_t *out, double *length_out,
                                 double *round_lnl, uint64_t round_cap);
/* The same for a sharded run (the reference has no such function; population.rs:531, :201-203): one Newton step on the sums of
 * the shards. */
int ps_multi_tree_model_ml_lengths(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                                   const ps_subst_model *model, const ps_ml_params *prm, ps_model_likelihood_t *out, double *length_out,
                                   double *round_lnl, uint64_t round_cap);
/* device ms of the last ps_tree_model_likelihood or ps_tree_model_ml_lengths on this core handle, summed over its passes (HIP
 * events; the reference has no such function; population.rs:531): the uploads, the kernel, the sum of the workgroups' rows.
 * Its own slots: ps_tree_likelihood_timing keeps its meaning.  PS_ERR_STATE before any call. */
int ps_tree_model_timing(ps_population *core, double *schedule_ms, double *pass_ms, double *reduce_ms);
/* One pass on the host (no device is touched; the reference has no such function; population.rs:531, :201-203), through the same
 * subst_rule.h functions as the kernel, the sites summed in ascending order.  rows: individual-major pop_size x cols bytes. */
int ps_model_likelihood_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                  const double *length, uint64_t merges, const ps_subst_model *model, ps_model_likelihood_t *out,
                                  double *site_mant, int32_t *site_exp, double *site_rate, double *branch_g, double *branch_h,
                                  double *branch_q);
/* The optimiser on the host (no device is touched; the reference has no such function; population.rs:531, :201-203) */
int ps_model_ml_lengths_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                  const double *length_in, uint64_t merges, const ps_subst_model *model, const ps_ml_params *prm,
                                  ps_model_likelihood_t *out, double *length_out, double *round_lnl, uint64_t round_cap);
/* Start lengths from the branch_changes of ps_tree_parsimony over `sites` sites under freq[4] (host only; the reference has no
 * such function; population.rs:531): with p = changes / sites, -beta ln(1 - p / beta); PS_LIK_MAX_LENGTH from p = 0.98 beta on,
 * PS_LIK_MIN_LENGTH without sites. */
int ps_f81_lengths_from_changes(const uint64_t *branch_changes, uint64_t nodes, uint64_t sites, const double *freq, double *length);

/* Likelihood tree search (docs/LIKELIHOOD_SEARCH.md): nearest-neighbour interchanges of a spanning tree with branch lengths
 * towards a local optimum of its likelihood under ps_subst_model over the core sites -- the likelihood twin of ps_tree_nni.  The
 * reference has no such function (its trees are implicit in the parent draws of population.rs:443; the process is its core
 * mutation, population.rs:531, from the founding genome of population.rs:201-203).
 * Tree, lengths, clamp, states and model: as ps_tree_model_likelihood takes them, 2 <= pop_size <= PS_MODEL_NNI_MAX_POP (4 LDS
 * bytes per leaf and 140 per merge); else PS_ERR_INVALID.  Candidates, kinds and the root's edge: the table of ps_tree_nni.
 * An interchange changes none of the four pieces around its edge -- the messages of the three subtrees and the message from
 * above -- nor any length: every subtree keeps the length of the branch above it, the edge keeps its own, the root stays on its
 * edge.  So one pass gives, per candidate, the exact ratio of the likelihood of the neighbour tree to this tree's:
 *   site ratio        assigned: l' / l of the class; mixture: sum_k post_sk l'_sk / l_sk, k ascending (= l'_s / l_s); a category
 *                     of likelihood 0 adds nothing; a site of likelihood 0 in this tree is left out of every product
 *   delta_mant/exp    [2 k + kind] of merge k: the product of the site ratios as mantissa in [1/2, 1) times 2^exp, multiplied
 *                     and rescaled after every site (frexp; no log per site); the gain is log(mant) + exp ln 2; mant = 0.0
 *                     where there is no candidate
 * Every site ratio is the same bits on host and device (pansim_amd/csrc/subst_rule.h); the products are taken in a fixed order
 * per device (a repeated call returns the same bits) and differ from the host's by their grouping only.
 * Search: from the canonical form of the start tree (ps_merges_canonical, the lengths carried with their nodes), per round:
 * with length_rounds > 0 up to that many rounds of the optimiser of ps_tree_model_ml_lengths (eps_lnl = eps_gain), one pass,
 * the candidates with gain > eps_gain in (gain descending, node, kind) order taken greedily while the nodes they touch are
 * unmarked, at most moves_per_round (0: no cap); a batch of several whose tree (after its own length rounds) has lnL below
 * this tree's lnL + the best gain is discarded (a rollback) and the best candidate applied alone.  It ends at a tree without
 * such a candidate (local_optimum = 1), after max_rounds rounds, or when a round fails to raise lnL.  A start tree whose lnL
 * is not finite is PS_ERR_INVALID. */
#define PS_MODEL_NNI_MAX_POP 1024u
typedef struct {
    uint32_t max_rounds;               /* >= 1 */
    uint32_t moves_per_round;          /* 0 = no cap */
    uint32_t length_rounds;            /* 0 = the lengths are never re-optimised */
    double eps_gain;                   /* > 0: a candidate must gain more */
} ps_ml_nni_params;
typedef struct {
    uint64_t pop_size, sites, merges;  /* N; core sites this result covers; N - 1 */
    uint64_t rounds, passes;           /* accepted rounds; passes of the search kernel = rounds + rollbacks + 1 (+ 1 when a round failed) */
    uint64_t length_passes;            /* passes of the likelihood kernel: the start tree's lnL and the length rounds */
    uint64_t rollbacks, moves;         /* discarded batches; interchanges applied in all rounds */
    uint64_t local_optimum;            /* 1 iff the returned tree has no candidate above eps_gain */
    uint64_t candidates_last;          /* candidates above eps_gain of the last pass */
    uint64_t zero_sites;               /* sites of likelihood 0 in the returned tree */
    uint64_t clamped_lengths, missing_cells;
    double start_lnl, lnl;             /* lnL of the start tree with the lengths given, and of the returned tree and lengths */
} ps_ml_nni_t;
/* One pass on the list as given, not canonicalised (the reference has no such function; population.rs:443, :531): *lnl,
 * delta_mant, delta_exp: 2 merges values each, *zero_sites (may be NULL) = the sites of likelihood 0.  A site-shard core handle
 * answers for its own sites.  Ordered behind the handle's queued work; changes no state.  PS_ERR_NO_DEVICE before anything else
 * when no GPU is visible; PS_ERR_OOM names the bytes. */
int ps_tree_model_nni_deltas(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                             const ps_subst_model *model, double *lnl, double *delta_mant, int64_t *delta_exp, uint64_t *zero_sites);
/* The same on the core matrix of a simulation (the reference has no such function; population.rs:443, :531) */
int ps_sim_tree_model_nni_deltas(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                 const ps_subst_model *model, double *lnl, double *delta_mant, int64_t *delta_exp, uint64_t *zero_sites);
/* The same for a sharded run (the reference has no such function; population.rs:443, :531): every shard passes over its own
 * sites, the shards' products multiply on the host in shard order, lnL adds. */
int ps_multi_tree_model_nni_deltas(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                   const ps_subst_model *model, double *lnl, double *delta_mant, int64_t *delta_exp, uint64_t *zero_sites);
/* The search on one core handle (the reference has no such function; population.rs:443, :531).  out_left, out_right: the
 * returned tree, canonical, merges values each; length_out: pop_size + merges values, its lengths (the root's 0); round_lnl:
 * max_rounds + 1 values, [0] = lnL of the first pass, [r] = after round r, strictly increasing; move_*: move_cap values each,
 * move i of round move_round[i] (from 1) is candidate (move_node[i], move_kind[i]) of that round's canonical tree with
 * move_gain[i].  Every array may be NULL (the move arrays with move_cap = 0).  Selection and surgery run on the host.  Ordered
 * behind the handle's queued work; changes no state. */
int ps_tree_model_nni(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                      const ps_subst_model *model, const ps_ml_nni_params *prm, ps_ml_nni_t *out, uint32_t *out_left, uint32_t *out_right,
                      double *length_out, double *round_lnl, uint32_t *move_round, uint32_t *move_node, uint32_t *move_kind,
                      double *move_gain, uint64_t move_cap);
/* The same on the core matrix of a simulation (the reference has no such function; population.rs:443, :531) */
int ps_sim_tree_model_nni(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                          const ps_subst_model *model, const ps_ml_nni_params *prm, ps_ml_nni_t *out, uint32_t *out_left, uint32_t *out_right,
                          double *length_out, double *round_lnl, uint32_t *move_round, uint32_t *move_node, uint32_t *move_kind,
                          double *move_gain, uint64_t move_cap);
/* The same for a sharded run (the reference has no such function; population.rs:443, :531): one selection on the combined
 * products, one Newton step on the sums of the shards. */
int ps_multi_tree_model_nni(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length_in, uint64_t merges,
                            const ps_subst_model *model, const ps_ml_nni_params *prm, ps_ml_nni_t *out, uint32_t *out_left, uint32_t *out_right,
                            double *length_out, double *round_lnl, uint32_t *move_round, uint32_t *move_node, uint32_t *move_kind,
                            double *move_gain, uint64_t move_cap);
/* device ms of the search kernel's passes of the last ps_tree_model_nni or ps_tree_model_nni_deltas on this core handle, summed
 * (each shard's own after the ps_multi form; HIP events; the reference has no such function; population.rs:443): the uploads,
 * the kernels, the products of the workgroups' rows.  The length rounds report to ps_tree_model_timing.  PS_ERR_STATE before
 * any call. */
int ps_tree_model_nni_timing(ps_population *core, double *schedule_ms, double *pass_ms, double *reduce_ms);
/* One pass on the host (no device is touched; the reference has no such function; population.rs:443, :531), through the same
 * subst_rule.h functions as the kernel, the sites multiplied in ascending order.  rows: individual-major pop_size x cols bytes. */
int ps_model_nni_deltas_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                  const double *length, uint64_t merges, const ps_subst_model *model, double *lnl, double *delta_mant,
                                  int64_t *delta_exp, uint64_t *zero_sites);
/* The search on the host (no device is touched; the reference has no such function; population.rs:443, :531): the same loop,
 * selection, surgery and length rounds as ps_tree_model_nni over host passes. */
int ps_model_nni_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                           const double *length_in, uint64_t merges, const ps_subst_model *model, const ps_ml_nni_params *prm,
                           ps_ml_nni_t *out, uint32_t *out_left, uint32_t *out_right, double *length_out, double *round_lnl,
                           uint32_t *move_round, uint32_t *move_node, uint32_t *move_kind, double *move_gain, uint64_t move_cap);
/* The canonical form of a spanning merge list with its lengths (host only; the reference has no such function;
 * population.rs:443): a length belongs to the node below its branch and follows it to its new id.  length, length_out: pop_size
 * + merges values. */
int ps_merges_canonical_lengths(const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges, uint64_t pop_size,
                                uint32_t *out_left, uint32_t *out_right, double *length_out);
/* Candidate (node, kind) of the list as given applied, the result and its lengths in canonical form (host only; the reference
 * has no such function; population.rs:443): every subtree keeps the length of the branch above it. */
int ps_nni_apply_lengths(const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges, uint64_t pop_size, uint32_t node,
                         uint32_t kind, uint32_t *out_left, uint32_t *out_right, double *length_out);

/* Marginal ancestral states (docs/ANCESTRAL_STATES.md): the sequences at the inner nodes of a spanning tree with branch lengths,
 * reconstructed under ps_subst_model.  The reference has no such function (its ancestors are overwritten generation by
 * generation, population.rs:443; the process is its core mutation, population.rs:531, from the founding genome of
 * population.rs:201-203).  Tree, lengths, clamp, states, missing-data rule and model: as ps_tree_model_likelihood takes them;
 * the list is spanning (merges = pop_size - 1) and is not canonicalised: node pop_size + k is merge k as given.
 * pop_size <= PS_ANC_MAX_POP for assigned sites (site_class given, or one category: 12 LDS bytes per leaf and 56 per merge),
 * <= PS_ANC_MAX_POP_MIX for a mixture (32 more per merge); else PS_ERR_INVALID.
 *   node posterior    in a category, from T (the message into the node from above, rho at the root) and the messages ml, mr of
 *                     its children: w_a = (T_a ml_a) mr_a, p_a = w_a / sum_a w_a; a mixture site: p_a = sum_k post_sk p_{k,a}, k
 *                     ascending, post of ps_tree_model_likelihood; a category whose sum is 0 adds nothing
 *   state             per (site, inner node) the one-hot byte 1 << argmax_a p_a, exact ties to the lowest a; byte 0 where
 *                     pmax < min_posterior (counted in masked_cells; min_posterior = 0 masks nothing)
 *   node_conf[k]      sum_s pmax of merge k (masked cells included)
 *   branch_diff[c]    sum_s of the posterior probability that the two ends of the branch above node c differ,
 *                     sum_k post_sk (1 - x) max(A - S, 0) / ((1 - x) A + x D), S = sum_a pi_a (U_a L_a); the root's 0
 * A site of likelihood 0 in this tree (an assigned invariant class at a variable site) is byte 0 at every node, adds nothing to
 * any sum and is counted in zero_sites.  Every cell's posterior is the same bits on host and device
 * (pansim_amd/csrc/subst_rule.h); sums over sites are taken in a fixed order per device. */
#define PS_ANC_MAX_POP 2304u
#define PS_ANC_MAX_POP_MIX 1536u
typedef struct {
    uint64_t pop_size, sites, merges;  /* N; core sites this result covers; N - 1 */
    uint64_t categories, classed;      /* K; 1 iff site_class was given */
    uint64_t masked_cells, zero_sites;
    uint64_t missing_cells, clamped_lengths;   /* as ps_model_likelihood_t */
    double lnl;                        /* as ps_tree_model_likelihood returns it */
    double mean_conf;                  /* sum node_conf / (merges (sites - zero_sites)) */
    double total_diff;                 /* sum branch_diff */
} ps_ancestral_t;
/* One pass on one core handle (the reference has no such function; population.rs:443, :531, :201-203).  *anc: a NEW core handle
 * of pop_size = merges with the source's ncols, col_offset, global_cols and core_genes, made as ps_population_pool makes one (a
 * stream of its own, output order = internal order, no rates set), row k = node pop_size + k, filled on the device; destroyed with
 * ps_population_destroy in any order relative to its source; its one-hot flag is set only if the source's is and no cell was
 * written 0.  anc may be NULL: no matrix is allocated or stored.  node_conf: merges f64, branch_diff: pop_size + merges f64; each
 * may be NULL.  A site-shard core handle answers for its own sites.  The source is read behind its queued work and never written.
 * PS_ERR_NO_DEVICE before anything else when no GPU is visible; PS_ERR_OOM names the bytes. */
int ps_tree_ancestral_states(ps_population *core, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                             const ps_subst_model *model, double min_posterior, ps_ancestral_t *out, ps_population **anc, double *node_conf,
                             double *branch_diff);
/* The same on the core matrix of a simulation (the reference has no such function; population.rs:443, :531); site_class goes by
 * the global site */
int ps_sim_tree_ancestral_states(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                 const ps_subst_model *model, double min_posterior, ps_ancestral_t *out, ps_population **anc,
                                 double *node_conf, double *branch_diff);
/* The same for a sharded run (the reference has no such function; population.rs:443, :531): *anc is a WHOLE handle on shard 0's
 * device, every shard's block of site rows placed as ps_multi_subset places it; the sums add on the host in shard order. */
int ps_multi_tree_ancestral_states(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                   const ps_subst_model *model, double min_posterior, ps_ancestral_t *out, ps_population **anc,
                                   double *node_conf, double *branch_diff);
/* device ms of the last ps_tree_ancestral_states on this core handle (each shard's own after the ps_multi form; HIP events; the
 * reference has no such function; population.rs:443): the uploads, the kernel with its stores, the sum of the workgroups' rows.
 * PS_ERR_STATE before any call. */
int ps_ancestral_states_timing(ps_population *core, double *upload_ms, double *pass_ms, double *reduce_ms);
/* One pass on the host (no device is touched; the reference has no such function; population.rs:443, :531), through the same
 * subst_rule.h functions as the kernel, the sites summed in ascending order.  rows: individual-major pop_size x cols bytes;
 * anc_rows (may be NULL): individual-major merges x cols bytes, row k = node pop_size + k. */
int ps_ancestral_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                           const double *length, uint64_t merges, const ps_subst_model *model, double min_posterior, ps_ancestral_t *out,
                           uint8_t *anc_rows, double *node_conf, double *branch_diff);

/* Gene gain and loss on a tree (docs/GENE_MODEL.md): the likelihood of the ACCESSORY matrix on a spanning tree with branch lengths
 * under a two-state Markov chain per gene (0 = absent, 1 = present), its rates fitted, and the gene content of the inner nodes.
 * The reference has no such function; the process is its gene gain / loss, a flip of a cell with p = (1 - exp(-2 lambda_c / |c|))
 * / 2 per generation (population.rs:505), which is this model with pi = (1/2, 1/2) and r_c = lambda_c / |c| for t in
 * generations, the compartments as rate classes.  P(t) = x I + y 1 pi^T, x = exp(-(r t) / beta), y = 1 - x formed as
 * -expm1(-(r t) / beta) (full precision on the shortest branches), beta = 1 - pi_0^2 - pi_1^2: the gain rate is r pi_1 / beta, the
 * loss rate r pi_0 / beta.
 *   freq      pi: both entries > 0, summing to 1 within 1e-12;   root: rho, both > 0, summing to 1 within 1e-12
 *   rate      r_k, finite and >= 0; weight: w_k > 0 summing to 1 within 1e-12; categories: 1 <= K <= 8
 *   gene_class  NULL: every gene is a mixture of the K classes; else one u8 < K per gene and gene_classes = their count
 * Anything else is PS_ERR_INVALID with a message that names the field.  Lengths: finite (else PS_ERR_INVALID), clamped below at
 * 1e-8 (counted in clamped_lengths) and NOT above: a tree in generations is legitimate input.  The tree: as ps_tree_parsimony
 * takes it, spanning (merges = pop_size - 1), leaf i = output row i; any byte but 0 of the host forms is present.
 * pop_size <= PS_GENE_MAX_POP assigned (gene_class given, or one class), <= PS_GENE_MAX_POP_MIX for a mixture; else PS_ERR_INVALID.
 *   gene likelihood   assigned: the class's (mant, exp); mixture, posterior and mean rate: as ps_tree_model_likelihood forms them
 *   gene_post         genes x K: the class posteriors (assigned: 1 at the gene's class)
 *   node posterior    w_a = (T_a ml_a) mr_a, p_a = w_a / (w_0 + w_1); mixture: sum_k post_k p_{k,a}, k ascending
 *   state             1 iff p_1 > p_0 (an exact tie is absent); node_conf[k] = sum_g max(p_0, p_1), node_genes[k] = sum_g p_1 (the
 *                     expected accessory genome size of the ancestor)
 *   branch_gains[c]   sum_g sum_k post_k (U_0 (y pi_1)) L_1 / (y A + x D): the expected number of genes absent above
 *                     and present below the branch above node c; branch_losses[c]: (U_1 (y pi_0)) L_0 likewise; the root's 0
 *   gene_gains[g]     the same summed over the branches of gene g; gene_losses[g] likewise
 * A gene of likelihood 0 (an assigned class of rate 0 at a variable gene) makes lnl -inf, is absent at every node, adds nothing to
 * any sum and is counted in zero_genes.  Every gene's (mant, exp), posteriors, mean rate and states are the same bits on host and
 * device (pansim_amd/csrc/gene_rule.h); sums over genes are taken in a fixed order per device.  The tuning key "gene_team" of the
 * accessory handle forces the threads of a team (0 = choose, 64 or 256). */
#define PS_GENE_MAX_POP 2304u
#define PS_GENE_MAX_POP_MIX 1792u
typedef struct {
    double freq[2], root[2];
    uint32_t categories;
    double rate[8], weight[8];
    const uint8_t *gene_class;         /* NULL: mixture */
    uint64_t gene_classes;
} ps_gene_model;
typedef struct {
    uint32_t fit_rates, fit_freq, fit_weights;   /* 0 / 1 each; fit_weights acts on a mixture only */
    uint32_t max_rounds;               /* >= 1 */
    double eps_lnl;                    /* > 0: a round that gains less ends the fit */
} ps_gene_fit_params;
typedef struct {
    uint64_t pop_size, genes, merges;  /* N; G; N - 1 */
    uint64_t categories, classed;      /* K; 1 iff gene_class was given */
    uint64_t zero_genes, clamped_lengths;
    uint64_t rounds, passes, converged;   /* the fit: rounds run, up passes, 1 iff a round gained less than eps_lnl */
    double lnl, start_lnl;             /* start_lnl: the fit's lnL before the first round (else = lnl) */
    double beta, mean_rate;            /* 1 - pi_0^2 - pi_1^2; sum_k w_k r_k */
    double total_gains, total_losses;  /* sum branch_gains, sum branch_losses (the ancestral call) */
    double mean_conf, total_genes;     /* sum node_conf / (merges (genes - zero_genes)); sum node_genes */
} ps_gene_t;
/* One up pass on an accessory handle (the reference has no such function; population.rs:505).  gene_mant, gene_rate: genes f64,
 * gene_exp: genes i32, gene_post: genes x categories f64; each may be NULL and then costs nothing.  A core handle is
 * PS_ERR_INVALID.  Ordered behind the handle's queued work; changes no state.  PS_ERR_NO_DEVICE before anything else when no GPU
 * is visible; PS_ERR_OOM names the bytes. */
int ps_tree_gene_likelihood(ps_population *acc, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                            const ps_gene_model *model, ps_gene_t *out, double *gene_mant, int32_t *gene_exp, double *gene_post,
                            double *gene_rate);
/* The same on the accessory matrix of a simulation (the reference has no such function; population.rs:505) */
int ps_sim_tree_gene_likelihood(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                const ps_gene_model *model, ps_gene_t *out, double *gene_mant, int32_t *gene_exp, double *gene_post,
                                double *gene_rate);
/* The same for a sharded run (the reference has no such function; population.rs:505): shard 0's accessory replica answers */
int ps_multi_tree_gene_likelihood(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                  const ps_gene_model *model, ps_gene_t *out, double *gene_mant, int32_t *gene_exp, double *gene_post,
                                  double *gene_rate);
/* The up and the down pass (the reference has no such function; population.rs:505).  *anc: a NEW accessory handle of pop_size
 * = merges with the source's ncols and core_genes, made as ps_population_pool makes one (a stream of its own, no rates set), row k
 * = node pop_size + k, both of its views filled on the device; destroyed with ps_population_destroy in any order relative to its
 * source.  anc may be NULL: no matrix is allocated or stored.  node_conf, node_genes: merges f64; branch_gains, branch_losses:
 * pop_size + merges f64; gene_gains, gene_losses: genes f64; each may be NULL.  The source is read behind its queued work and never
 * written. */
int ps_tree_gene_ancestral(ps_population *acc, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                           const ps_gene_model *model, ps_gene_t *out, ps_population **anc, double *node_conf, double *node_genes,
                           double *branch_gains, double *branch_losses, double *gene_gains, double *gene_losses);
/* The same on the accessory matrix of a simulation (the reference has no such function; population.rs:505) */
int ps_sim_tree_gene_ancestral(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                               const ps_gene_model *model, ps_gene_t *out, ps_population **anc, double *node_conf, double *node_genes,
                               double *branch_gains, double *branch_losses, double *gene_gains, double *gene_losses);
/* The same for a sharded run (the reference has no such function; population.rs:505): shard 0's accessory replica answers */
int ps_multi_tree_gene_ancestral(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                                 const ps_gene_model *model, ps_gene_t *out, ps_population **anc, double *node_conf, double *node_genes,
                                 double *branch_gains, double *branch_losses, double *gene_gains, double *gene_losses);
/* The fit of the rates, pi_1 and (a mixture) the weights from `model` as the start; rho and the lengths are never fitted (the
 * reference has no such function; population.rs:505).  Derivative-free and deterministic.  Every 1-D search brackets the
 * optimum from the current value by steps that double, then narrows by golden section, and keeps the best point it has seen.  Per
 * round: the rates -- assigned classes: lnL = sum_k lnL_k and r_k touches lnL_k only, so the K searches on ln r_k advance in
 * lockstep, one up pass evaluating one trial rate of every class; a mixture: the r_k in turn on the whole lnL; a rate of 0 is
 * held -- then, a mixture, up to 8 EM updates w_k <- mean_g post_gk while each raises lnL, then pi_1 on logit pi_1.  lnL is formed
 * on the host from the genes' (mant, exp) in ascending order: the device fit and ps_gene_fit_from_rows take the same decisions
 * and return the same bits.  A round never ends below where it started; the fit ends when a round gains less than eps_lnl
 * (converged = 1) or after max_rounds.  rate_out, weight_out: categories f64; freq_out: 2 f64; round_lnl: round_cap values, [0] =
 * the start's lnL, [r] = after round r (as many as fit); each may be NULL. */
int ps_tree_gene_fit(ps_population *acc, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                     const ps_gene_model *model, const ps_gene_fit_params *prm, ps_gene_t *out, double *rate_out, double *weight_out,
                     double *freq_out, double *round_lnl, uint64_t round_cap);
/* The same on the accessory matrix of a simulation (the reference has no such function; population.rs:505) */
int ps_sim_tree_gene_fit(ps_sim *s, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                         const ps_gene_model *model, const ps_gene_fit_params *prm, ps_gene_t *out, double *rate_out, double *weight_out,
                         double *freq_out, double *round_lnl, uint64_t round_cap);
/* The same for a sharded run (the reference has no such function; population.rs:505): shard 0's accessory replica answers */
int ps_multi_tree_gene_fit(ps_multi *m, const uint32_t *left, const uint32_t *right, const double *length, uint64_t merges,
                           const ps_gene_model *model, const ps_gene_fit_params *prm, ps_gene_t *out, double *rate_out, double *weight_out,
                           double *freq_out, double *round_lnl, uint64_t round_cap);
/* device ms of the last of the three calls above on this accessory handle, summed over its passes (HIP events; the reference has
 * no such function; population.rs:505): the uploads, the kernel with its stores and the transpose, the sum of the workgroups'
 * rows.  PS_ERR_STATE before any call. */
int ps_tree_gene_timing(ps_population *acc, double *upload_ms, double *pass_ms, double *reduce_ms);
/* One up pass on the host (no device is touched; the reference has no such function; population.rs:505), through the same
 * gene_rule.h functions as the kernel, the genes summed in ascending order.  rows: individual-major pop_size x cols bytes. */
int ps_gene_likelihood_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                 const double *length, uint64_t merges, const ps_gene_model *model, ps_gene_t *out, double *gene_mant,
                                 int32_t *gene_exp, double *gene_post, double *gene_rate);
/* The up and the down pass on the host (no device is touched; the reference has no such function; population.rs:505).
 * anc_rows (may be NULL): individual-major merges x cols bytes 0 / 1, row k = node pop_size + k. */
int ps_gene_ancestral_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                                const double *length, uint64_t merges, const ps_gene_model *model, ps_gene_t *out, uint8_t *anc_rows,
                                double *node_conf, double *node_genes, double *branch_gains, double *branch_losses, double *gene_gains,
                                double *gene_losses);
/* The fit on the host (no device is touched; the reference has no such function; population.rs:505): the same loop over host
 * passes. */
int ps_gene_fit_from_rows(const uint8_t *rows, uint64_t pop_size, uint64_t cols, const uint32_t *left, const uint32_t *right,
                          const double *length, uint64_t merges, const ps_gene_model *model, const ps_gene_fit_params *prm, ps_gene_t *out,
                          double *rate_out, double *weight_out, double *freq_out, double *round_lnl, uint64_t round_cap);

#ifdef __cplusplus
}
#endif
#endif
