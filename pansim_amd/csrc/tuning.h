// tuning.h -- every switch of the library, written down once: the table of the per-handle tuning keys (ps_set_tuning,
// ps_get_tuning, ps_tuning_key and the PANSIM_* variables that pop_create_impl reads into a new handle) and the one reader of
// the environment for everything else.  The defaults are the initialisers of struct ps_population.  Included by
// pansim_capi.hip behind that struct; the list of every PANSIM_* name the library reads closes the file.
#pragma once

// ---------------------------------------------------------------------------
// the environment: getenv is called here and nowhere else
// ---------------------------------------------------------------------------
static const char *env_str(const char *name) { return getenv(name); }
// the variable is present, whatever it holds
static bool env_given(const char *name) { return env_str(name) != nullptr; }
static long long env_int(const char *name, long long fallback)
{
    const char *e = env_str(name);
    return e ? atoll(e) : fallback;
}
// present: its number is non-zero; absent: `fallback` (true for a switch that only "=0" turns off)
static bool env_flag(const char *name, bool fallback)
{
    const char *e = env_str(name);
    return e ? atoi(e) != 0 : fallback;
}

// ---------------------------------------------------------------------------
// the per-handle switches
// ---------------------------------------------------------------------------
enum tune_check { TUNE_RANGE, TUNE_SET, TUNE_BOOL };    // v[0] <= value <= v[1] | value is one of v[0..3] | value != 0
// what a new handle does with an environment value that fails the check (a key always refuses it)
enum tune_env { ENV_IGNORE, ENV_CLAMP, ENV_TAKE };      // keep the default | the nearest end of the range | store it as it is
enum tune_scope { ANY_HANDLE, CORE_ONLY, ACC_ONLY };    // the handles whose creation reads the environment name

// the field of a switch: a pointer to a uint32_t, int or bool member, or none (accepted and ignored)
struct tune_field {
    uint32_t ps_population::*u = nullptr;
    int ps_population::*i = nullptr;
    bool ps_population::*b = nullptr;
    constexpr tune_field() {}
    constexpr tune_field(uint32_t ps_population::*m) : u(m) {}
    constexpr tune_field(int ps_population::*m) : i(m) {}
    constexpr tune_field(bool ps_population::*m) : b(m) {}
};

struct tuning_row {
    const char *key;
    const char *env;                    // nullptr: none
    tune_field field;
    tune_check check;
    int64_t v[4];                       // (a set of fewer than four repeats its last member)
    const char *error;                  // what ps_set_tuning says to a refused value
    tune_env env_bad;
    tune_scope env_scope;               // (a key is taken by every handle)
    bool env_only;                      // the environment alone sets it: ps_set_tuning does not know the key
    void (*after)(ps_population *);     // runs behind a stored value, or nullptr
};                                      // (a row ends where the rest is 0: ENV_IGNORE, ANY_HANDLE, false, nullptr)

// the cached pair list is sorted / has a thread table depending on the LDS tile
static void tune_drop_pair_cache(ps_population *p) { p->pairs_cached = 0; }

#define PS_POP(f) &ps_population::f
// The environment values that are not held to their key's check, kept as they were found:
//   PANSIM_HGT_MODE, PANSIM_BLOCK_BATCH, PANSIM_BLOCK_WAVES, PANSIM_HGT_SLICES are stored as given (a negative one wraps to u32);
//   PANSIM_SWEEP_OOP, PANSIM_WINDOW_SWEEP, PANSIM_WINDOW_BPC are clamped where their keys refuse;
//   PANSIM_ACC_LDS_LIMIT is read by accessory handles only ("lds_limit" is taken by both);
//   the others (ENV_IGNORE) hold the check, but a value that fails it is dropped without a word where the key reports an error.
static const tuning_row g_tuning[] = {
    { "sweep_blocks_per_cu", "PANSIM_SWEEP_BLOCKS_PER_CU", PS_POP(sweep_blocks_per_cu), TUNE_RANGE, { 1, 8 }, "sweep_blocks_per_cu must be 1..8" },
    // (accepted and ignored since round 6: a wave takes the 4 sites of a level-1 block group per iteration)
    { "sweep_rows", "PANSIM_SWEEP_ROWS", {}, TUNE_RANGE, { 2, 4 }, "sweep_rows must be 2..4" },
    { "sweep_out_of_place", "PANSIM_SWEEP_OOP", PS_POP(sweep_oop), TUNE_RANGE, { -1, 2 }, "sweep_out_of_place must be -1 (choose), 0 (in place), 1 (out of place) or 2 (out of place, nontemporal loads and stores)", ENV_CLAMP },
    { "hgt_apply_threads", "PANSIM_HGT_APPLY_THREADS", PS_POP(hgt_apply_threads), TUNE_SET, { 256, 512, 1024, 1024 }, "hgt_apply_threads must be 256, 512 or 1024" },
    { "window_blocks_per_cu", "PANSIM_WINDOW_BPC", PS_POP(window_blocks_per_cu), TUNE_RANGE, { 0, 8 }, "window_blocks_per_cu must be 0 (choose) or 1..8", ENV_CLAMP },
    { "davg_form", nullptr, PS_POP(davg_form), TUNE_RANGE, { 0, 3 }, "davg_form must be 0 (choose), 1 (LDS-tile popcount kernels), 2 (matrix cores, one kernel) or 3 (matrix cores, two phases)" },
    { "core_davg_form", nullptr, PS_POP(core_davg_form), TUNE_RANGE, { 0, 3 }, "core_davg_form must be 0 (choose), 1 (whole matrix), 2 (banded) or 3 (generic)" },
    { "ld_band", nullptr, PS_POP(ld_band), TUNE_RANGE, { 0, 65536 }, "ld_band must be 0 (choose)..65536 rows of loci" },
    { "mlst_band", nullptr, PS_POP(mlst_band), TUNE_RANGE, { 0, 65535 }, "mlst_band must be 0 (choose)..65535 loci" },
    { "gene_team", nullptr, PS_POP(gene_team), TUNE_SET, { 0, 64, 256, 256 }, "gene_team must be 0 (choose), 64 or 256 threads" },
    { "gather_form", nullptr, PS_POP(gather_form), TUNE_RANGE, { 0, 2 }, "gather_form must be 0 (choose), 1 (source rows staged in LDS) or 2 (bytes loaded from global memory)" },
    { "core_davg_band", nullptr, PS_POP(core_davg_band), TUNE_RANGE, { 0, 1ll << 31 }, "core_davg_band must be 0 (choose)..2^31 rows" },
    { "davg_plain_division", nullptr, PS_POP(davg_plain_division), TUNE_BOOL },
    { "davg_ib", nullptr, PS_POP(davg_ib), TUNE_SET, { 0, 16, 32, 32 }, "davg_ib must be 0 (choose), 16 or 32" },
    { "davg_nb", nullptr, PS_POP(davg_nb), TUNE_SET, { 0, 1, 2, 4 }, "davg_nb must be 0 (choose), 1, 2 or (two-phase form only) 4" },
    { "hgt_mode", "PANSIM_HGT_MODE", PS_POP(hgt_mode), TUNE_RANGE, { 0, 2 }, "hgt_mode must be 0 (auto), 1 (one atomic per event) or 2 (binned by recipient partition, two passes)", ENV_TAKE },
    { "pair_mode", nullptr, PS_POP(pair_mode), TUNE_RANGE, { 0, 7 }, "pair_mode must be 0 (auto), 1 (sampled), 2 (all pairs), 3 (sampled, nibble form even for one-hot matrices), 4 (transposed bit strings, streamed per pair), 5 (all pairs, xor + popcount tiles even for one-hot matrices), 6 (all pairs, i8 matrix cores when the matrix is one-hot; mode 2 takes the FP4 form) or 7 (the FP4 form on three +-1 features per site)" },
    { "pair_ranges", nullptr, PS_POP(pair_ranges), TUNE_RANGE, { 0, 65535 }, "pair_ranges must be 0 (choose)..65535" },
    { "force_block_sweep", nullptr, PS_POP(force_block_sweep), TUNE_BOOL },
    { "force_inline_sweep", nullptr, PS_POP(force_inline_sweep), TUNE_BOOL },
    { "hgt_slices", "PANSIM_HGT_SLICES", PS_POP(hgt_slices), TUNE_RANGE, { 0, 4096 }, "hgt_slices must be 0..4096", ENV_TAKE },
    { "block_batch", "PANSIM_BLOCK_BATCH", PS_POP(block_batch), TUNE_SET, { 0, 2, 4, 4 }, "block_batch must be 0 (choose), 2 or 4", ENV_TAKE },
    { "hgt_bin_cap", nullptr, PS_POP(hgt_bin_cap), TUNE_RANGE, { 0, 1 << 30 }, "hgt_bin_cap must be 0 (sized by the rates)..2^30" },
    { "hgt_events_per_thread", nullptr, PS_POP(hgt_events_per_thread), TUNE_RANGE, { 0, 100000 }, "hgt_events_per_thread must be 0 (whole chip)..100000" },
    { "window_sweep", "PANSIM_WINDOW_SWEEP", PS_POP(window_sweep), TUNE_RANGE, { -1, 1 }, "window_sweep must be -1 (choose), 0 (block sweep) or 1 (window sweep where the parents are sorted)", ENV_CLAMP },
    { "sweep_generations", "PANSIM_SWEEP_GENERATIONS", PS_POP(sweep_generations), TUNE_RANGE, { 0, PS_SWEEP_MAX_GENS }, "sweep_generations must be 0 (choose), 1 or 2" },
    { "sweep_queue_cap", nullptr, PS_POP(sweep_queue_cap), TUNE_RANGE, { 0, 65536 }, "sweep_queue_cap must be 0 (real size)..65536" },
    { "hgt_list_in_global", nullptr, PS_POP(hgt_list_in_global), TUNE_BOOL },
    { "hgt_bin_list_in_global", "PANSIM_HGT_BIN_LIST_GLOBAL", PS_POP(hgt_bin_list_in_global), TUNE_BOOL },
    { "no_block_preload", nullptr, PS_POP(no_block_preload), TUNE_BOOL },
    { "block_waves", "PANSIM_BLOCK_WAVES", PS_POP(block_waves), TUNE_SET, { 0, 4, 8, 16 }, "block_waves must be 0 (auto), 4, 8 or 16", ENV_TAKE },
    { "lds_limit", "PANSIM_ACC_LDS_LIMIT", PS_POP(lds_limit), TUNE_RANGE, { 1024, 160 * 1024 }, "lds_limit must be 1 KiB..160 KiB", ENV_IGNORE, ACC_ONLY, false, tune_drop_pair_cache },
    // the two that only the environment sets, at creation (ps_get_tuning reads them)
    { "free_cus_per_xcd", "PANSIM_SWEEP_FREE_CUS", PS_POP(free_cus_per_xcd), TUNE_RANGE, { 0, 8 }, nullptr, ENV_CLAMP, CORE_ONLY, true },
    { "hgt_bin_prio", "PANSIM_HGT_BIN_PRIO", PS_POP(hgt_bin_prio), TUNE_RANGE, { 0, 3 }, nullptr, ENV_CLAMP, ANY_HANDLE, true },
};
#undef PS_POP

static const tuning_row *tuning_find(const char *key)
{
    for (const tuning_row &r : g_tuning)
        if (strcmp(r.key, key) == 0) return &r;
    return nullptr;
}

// One value into one switch.  refuse: a value that fails the row's check is an error (a key); otherwise the row's tune_env
// decides (the environment at creation).
static int tuning_apply(ps_population *p, const tuning_row &r, int64_t value, bool refuse)
{
    bool ok = true;
    if (r.check == TUNE_RANGE) ok = value >= r.v[0] && value <= r.v[1];
    if (r.check == TUNE_SET) ok = value == r.v[0] || value == r.v[1] || value == r.v[2] || value == r.v[3];
    if (!ok) {
        if (refuse) return ps_fail(PS_ERR_INVALID, "%s", r.error);
        if (r.env_bad == ENV_IGNORE) return PS_OK;
        if (r.env_bad == ENV_CLAMP) value = std::max(r.v[0], std::min(r.v[1], value));
    }
    if (r.field.u) p->*r.field.u = (uint32_t)value;
    if (r.field.i) p->*r.field.i = (int)value;
    if (r.field.b) p->*r.field.b = value != 0;
    if (r.after) r.after(p);
    return PS_OK;
}

// a new handle: every row whose environment name is present and meant for this kind of handle
static void tuning_from_env(ps_population *p)
{
    for (const tuning_row &r : g_tuning) {
        if (!r.env || (r.env_scope == CORE_ONLY && !p->cfg.core) || (r.env_scope == ACC_ONLY && p->cfg.core)) continue;
        if (const char *e = env_str(r.env)) (void)tuning_apply(p, r, atoi(e), false);
    }
}

extern "C" const char *ps_tuning_key(uint32_t index)
{
    return index < sizeof g_tuning / sizeof g_tuning[0] ? g_tuning[index].key : nullptr;
}

extern "C" int ps_set_tuning(ps_population *p, const char *key, int64_t value)
{
    if (!p || !key) return ps_fail(PS_ERR_INVALID, "null argument");
    const tuning_row *r = tuning_find(key);
    if (!r || r->env_only) return ps_fail(PS_ERR_INVALID, "unknown tuning key %s", key);
    return tuning_apply(p, *r, value, true);
}

extern "C" int ps_get_tuning(ps_population *p, const char *key, int64_t *value)
{
    if (!p || !key || !value) return ps_fail(PS_ERR_INVALID, "null argument");
    const tuning_row *r = tuning_find(key);
    if (!r) return ps_fail(PS_ERR_INVALID, "unknown tuning key %s", key);
    const tune_field &f = r->field;
    // (an accepted-and-ignored key reads as what the library does whatever was set: the upper end of its range)
    *value = f.u ? (int64_t)(p->*f.u) : f.i ? (int64_t)(p->*f.i) : f.b ? (int64_t)(p->*f.b) : r->v[1];
    return PS_OK;
}

// ---------------------------------------------------------------------------
// Every PANSIM_* name the library reads.  (PANSIM_BENCH_* belong to bench.py.)
// ---------------------------------------------------------------------------
// Into a new handle, through the table above (key in quotes):
//   PANSIM_SWEEP_BLOCKS_PER_CU   "sweep_blocks_per_cu"; present at all, it also keeps ps_sim_create from choosing the value
//   PANSIM_SWEEP_ROWS            "sweep_rows" (accepted and ignored)
//   PANSIM_SWEEP_OOP             "sweep_out_of_place"
//   PANSIM_SWEEP_GENERATIONS     "sweep_generations"
//   PANSIM_WINDOW_SWEEP          "window_sweep"
//   PANSIM_WINDOW_BPC            "window_blocks_per_cu"; present at all, it also keeps a donor-sharded ps_sim from choosing 5
//   PANSIM_BLOCK_BATCH           "block_batch"
//   PANSIM_BLOCK_WAVES           "block_waves"
//   PANSIM_HGT_MODE              "hgt_mode"
//   PANSIM_HGT_SLICES            "hgt_slices"
//   PANSIM_HGT_APPLY_THREADS     "hgt_apply_threads"
//   PANSIM_HGT_BIN_LIST_GLOBAL   "hgt_bin_list_in_global"
//   PANSIM_HGT_BIN_PRIO          s_setprio level of the binned HGT's bin pass beside the sweep, 0..3
//   PANSIM_ACC_LDS_LIMIT         "lds_limit", accessory handles
//   PANSIM_SWEEP_FREE_CUS        core handles: CUs per XCD that the CU mask of the core stream leaves to the other streams, 0..8
// At every ps_sim_create / ps_sim_set_exchange / ps_multi_create:
//   PANSIM_HGT_EVENTS_PER_THREAD events per thread of the light HGT kernel instead of the estimate from the sweep time
//   PANSIM_HEAVY_HGT             0/1: sweep and binned HGT take turns, instead of the choice by expected events
//   PANSIM_DEVICE_DRAW           0/1: the parents are drawn on the device, instead of the choice by pop_size
//   PANSIM_FUSE_COUNTS           =0: gene counts by their own kernel, not by the reduce pass of the binned HGT (A/B runs)
//   PANSIM_EXCHANGE_BESIDE_SWEEP =1 (experiment): the next sweep of a donor-sharded run waits for the LDS-image pass only
//   PANSIM_MULTI_REPLICATED_HGT  present: every shard of a ps_multi generates every event, no exchange
//   PANSIM_MULTI_EXCHANGE        =or: the shards' deltas are ORed whole, not in slices
//   PANSIM_MULTI_OWN_WEIGHTS     present: every shard of a ps_multi computes the selection weights itself
// At every use:
//   PANSIM_HGT_DONOR_BLOCKS      donor workgroups of the binned HGT's bin pass (1024)
//   PANSIM_HOST_THREADS          host threads of the softmaxes' libm calls, instead of the hardware's count (at most 16)
//   PANSIM_STATE_CHUNK_ROWS      site rows per chunk of a state file's core section, instead of 64 MiB of file bytes
//   PANSIM_RCCL_GATHER           =ring: ncclAllGather instead of the direct sends (at every ps_rccl_exchange_create)
//   PANSIM_PRINT_STAMPS          present: a destroyed handle prints its diagnostic phase stamps
// Once per process, at the first use:
//   PANSIM_GAP_ON_CORE_STREAM    =1: the bin pass of a heavy HGT is recorded for the core stream (measured, not the default)
//   PANSIM_DAVG_AHEAD            =0: the D-avg of the next generation is not run ahead of the sweep
//   PANSIM_EMU_RING              =1: the emulated exchange prices a ring all-gather
//   PANSIM_RCCL_LIBRARY          the library to open instead of librccl.so (a path: read as a string)
// Once per emulating ps_sim, at its first exchange:
//   PANSIM_EMU_XGMI_GBPS, PANSIM_EMU_COLL_LATENCY_US   link rate and collective latency of bench.py --emulate-shard
