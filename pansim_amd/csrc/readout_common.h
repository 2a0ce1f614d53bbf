// readout_common.h -- what the device read-outs (core_diversity.h .. locus_ld.h) share on the host: the device check of every
// entry, the layout and the growth of the scratch a handle keeps per read-out (ps_population::ro), the event timer behind the
// ps_*_timing entries and the grid of the binning kernels.  Included by pansim_capi.hip behind dev_grow_err; scratch_layout alone needs nothing but <cstdint> (PS_READOUT_LAYOUT_ONLY: a host program that checks layouts).
#pragma once

#include <cstdint>

// The regions of one scratch buffer, in order: add() rounds the region's bytes up to `align` (a power of two) and returns its
// offset from the base; `bytes` is the buffer's size so far.
struct scratch_layout {
    uint64_t bytes = 0;
    uint64_t add(uint64_t n, uint64_t align)
    {
        const uint64_t off = bytes;
        bytes += (n + align - 1) & ~(align - 1);
        return off;
    }
};

#ifndef PS_READOUT_LAYOUT_ONLY

// behind every entry that computes: `count` (if asked for) = the devices visible
static int ps_needs_device(int *count = nullptr)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return ps_fail(PS_ERR_NO_DEVICE, "no HIP device is visible: libpansim_hip has no CPU path");
    if (count) *count = ndev;
    return PS_OK;
}

// The slot grown to `bytes` -> its base.  `oom`: the read-out's own out-of-memory message, a printf format whose first argument is
// the bytes (%llu), the others follow (nullptr: the HIP error as HIPCHK words it)
template <class... A>
static int scratch_get(readout_slot &ro, uint64_t bytes, uint8_t **base, const char *oom, A... args)
{
    const hipError_t e = dev_grow_err(ro.d, ro.cap, bytes);
    if (e != hipSuccess && !ro.d && oom) {
        (void)hipGetLastError();
        return ps_fail(PS_ERR_OOM, oom, (unsigned long long)bytes, args...);
    }
    HIPCHK(e);
    *base = (uint8_t *)ro.d;
    return PS_OK;
}

// HIP events around pieces of work in up to five groups, all on one device; the totals once the streams have been synchronised
struct event_timer {
    std::vector<hipEvent_t> pool;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> timers[5];
    ~event_timer() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
    int make(hipEvent_t *out)
    {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        pool.push_back(e);
        *out = e;
        return PS_OK;
    }
    template <class W>
    int timed(int group, hipStream_t st, W &&work)
    {
        hipEvent_t e0, e1;
        PSCHK(make(&e0));
        PSCHK(make(&e1));
        HIPCHK(hipEventRecord(e0, st));
        PSCHK(work());
        HIPCHK(hipEventRecord(e1, st));
        timers[group].push_back({ e0, e1 });
        return PS_OK;
    }
    int total_ms(int group, double *out)
    {
        *out = 0.0;
        for (const auto &e : timers[group]) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, e.first, e.second));
            *out += (double)ms;
        }
        return PS_OK;
    }
    // the first `groups` totals into the slot, which then counts as computed (the callers clear `timed` before their first launch)
    int collect(readout_slot &ro, int groups)
    {
        for (int g = 0; g < groups; g++) PSCHK(total_ms(g, &ro.ms[g]));
        ro.timed = true;
        return PS_OK;
    }
};

// behind a ps_*_timing entry: the slot's times through the optional pointers, `none` while nothing has been computed
static int readout_timing(const readout_slot &ro, const char *none, std::initializer_list<double *> out)
{
    if (!ro.timed) return ps_fail(PS_ERR_STATE, "%s", none);
    int g = 0;
    for (double *o : out) {
        if (o) *o = ro.ms[g];
        g++;
    }
    return PS_OK;
}

// four waves per workgroup over the 256-column chunks of a row: the x extent of the grids of the kernels that walk all pairs
static uint32_t pair_grid_x(uint32_t N)
{
    const uint32_t nchunk = (N + 255u) / 256u;
    return std::max(1u, std::min((nchunk + 3u) / 4u, 8u));
}

// The grid of a binning kernel over `nrows` rows of `cols` columns: the rows over y, as many workgroups as `lds` bytes of bins
// (and `pad` more per workgroup) let a CU hold; above 32 KB the kernel is allowed its dynamic LDS
static int bin_grid(const void *kern, uint32_t cols, uint32_t nrows, uint32_t lds, uint32_t pad, dim3 *grid)
{
    const uint32_t gx = pair_grid_x(cols), per_cu = std::max(1u, std::min(8u, (160u * 1024u) / (lds + pad)));
    if (lds > 32768u) HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    *grid = dim3(gx, std::max(1u, std::min(std::min(nrows, 65535u), 256u * per_cu / gx)));
    return PS_OK;
}

#endif
