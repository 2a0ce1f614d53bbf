// pair_hist_kernels.h -- the binning kernel of ps_distance_histogram (docs/DISTANCE_HISTOGRAM.md) and the integer rules it
// shares with the host restatement (ps_histogram_from_counts).
//
// Input per band of rows [lo, lo + nrows): the u32 Hamming numerators h(i, j) against all N columns (core_davg_band_counts),
// the u16 accessory intersections of the same rows (acc_intersections_mfma_kernel) and the rows' gene counts
// (acc_rows_pad_kernel).  Only j > i is used; columns >= N and pad rows are never read as pairs.
//   core:       d = h / 2, bin_c = min(Bc - 1, floor(d Bc / S)); d >= S is counted in `clamped`
//   accessory:  U = |x| + |y| - I, a = U - I, b = U + cg, bin_a = min(Ba - 1, floor(a Ba / b)); b == 0 is `undefined`
// Both quotients are below 2^14 + 1, so an f32 estimate is off by at most one and two integer comparisons make it exact
// (ps_ph_div; the loops never run twice).  Every sum is an integer sum: the result does not depend on the launch geometry.
#pragma once

#include <stdint.h>

// the summary words (u64 each).  The square sum of a thread is kept in 96 bits (u64 + carry count); its three 32-bit
// words are added as three u64 sums and recombined on the host: sqsum = SQ0 + SQ1 2^32 + SQ2 2^64.
enum { PS_PH_UNDEF = 0, PS_PH_CLAMP, PS_PH_MIN, PS_PH_MAX, PS_PH_SUM, PS_PH_SQ0, PS_PH_SQ1, PS_PH_SQ2, PS_PH_WORDS };

struct ps_ph_args {
    uint32_t Bc, Ba;
    uint64_t S;          // core span (>= 1)
    uint64_t cg;         // core genes
    float c_scale;       // ~ Bc / S
    float cg_f;          // ~ cg
};

// floor(x / y) for y >= 1 and a quotient below 2^24, from an estimate `est` of it (any value: a wrong estimate only costs steps)
__host__ __device__ __forceinline__ uint32_t ps_ph_div(uint64_t x, uint64_t y, float est)
{
    uint32_t q = est > 0.0f ? (est < 16777216.0f ? (uint32_t)est : 16777216u) : 0u;
    // (q y <= x (1 + 2^-20) + y here whenever q >= 1: far from 2^64 for x below 2^46)
    while (q > 0u && (uint64_t)q * y > x) q--;
    while (x - (uint64_t)q * y >= y) q++;
    return q;
}

__host__ __device__ __forceinline__ uint32_t ps_ph_core_bin(uint32_t d, const ps_ph_args &a, bool *clamped)
{
    *clamped = (uint64_t)d >= a.S;
    if (*clamped) return a.Bc - 1u;
    const uint32_t q = ps_ph_div((uint64_t)d * a.Bc, a.S, (float)d * a.c_scale);
    return q < a.Bc - 1u ? q : a.Bc - 1u;
}

// in <= un <= 2^17: a Ba < 2^31
__host__ __device__ __forceinline__ uint32_t ps_ph_acc_bin(uint32_t in, uint32_t un, const ps_ph_args &a, bool *undefined)
{
    const uint64_t b = (uint64_t)un + a.cg;
    *undefined = b == 0ull;
    if (*undefined) return 0u;
    const uint64_t x = (uint64_t)(un - in) * a.Ba;
#if defined(__HIP_DEVICE_COMPILE__)
    const float est = (float)(uint32_t)x * __builtin_amdgcn_rcpf((float)un + a.cg_f);     // (one ulp: an estimate is all it is)
#else
    const float est = (float)(uint32_t)x / ((float)un + a.cg_f);
#endif
    const uint32_t q = ps_ph_div(x, b, est);
    return q < a.Ba - 1u ? q : a.Ba - 1u;
}

__device__ __forceinline__ unsigned long long ps_ph_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
    return v;
}

// BIN: fill the joint bins (and count the undefined and the clamped pairs); MOM: the core moments.  The automatic span runs
// <false, true> first and <true, false> with S = max + 1 after it.
// Grid: x = workgroups of four waves striding over the 256-column chunks of a row, y strides over the band's rows; any grid
// is valid.  Dynamic LDS: Bc Ba u32 bins when BIN.  In == nullptr: no accessory genes (I = U = 0 for every pair).
template <bool BIN, bool MOM>
__global__ void __launch_bounds__(256) pair_hist_kernel(const uint32_t *C, uint64_t ldc, const uint16_t *In, uint32_t ldi,
                                                        const uint32_t *rowcnt, uint32_t N, uint32_t lo, uint32_t nrows,
                                                        ps_ph_args a, unsigned long long *joint, unsigned long long *words)
{
    extern __shared__ uint32_t ph_bins[];
    __shared__ unsigned long long ph_acc[PS_PH_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t nbins = BIN ? a.Bc * a.Ba : 0u;
    for (uint32_t b = tid; b < nbins; b += 256u) ph_bins[b] = 0u;
    if (tid < (uint32_t)PS_PH_WORDS) ph_acc[tid] = tid == (uint32_t)PS_PH_MIN ? ~0ull : 0ull;
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (tid >> 6)));
    const uint32_t nwaves = gridDim.x * 4u, nchunk = (N + 255u) >> 8;
    uint32_t n_undef = 0, n_clamp = 0, d_min = ~0u, d_max = 0u, sq_carry = 0u;
    uint64_t d_sum = 0, sq_lo = 0;
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t i = lo + r;
        if (i + 1u >= N) break;                 // (rows ascend: nothing right of the diagonal from here on)
        const uint32_t ci = (BIN && In) ? rowcnt[i] : 0u;
        // chunks left of the one that holds column i + 1 lie wholly at or below the diagonal
        for (uint32_t c = ((i + 1u) >> 8) + wave; c < nchunk; c += nwaves) {
            const uint32_t j0 = (c << 8) + lane * 4u;
            if (j0 >= N || j0 + 3u <= i) continue;
            // (ldc >= N rounded up to 64, ldi >= N rounded up to 128, rowcnt has as many entries: four columns from a
            // multiple of four below N stay inside the row)
            const uint4 h4 = *(const uint4 *)(C + (size_t)r * ldc + j0);
            const uint32_t hv[4] = { h4.x, h4.y, h4.z, h4.w };
            uint32_t iv[4] = { 0u, 0u, 0u, 0u }, cj[4] = { 0u, 0u, 0u, 0u };
            if (BIN && In) {
                const uint2 i2 = *(const uint2 *)(In + (size_t)r * ldi + j0);
                const uint4 c4 = *(const uint4 *)(rowcnt + j0);
                iv[0] = i2.x & 0xffffu; iv[1] = i2.x >> 16; iv[2] = i2.y & 0xffffu; iv[3] = i2.y >> 16;
                cj[0] = c4.x; cj[1] = c4.y; cj[2] = c4.z; cj[3] = c4.w;
            }
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                const uint32_t j = j0 + q;
                if (j <= i || j >= N) continue;
                const uint32_t d = hv[q] >> 1;
                if (MOM) {
                    d_min = min(d_min, d);
                    d_max = max(d_max, d);
                    d_sum += d;
                    const uint64_t sq = (uint64_t)d * d;
                    sq_lo += sq;
                    sq_carry += sq_lo < sq ? 1u : 0u;
                }
                if (BIN) {
                    bool clamped, undefined;
                    const uint32_t bc = ps_ph_core_bin(d, a, &clamped);
                    const uint32_t ba = ps_ph_acc_bin(iv[q], ci + cj[q] - iv[q], a, &undefined);
                    n_clamp += clamped ? 1u : 0u;
                    n_undef += undefined ? 1u : 0u;
                    if (!undefined) atomicAdd(&ph_bins[bc * a.Ba + ba], 1u);
                }
            }
        }
    }
    // per wave, then per workgroup, then one global atomic per word
    if (BIN) {
        const unsigned long long u = ps_ph_wave_sum(n_undef), k = ps_ph_wave_sum(n_clamp);
        if (lane == 0u) {
            if (u) atomicAdd(&ph_acc[PS_PH_UNDEF], u);
            if (k) atomicAdd(&ph_acc[PS_PH_CLAMP], k);
        }
    }
    if (MOM) {
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            d_min = min(d_min, (uint32_t)__shfl_xor((int)d_min, o, 64));
            d_max = max(d_max, (uint32_t)__shfl_xor((int)d_max, o, 64));
        }
        const unsigned long long s = ps_ph_wave_sum(d_sum), s0 = ps_ph_wave_sum(sq_lo & 0xffffffffull),
                                 s1 = ps_ph_wave_sum(sq_lo >> 32), s2 = ps_ph_wave_sum(sq_carry);
        if (lane == 0u) {
            atomicMin(&ph_acc[PS_PH_MIN], (unsigned long long)d_min | (d_min == ~0u ? ~0ull : 0ull));
            atomicMax(&ph_acc[PS_PH_MAX], (unsigned long long)d_max);
            atomicAdd(&ph_acc[PS_PH_SUM], s);
            atomicAdd(&ph_acc[PS_PH_SQ0], s0);
            atomicAdd(&ph_acc[PS_PH_SQ1], s1);
            atomicAdd(&ph_acc[PS_PH_SQ2], s2);
        }
    }
    __syncthreads();
    if (tid < (uint32_t)PS_PH_WORDS) {
        const unsigned long long v = ph_acc[tid];
        if (tid == (uint32_t)PS_PH_MIN) { if (MOM && v != ~0ull) atomicMin(&words[tid], v); }
        else if (tid == (uint32_t)PS_PH_MAX) { if (MOM && v) atomicMax(&words[tid], v); }
        else if (v) atomicAdd(&words[tid], v);
    }
    for (uint32_t b = tid; b < nbins; b += 256u) {
        const uint32_t v = ph_bins[b];
        if (v) atomicAdd(&joint[b], (unsigned long long)v);
    }
}

