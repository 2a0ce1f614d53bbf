// ld_kernels.h -- gfx950 kernels of the linkage disequilibrium between loci (ps_locus_ld, include/pansim_hip.h; the
// definitions: docs/LINKAGE_DISEQUILIBRIUM.md) and the integer rule of one pair that they share with the host restatement
// (ps_ld_from_counts).
//
// A locus is a column of a matrix; its indicator over the N individuals becomes one padded blocked bit row (the layout of
// acc_rows_pad_kernel: WP dwords, a multiple of 8, rows in the order of ps_da_row_offset), so that n11 of all pairs of loci is
// the {0, 1} contraction acc_intersections_mfma_kernel already computes for D-avg with rows = individuals: here rows = loci and
// K runs over the individuals.  The bit order along K only has to be the same in every row.
//   ld_candidate_kernel   ones of every column from its counts, flag = min(c, N - c) >= min_minor
//   ld_select_kernel      the chosen list from the inclusive prefix sums of the flags (idx_* scan pieces, acc_kernels.h)
//   ld_pack_core_kernel   one wave per selected site: the four base counts (bytes equal to 1 / 2 / 4 / 8: any other byte is in
//                         no class), the major base, then 16 cells -> 16 bits per lane and 1 KiB piece
//   ld_pack_acc_kernel    the same from a row of the gene-major bit view
//   ld_pair_kernel        per band of loci: n11 (u16) + two counts + two columns -> ps_ld_pair -> LDS bins
// A monomorphic locus keeps an all-zero row: its pairs are undefined from c alone, and every n11 the contraction meets is at most
// N - 1 <= 65535 -- which is what lets u16 counts serve N = 65536.  Every sum is an integer sum.
#pragma once

#include "diversity_kernels.h"
#include "pair_hist_kernels.h"

// the summary words the pair kernel accumulates (u64 each); the defined pairs and sum_q follow from the bins and the lag sums
enum { PS_LD_UNDEF = 0, PS_LD_FOURG, PS_LD_COMPLETE, PS_LD_POS, PS_LD_NEG, PS_LD_WORDS = 8 };
#define PS_LD_MAX_LAGS 32u

struct ps_ld_pair_t {
    uint32_t q, r2_bin, lag_bin;
    int32_t sign;                // of D
    uint32_t four, complete;     // 0 / 1
};

PS_HD uint64_t ps_ld_mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// One pair of POLYMORPHIC loci (0 < ca, cb < N <= 65536; n11 what the two counts allow), columns sa < sb.
//   D = N n11 - ca cb (|D| < 2^32), den = ca (N - ca) cb (N - cb) <= 2^60, D^2 <= den (r^2 <= 1)
//   q = floor(2^16 D^2 / den): the 76-bit product is (D^2 >> 48, D^2 << 16); an f64 estimate of the quotient (relative error
//   2^-51 on a value of at most 2^16: off by at most one) is corrected by exact 128-bit comparisons of q den against it.
PS_HD void ps_ld_pair(uint32_t N, uint32_t ca, uint32_t cb, uint32_t n11, uint32_t sa, uint32_t sb, uint32_t r2_bins, uint32_t lag_bins,
                      ps_ld_pair_t *o)
{
    const int64_t D = (int64_t)((uint64_t)N * n11) - (int64_t)((uint64_t)ca * cb);
    const uint64_t aD = (uint64_t)(D < 0 ? -D : D);
    const uint64_t den = ((uint64_t)ca * (N - ca)) * ((uint64_t)cb * (N - cb));
    const uint64_t d2 = aD * aD;
    const uint64_t xh = d2 >> 48, xl = d2 << 16;
    uint32_t q = (uint32_t)((double)d2 * 65536.0 / (double)den);
    auto fits = [&](uint32_t k) {            // k den <= 2^16 D^2
        const uint64_t hi = ps_ld_mulhi64((uint64_t)k, den), lo = (uint64_t)k * den;
        return hi < xh || (hi == xh && lo <= xl);
    };
    while (q > 0u && !fits(q)) q--;
    while (q < 65536u && fits(q + 1u)) q++;
    o->q = q;
    const uint32_t rb = (q * r2_bins) >> 16;
    o->r2_bin = rb < r2_bins - 1u ? rb : r2_bins - 1u;
    const uint32_t lg = 31u - (uint32_t)__builtin_clz(sb - sa);
    o->lag_bin = lg < lag_bins - 1u ? lg : lag_bins - 1u;
    o->sign = D > 0 ? 1 : D < 0 ? -1 : 0;
    o->complete = q == 65536u ? 1u : 0u;
    o->four = (n11 > 0u && ca > n11 && cb > n11 && (uint64_t)N + n11 > (uint64_t)ca + cb) ? 1u : 0u;
}

PS_HD bool ps_ld_monomorphic(uint32_t c, uint32_t N) { return c == 0u || c == N; }

// The ones of a column from its counts (the major base: the largest of the four, ties to the lowest byte -- its count is the
// maximum either way) and whether it is a candidate, as the 0 / 1 the scan runs over.
__global__ void __launch_bounds__(256) ld_candidate_kernel(const uint32_t *colcnt, uint32_t core, uint32_t ncols, uint32_t N,
                                                           uint32_t min_minor, uint32_t *flag)
{
    const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncols) return;
    uint32_t c;
    if (core) {
        const uint4 n = *(const uint4 *)(colcnt + (size_t)col * 4u);
        c = max(max(n.x, n.y), max(n.z, n.w));
    } else {
        c = colcnt[col];
    }
    flag[col] = min(c, N - c) >= min_minor ? 1u : 0u;
}

// Entry j of the list, j_lo <= j < j_lo + j_cnt: the candidate of rank j (C <= max_loci) or floor(j C / max_loci), C the
// candidates of ALL shards; this handle holds the ranks [rank_lo, rank_lo + incl[ncols - 1]).  sel[j - j_lo] = its local column.
__global__ void __launch_bounds__(256) ld_select_kernel(const uint32_t *incl, uint32_t ncols, uint64_t C, uint64_t rank_lo, uint32_t j_lo,
                                                        uint32_t j_cnt, uint32_t max_loci, uint32_t *sel)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= j_cnt) return;
    const uint64_t j = (uint64_t)j_lo + t;
    const uint64_t rank = (C <= (uint64_t)max_loci ? j : j * C / max_loci) - rank_lo;
    // the first column whose inclusive prefix exceeds the rank (as idx_fill_kernel)
    uint32_t lo = 0, hi = ncols - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)incl[mid] <= rank) lo = mid + 1u; else hi = mid;
    }
    sel[t] = lo;
}

// the bytes of w equal to the byte replicated in v4: bit 7 of each such byte
__device__ __forceinline__ uint32_t ps_ld_eq_bytes(uint32_t w, uint32_t v4)
{
    const uint32_t t = w ^ v4;
    return ~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) & 0x80808080u;
}

// bits 7 / 15 / 23 / 31 -> bits 0 .. 3 (the partial products land on distinct bits, all below 28 or past 31)
__device__ __forceinline__ uint32_t ps_ld_gather4(uint32_t z) { return ((z >> 7) * 0x10204080u) >> 28; }

__device__ __forceinline__ uint32_t ps_ld_wave_sum32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

// dword w of blocked row `row` (rows of WP dwords)
__device__ __forceinline__ size_t ps_ld_dword_offset(uint32_t row, uint32_t w, uint32_t WP)
{
    return ps_da_row_offset(row, WP / 8u) + (size_t)(w >> 3) * 256u + ((w >> 2) & 1u) * 128u + (w & 3u);
}

// One wave per selected site: list entry row0 + t is local site sel[t], t < rows.  rowsP (zeroed by the caller: pad dwords, pad
// rows and monomorphic rows stay zero) and cnt are indexed by the list position.  The row is read as the counts kernel reads it:
// 16 bytes per lane, nontemporal when one piece holds it (it then stays in registers for the second pass), cells >= N masked.
__global__ void __launch_bounds__(256) ld_pack_core_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, const uint32_t *sel,
                                                           uint32_t rows, uint32_t row0, uint32_t WP, uint32_t *rowsP, uint32_t *cnt)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (t >= rows) return;                   // (wave-uniform; no barrier follows)
    const uint8_t *src = state + (size_t)sel[t] * pitch;
    const uint32_t steps = (pitch + 1023u) >> 10, lofs = lane * 16u;
    const bool one = steps == 1u;
    auto piece = [&](uint32_t s, uint32_t (&x)[4]) {
        const uint32_t c0 = (s << 10) + lofs;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (c0 < pitch) v = ps_load_row16(src + c0, one);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        if (c0 + 16u > N) {
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) x[q] &= ps_state_cell_mask(c0 + 4u * q, N);
        }
    };
    uint32_t x[4], n[4] = { 0u, 0u, 0u, 0u };
    for (uint32_t s = 0; s < steps; s++) {
        piece(s, x);
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++)
#pragma unroll
            for (uint32_t a = 0; a < 4u; a++) n[a] += (uint32_t)__popc(ps_ld_eq_bytes(x[q], 0x01010101u << a));
    }
#pragma unroll
    for (uint32_t a = 0; a < 4u; a++) n[a] = ps_ld_wave_sum32(n[a]);
    uint32_t major = 0u, c = n[0];
#pragma unroll
    for (uint32_t a = 1; a < 4u; a++)
        if (n[a] > c) { c = n[a]; major = a; }       // (ties: the lowest byte stays)
    const uint32_t row = row0 + t;
    if (lane == 0u) cnt[row] = c;
    if (ps_ld_monomorphic(c, N)) return;
    const uint32_t m4 = 0x01010101u << major;
    for (uint32_t s = 0; s < steps; s++) {
        if (!one) piece(s, x);
        uint32_t bits = 0u;
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) bits |= ps_ld_gather4(ps_ld_eq_bytes(x[q], m4)) << (4u * q);
        // two lanes make a dword: the even one stores it
        const uint32_t other = (uint32_t)__shfl_xor((int)bits, 1, 64);
        const uint32_t w = (s << 5) + (lane >> 1);
        if ((lane & 1u) == 0u && w < WP) rowsP[ps_ld_dword_offset(row, w, WP)] = bits | (other << 16);
    }
}

// The same from the gene-major view: list entry row0 + t is gene sel[t], whose row holds W u64 words over the individuals.
__global__ void __launch_bounds__(256) ld_pack_acc_kernel(const uint64_t *accG, acc_dims d, const uint32_t *sel, uint32_t rows,
                                                          uint32_t row0, uint32_t WP, uint32_t *rowsP, uint32_t *cnt)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (t >= rows) return;
    const uint32_t *src = (const uint32_t *)(accG + (uint64_t)sel[t] * d.W);
    auto dword = [&](uint32_t w) {
        uint32_t v = w < 2u * d.W ? src[w] : 0u;
        const uint32_t first = w * 32u;          // (individuals >= N masked: nothing depends on the pad bits)
        if (first + 32u > d.N) v &= first >= d.N ? 0u : (1u << (d.N - first)) - 1u;
        return v;
    };
    uint32_t c = 0u;
    for (uint32_t w = lane; w < WP; w += 64u) c += (uint32_t)__popc(dword(w));
    c = ps_ld_wave_sum32(c);
    const uint32_t row = row0 + t;
    if (lane == 0u) cnt[row] = c;
    if (ps_ld_monomorphic(c, d.N)) return;
    for (uint32_t w = lane; w < WP; w += 64u) rowsP[ps_ld_dword_offset(row, w, WP)] = dword(w);
}

// dst |= src: the rows another shard packed (everything else in its buffer is zero) join shard 0's
__global__ void __launch_bounds__(256) ld_or_kernel(uint32_t *dst, const uint32_t *src, uint64_t n)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) dst[k] |= src[k];
}

// The pairs (a, b), b > a, of the band of list rows [lo, lo + nrows): In[(a - lo) * ldi + b] = n11 (u16; the contraction's pitch
// ldi >= M rounded up to 128), cnt and idx the ones and the columns of the M loci, both readable up to M rounded up to 4.
// Grid as pair_hist_kernel: x = workgroups of four waves striding over the 256-column chunks of a row, y strides over the rows;
// any grid is valid.  Dynamic LDS: lag_bins x r2_bins u32 bins (a band holds fewer than 2^32 pairs).  The sum of q of a lag bin
// goes lane -> LDS -> global, a lane adding only when its lag bin changes; the other sums per wave, per workgroup, then one
// global atomic per word.
__global__ void __launch_bounds__(256) ld_pair_kernel(const uint16_t *In, uint32_t ldi, const uint32_t *cnt, const uint32_t *idx, uint32_t N,
                                                      uint32_t M, uint32_t lo, uint32_t nrows, uint32_t r2_bins, uint32_t lag_bins,
                                                      unsigned long long *hist, unsigned long long *lag_sum, unsigned long long *words)
{
    extern __shared__ uint32_t ld_bins[];
    __shared__ unsigned long long ld_acc[PS_LD_WORDS], ld_lag[PS_LD_MAX_LAGS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t nbins = r2_bins * lag_bins;
    for (uint32_t b = tid; b < nbins; b += 256u) ld_bins[b] = 0u;
    if (tid < (uint32_t)PS_LD_WORDS) ld_acc[tid] = 0ull;
    if (tid < PS_LD_MAX_LAGS) ld_lag[tid] = 0ull;
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (tid >> 6)));
    const uint32_t nwaves = gridDim.x * 4u, nchunk = (M + 255u) >> 8;
    uint32_t n_undef = 0, n_four = 0, n_complete = 0, n_pos = 0, n_neg = 0, cur_lag = 0;
    uint64_t q_run = 0;
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t a = lo + r;
        if (a + 1u >= M) break;                 // (rows ascend: nothing right of the diagonal from here on)
        const uint32_t ca = cnt[a], sa = idx[a];
        const bool mono_a = ps_ld_monomorphic(ca, N);
        for (uint32_t c = ((a + 1u) >> 8) + wave; c < nchunk; c += nwaves) {
            const uint32_t j0 = (c << 8) + lane * 4u;
            if (j0 >= M || j0 + 3u <= a) continue;
            const uint2 i2 = *(const uint2 *)(In + (size_t)r * ldi + j0);
            const uint4 c4 = *(const uint4 *)(cnt + j0), s4 = *(const uint4 *)(idx + j0);
            const uint32_t iv[4] = { i2.x & 0xffffu, i2.x >> 16, i2.y & 0xffffu, i2.y >> 16 };
            const uint32_t cj[4] = { c4.x, c4.y, c4.z, c4.w }, sj[4] = { s4.x, s4.y, s4.z, s4.w };
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t b = j0 + k;
                if (b <= a || b >= M) continue;
                if (mono_a || ps_ld_monomorphic(cj[k], N)) { n_undef++; continue; }
                ps_ld_pair_t p;
                ps_ld_pair(N, ca, cj[k], iv[k], sa, sj[k], r2_bins, lag_bins, &p);
                atomicAdd(&ld_bins[p.lag_bin * r2_bins + p.r2_bin], 1u);
                if (p.lag_bin != cur_lag) {
                    if (q_run) atomicAdd(&ld_lag[cur_lag], (unsigned long long)q_run);
                    cur_lag = p.lag_bin;
                    q_run = 0;
                }
                q_run += p.q;
                n_four += p.four;
                n_complete += p.complete;
                n_pos += p.sign > 0 ? 1u : 0u;
                n_neg += p.sign < 0 ? 1u : 0u;
            }
        }
    }
    if (q_run) atomicAdd(&ld_lag[cur_lag], (unsigned long long)q_run);
    const unsigned long long u = ps_ph_wave_sum(n_undef), f = ps_ph_wave_sum(n_four), k = ps_ph_wave_sum(n_complete),
                             sp = ps_ph_wave_sum(n_pos), sn = ps_ph_wave_sum(n_neg);
    if (lane == 0u) {
        if (u) atomicAdd(&ld_acc[PS_LD_UNDEF], u);
        if (f) atomicAdd(&ld_acc[PS_LD_FOURG], f);
        if (k) atomicAdd(&ld_acc[PS_LD_COMPLETE], k);
        if (sp) atomicAdd(&ld_acc[PS_LD_POS], sp);
        if (sn) atomicAdd(&ld_acc[PS_LD_NEG], sn);
    }
    __syncthreads();
    if (tid < (uint32_t)PS_LD_WORDS && ld_acc[tid]) atomicAdd(&words[tid], ld_acc[tid]);
    if (tid < lag_bins && ld_lag[tid]) atomicAdd(&lag_sum[tid], ld_lag[tid]);
    for (uint32_t b = tid; b < nbins; b += 256u) {
        const uint32_t v = ld_bins[b];
        if (v) atomicAdd(&hist[b], (unsigned long long)v);
    }
}
