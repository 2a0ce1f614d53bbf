// gene_site_kernels.h -- the gfx950 kernel of the gene-site association (ps_gene_site_ld, include/pansim_hip.h; the definitions:
// docs/GENE_SITE_ASSOCIATION.md) and the integer rules it shares with the host restatement (ps_gene_site_from_counts).
//
// The two lists live in ONE blocked bit operand (the layout of ld_kernels.h): genes at the list positions [0, Mg), sites at
// [Mg, Mg + Ms), packed by ld_pack_acc_kernel and ld_pack_core_kernel.  The contraction (acc_intersections_mfma_kernel) runs over
// bands of gene rows and all columns; gene_site_pair_kernel reads the site columns of a band only.  Every sum is an integer sum
// and every maximum is one of strictly ordered keys: nothing depends on the grid or on the order of the atomics.
#pragma once

#include "ld_kernels.h"

// the summary words the pair kernel accumulates (u64 each); the defined pairs follow from the bins, sum_q from the frequency sums
enum { PS_GS_UNDEF = 0, PS_GS_FOURG, PS_GS_COMPLETE, PS_GS_POS, PS_GS_NEG, PS_GS_STRONG, PS_GS_WORDS = 8 };

// the frequency bin of a gene with c ones among N individuals
PS_HD uint32_t ps_gs_freq_bin(uint32_t c, uint32_t N, uint32_t freq_bins)
{
    const uint32_t m = c < N - c ? c : N - c;
    const uint32_t b = 2u * m * freq_bins / N;         // (m <= 2^15 and freq_bins <= 2^14: the product fits 32 bits)
    return b < freq_bins - 1u ? b : freq_bins - 1u;
}

// One candidate of an arg-max as a key: q first, then the LOWER list position of the partner, then the sign of D; bit 0 makes
// every defined pair differ from 0 = "no defined pair".  Two candidates of one locus never share a partner: the order is strict.
PS_HD uint64_t ps_gs_key(uint32_t q, uint32_t partner, int32_t sign)
{
    return ((uint64_t)q << 19) | ((uint64_t)(65535u - partner) << 3) | ((uint64_t)(uint32_t)(sign + 1) << 1) | 1ull;
}
PS_HD uint32_t ps_gs_key_q(uint64_t k) { return (uint32_t)(k >> 19); }
PS_HD uint32_t ps_gs_key_partner(uint64_t k) { return 65535u - ((uint32_t)(k >> 3) & 0xffffu); }
PS_HD int32_t ps_gs_key_sign(uint64_t k) { return (int32_t)((uint32_t)(k >> 1) & 3u) - 1; }

__device__ __forceinline__ unsigned long long ps_gs_wave_max(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long w = (unsigned long long)__shfl_xor((long long)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// The pairs (gene a, site b) of the band of gene rows [lo, lo + nrows): In[(a - lo) * ldi + Mg + b] = n11 (u16; the contraction's
// pitch ldi > Mg + Ms rounded up to 128), cnt the ones of the Mg + Ms list entries, readable up to the next multiple of 4.
// Grid: x = workgroups of four waves striding over the 256-column chunks of the site columns (from Mg rounded down to 4: the
// loads stay aligned, the columns below Mg are skipped), y strides over the band's rows; any grid is valid.  A wave keeps one
// chunk while it walks the rows, so that what belongs to a SITE (its strong pairs, its best gene) stays in the lane's registers
// and leaves as one atomic per site, chunk and y; what belongs to the GENE of a row (strong pairs, sum of q, best site) is reduced
// in the wave per row.  Dynamic LDS: freq_bins x r2_bins u32 bins (a band holds fewer than 2^32 pairs).  The sum of q of a
// frequency bin is a run per wave: lane 0 adds to the global sum only when the bin changes.  The summary words go per wave, per
// workgroup, then one global atomic per word.
__global__ void __launch_bounds__(256) gene_site_pair_kernel(const uint16_t *In, uint32_t ldi, const uint32_t *cnt, uint32_t N, uint32_t Mg,
                                                             uint32_t Ms, uint32_t lo, uint32_t nrows, uint32_t r2_bins, uint32_t freq_bins,
                                                             uint32_t strong_q, unsigned long long *hist, unsigned long long *freq_sum,
                                                             unsigned long long *words, uint32_t *gene_strong, uint32_t *site_strong,
                                                             unsigned long long *gene_key, unsigned long long *site_key)
{
    extern __shared__ uint32_t gs_bins[];
    __shared__ unsigned long long gs_acc[PS_GS_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t nbins = r2_bins * freq_bins;
    for (uint32_t b = tid; b < nbins; b += 256u) gs_bins[b] = 0u;
    if (tid < (uint32_t)PS_GS_WORDS) gs_acc[tid] = 0ull;
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (tid >> 6)));
    const uint32_t nwaves = gridDim.x * 4u, col0 = Mg & ~3u, Mt = Mg + Ms, nchunk = (Mt - col0 + 255u) >> 8;
    uint32_t n_undef = 0, n_four = 0, n_complete = 0, n_pos = 0, n_neg = 0, n_strong = 0;
    uint32_t cur_fb = 0;                          // (wave-uniform, as q_run)
    unsigned long long q_run = 0;
    for (uint32_t c = wave; c < nchunk; c += nwaves) {
        const uint32_t j0 = col0 + (c << 8) + lane * 4u;
        const bool any = j0 < Mt;                 // (j0 + 3 < the pad of cnt and of a row of In either way; nothing is read beyond Mt rounded up to 4)
        uint4 c4 = make_uint4(0u, 0u, 0u, 0u);
        if (any) c4 = *(const uint4 *)(cnt + j0);
        const uint32_t cj[4] = { c4.x, c4.y, c4.z, c4.w };
        bool valid[4], mono[4];
        uint32_t n_valid = 0, s_strong[4] = { 0u, 0u, 0u, 0u };
        unsigned long long s_key[4] = { 0ull, 0ull, 0ull, 0ull };
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            valid[k] = j0 + k >= Mg && j0 + k < Mt;
            mono[k] = ps_ld_monomorphic(cj[k], N);
            n_valid += valid[k] ? 1u : 0u;
        }
        for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
            const uint32_t a = lo + r;            // (lo + nrows <= Mg: the host bands the gene rows only)
            const uint32_t ca = cnt[a];
            if (ps_ld_monomorphic(ca, N)) { n_undef += n_valid; continue; }      // (wave-uniform)
            const uint32_t fb = ps_gs_freq_bin(ca, N, freq_bins);
            uint2 i2 = make_uint2(0u, 0u);
            if (any) i2 = *(const uint2 *)(In + (size_t)r * ldi + j0);
            const uint32_t iv[4] = { i2.x & 0xffffu, i2.x >> 16, i2.y & 0xffffu, i2.y >> 16 };
            unsigned long long g_key = 0ull, g_sum = 0ull;       // g_sum: the strong pairs above bit 32, the sum of q (< 2^27 per wave) below
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                if (!valid[k]) continue;
                if (mono[k]) { n_undef++; continue; }
                ps_ld_pair_t p;
                ps_ld_pair(N, ca, cj[k], iv[k], 0u, 1u, r2_bins, 1u, &p);
                atomicAdd(&gs_bins[fb * r2_bins + p.r2_bin], 1u);
                const uint32_t strong = p.q >= strong_q ? 1u : 0u;
                g_sum += ((unsigned long long)strong << 32) | p.q;
                n_strong += strong;
                s_strong[k] += strong;
                n_four += p.four;
                n_complete += p.complete;
                n_pos += p.sign > 0 ? 1u : 0u;
                n_neg += p.sign < 0 ? 1u : 0u;
                const unsigned long long kg = ps_gs_key(p.q, j0 + k - Mg, p.sign), ks = ps_gs_key(p.q, a, p.sign);
                g_key = kg > g_key ? kg : g_key;
                s_key[k] = ks > s_key[k] ? ks : s_key[k];
            }
            g_key = ps_gs_wave_max(g_key);
            g_sum = ps_ph_wave_sum(g_sum);
            if (lane == 0u) {
                if (g_key) atomicMax(&gene_key[a], g_key);
                if (g_sum >> 32) atomicAdd(&gene_strong[a], (uint32_t)(g_sum >> 32));
                if (fb != cur_fb) {
                    if (q_run) atomicAdd(&freq_sum[cur_fb], q_run);
                    cur_fb = fb;
                    q_run = 0ull;
                }
                q_run += g_sum & 0xffffffffull;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            if (!valid[k]) continue;
            if (s_strong[k]) atomicAdd(&site_strong[j0 + k - Mg], s_strong[k]);
            if (s_key[k]) atomicMax(&site_key[j0 + k - Mg], s_key[k]);
        }
    }
    if (lane == 0u && q_run) atomicAdd(&freq_sum[cur_fb], q_run);
    const unsigned long long u = ps_ph_wave_sum(n_undef), f = ps_ph_wave_sum(n_four), k = ps_ph_wave_sum(n_complete),
                             sp = ps_ph_wave_sum(n_pos), sn = ps_ph_wave_sum(n_neg), st = ps_ph_wave_sum(n_strong);
    if (lane == 0u) {
        if (u) atomicAdd(&gs_acc[PS_GS_UNDEF], u);
        if (f) atomicAdd(&gs_acc[PS_GS_FOURG], f);
        if (k) atomicAdd(&gs_acc[PS_GS_COMPLETE], k);
        if (sp) atomicAdd(&gs_acc[PS_GS_POS], sp);
        if (sn) atomicAdd(&gs_acc[PS_GS_NEG], sn);
        if (st) atomicAdd(&gs_acc[PS_GS_STRONG], st);
    }
    __syncthreads();
    if (tid < (uint32_t)PS_GS_WORDS && gs_acc[tid]) atomicAdd(&words[tid], gs_acc[tid]);
    for (uint32_t b = tid; b < nbins; b += 256u) {
        const uint32_t v = gs_bins[b];
        if (v) atomicAdd(&hist[b], (unsigned long long)v);
    }
}
