// sample_kernels.h -- the kernels of the isolate samples (isolate_samples.h; docs/ISOLATE_SAMPLES.md): the requested rows of a
// population gathered into a new one on the device.  The core matrix is site-major (state[site][pitch] bytes), so a sample is a
// gather WITHIN every site row, L times with the same index list; the accessory matrix is individual-major bit rows, so a sample
// copies whole rows of GW words.  Included by pansim_capi.hip in front of isolate_samples.h.
#pragma once

// the forms and the grid of core_gather_rows_kernel (PS_GATHER_*)
#include "sample_plan.h"

// the index list of one part: idx[j] = the internal row (the byte column of the core matrix) of requested output row rows[j];
// rows == nullptr: every row in order; slot == nullptr: output order = internal order
__global__ void sample_index_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ slot, uint32_t n, uint32_t *__restrict__ idx)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = rows ? rows[j] : j;
    idx[j] = slot ? slot[r] : r;
}

// out[site][off + j] = in[site][idx[j]] for j < n and the sites [0, L) of one handle.  A thread owns CH 16-byte chunks of the
// output row (chunk c = bytes [16 c, 16 c + 16)), keeps their indices and byte masks in registers and reuses them for every site of
// the workgroup's run of `sites_per_wg` sites; blockDim.y sites are in flight at once.  LDS form (DIRECT = false, pitch_in <=
// PS_GATHER_LDS_PITCH, dynamic LDS = blockDim.y * pitch_in): the blockDim.y source rows, contiguous in memory, are staged with
// 16-byte loads and every output dword is assembled from four LDS byte reads; the indices are packed two to a register.  Direct
// form: the bytes are loaded from global memory (rows that do not fit the LDS, and n << N, where n sectors are fewer bytes than the
// row).  The bytes of [off + n, own_end) are written as zeros (the pad of the output row: own_end = pitch_out in the launch of the
// last part, off + n in the others).  A chunk whose 16 bytes all lie in [off, own_end) is one 16-byte store; the chunks at the
// edges of the range write their own bytes with byte stores, so launches of neighbouring parts never touch each other's bytes and
// need no order.  grid.x: tiles of blockDim.x * CH chunks; grid.y: runs of sites.
template <int CH, bool DIRECT>
__global__ void __launch_bounds__(1024) core_gather_rows_kernel(const uint8_t *__restrict__ in, uint32_t pitch_in, uint8_t *__restrict__ out,
                                                                uint32_t pitch_out, const uint32_t *__restrict__ idx, uint32_t n, uint32_t off,
                                                                uint32_t own_end, uint64_t L, uint32_t sites_per_wg)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t gather_lds[];
    constexpr int IW = DIRECT ? 16 : 8;
    const uint32_t tx = threadIdx.x, sy = threadIdx.y, TX = blockDim.x, SY = blockDim.y;
    const uint64_t end = (uint64_t)off + n;
    const uint64_t c_end = ((uint64_t)own_end + 15u) / 16u;
    uint32_t ix[CH][IW], keep[CH][4], own[CH], chunk[CH];
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const uint64_t c = (uint64_t)off / 16u + ((uint64_t)blockIdx.x * CH + k) * TX + tx;
        chunk[k] = (uint32_t)c;
        own[k] = 0;
#pragma unroll
        for (int w = 0; w < IW; w++) ix[k][w] = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) keep[k][w] = 0;
        if (c >= c_end) continue;
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const uint64_t pos = 16u * c + b;
            if (pos < off || pos >= own_end) continue;
            own[k] |= 1u << b;
            if (pos >= end) continue;
            const uint32_t i = idx[pos - off];
            keep[k][b / 4] |= 0xFFu << (8 * (b % 4));
            if (DIRECT) ix[k][b] = i;
            else ix[k][b / 2] |= i << (16 * (b % 2));
        }
    }
    const uint64_t s_begin = (uint64_t)blockIdx.y * sites_per_wg, s_end = s_begin + sites_per_wg < L ? s_begin + sites_per_wg : L;
    for (uint64_t s0 = s_begin; s0 < s_end; s0 += SY) {
        const uint32_t ns = (uint32_t)(s_end - s0 < SY ? s_end - s0 : SY);
        if (!DIRECT) {
            __syncthreads();                        // (the reads of the sites before)
            const uint4 *src = (const uint4 *)(in + s0 * pitch_in);
            const uint32_t total = ns * (pitch_in / 16u);
            for (uint32_t i = sy * TX + tx; i < total; i += TX * SY) ((uint4 *)gather_lds)[i] = src[i];
            __syncthreads();
        }
        if (sy >= ns) continue;
        const uint8_t *row = DIRECT ? in + (s0 + sy) * pitch_in : gather_lds + (size_t)sy * pitch_in;
        uint8_t *orow = out + (s0 + sy) * pitch_out;
#pragma unroll
        for (int k = 0; k < CH; k++) {
            if (!own[k]) continue;
            uint32_t w[4];
#pragma unroll
            for (int d = 0; d < 4; d++) {
                uint32_t x = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const uint32_t i = DIRECT ? ix[k][4 * d + b] : (ix[k][(4 * d + b) / 2] >> (16 * (b % 2))) & 0xFFFFu;
                    x |= (uint32_t)row[i] << (8 * b);
                }
                w[d] = x & keep[k][d];
            }
            uint8_t *dst = orow + 16ull * chunk[k];
            if (own[k] == 0xFFFFu) {
                *(uint4 *)dst = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int b = 0; b < 16; b++)
                    if (own[k] >> b & 1u) dst[b] = (uint8_t)(w[b / 4] >> (8 * (b % 4)));
            }
        }
    }
}

// out[j][w] = in[idx[j]][w] for j < n: whole bit rows of GW words (the pad bits of the last word travel as the zeros they are)
__global__ void acc_gather_rows_kernel(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, const uint32_t *__restrict__ idx, uint64_t n,
                                       uint32_t GW)
{
    const uint64_t total = n * GW;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = t / GW;
        out[t] = in[(uint64_t)idx[j] * GW + (t - j * GW)];
    }
}
