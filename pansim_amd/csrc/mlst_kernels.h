// mlst_kernels.h -- the kernels of ps_allele_profiles (docs/ALLELE_PROFILES.md): fingerprints of the loci, their classes and
// dense allele numbers, the byte-for-byte verification of the classes and the allele distance of all pairs.
//
// A locus is a run of core sites, an allele a distinct byte sequence of that run.  mlst_fingerprint_kernel writes two u64
// words per (locus, INTERNAL row): word w = the sum over the locus's sites s of K_w(s) x byte, mod 2^64, K_w a keyed mix of
// the GLOBAL site index -- a sum, so the tables of the site shards of a run add (mlst_add_kernel).  mlst_canon_kernel takes
// equal fingerprints as one class and numbers the classes of a locus 0 .. A - 1 by first appearance in OUTPUT row order;
// mlst_verify_kernel compares every row with the representative of its class site by site, so that a call whose count of
// differing entries is 0 has exactly the classes of byte equality.  mlst_pair_kernel counts the loci at which two rows carry
// different numbers.  Every result is an integer sum, a minimum or a maximum: nothing depends on the launch geometry, the
// order of the atomics, the bands or the sharding.
#pragma once

#include <stdint.h>

enum { PS_MLST_SUM = 0, PS_MLST_MAX, PS_MLST_MININV, PS_MLST_IDENT, PS_MLST_EDGES, PS_MLST_BAD, PS_MLST_WORDS };

#define PS_MLST_EMPTY 0xFFFFFFFFu
#define PS_MLST_TILE 64u        // rows and columns of a tile of mlst_pair_kernel
#define PS_MLST_CHUNK 16u       // dwords (two loci each) of a row staged per step: the ids are padded to 2 x PS_MLST_CHUNK loci

// the finaliser of splitmix64
__host__ __device__ __forceinline__ uint64_t ps_mlst_mix(uint64_t x)
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// K_w(s): odd, masked to the low key_bits bits (mask = 2^key_bits - 1; at key_bits = 1 every key is 1)
__host__ __device__ __forceinline__ uint64_t ps_mlst_key(uint64_t seed, uint32_t w, uint64_t site, uint64_t mask)
{
    return (ps_mlst_mix(ps_mlst_mix(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(w + 1u)) ^ (site * 0xD1342543DE82EF95ull + (uint64_t)w)) | 1ull) & mask;
}

__device__ __forceinline__ uint32_t ps_mlst_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void ps_mlst_store(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// state: ncols x pitch bytes, the local sites [col_offset, col_offset + ncols) of the handle (pitch a multiple of 128, N live
// cells per row); bounds: the n_loci + 1 global site bounds.  Grid: x = the 256-individual chunks, y strides over the band's
// loci [g_lo, g_lo + nb).  A lane owns four individuals (one dword per site), the four waves of a workgroup take every fourth
// site of the locus and their partial sums add in LDS.  F[b * N + i]: the two words of band locus b and internal row i -- all
// of the band is written, zeros where the handle holds no site of the locus.
__global__ void __launch_bounds__(256) mlst_fingerprint_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, uint64_t col_offset, uint64_t ncols,
                                                               const unsigned long long *bounds, uint32_t g_lo, uint32_t nb, uint64_t seed,
                                                               uint64_t mask, ulonglong2 *F)
{
    __shared__ unsigned long long fp_part[3][2][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t i0 = (blockIdx.x * 64u + lane) * 4u;
    const bool live = i0 < pitch;              // (a dword inside the row: pitch is a multiple of 4)
    for (uint32_t b = blockIdx.y; b < nb; b += gridDim.y) {
        const uint64_t b_lo = bounds[g_lo + b], b_hi = bounds[g_lo + b + 1u], end = col_offset + ncols;
        const uint64_t lo = b_lo > col_offset ? b_lo : col_offset, hi = b_hi < end ? b_hi : end;
        unsigned long long a0[4] = { 0ull, 0ull, 0ull, 0ull }, a1[4] = { 0ull, 0ull, 0ull, 0ull };
#pragma unroll 4
        for (uint64_t s = lo + wave; s < hi; s += 4u) {
            const uint64_t k0 = ps_mlst_key(seed, 0u, s, mask), k1 = ps_mlst_key(seed, 1u, s, mask);      // (wave-uniform)
            const uint32_t v = live ? *(const uint32_t *)(state + (size_t)(s - col_offset) * pitch + i0) : 0u;
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                const uint64_t byte = (v >> (8u * q)) & 255u;
                a0[q] += k0 * byte;
                a1[q] += k1 * byte;
            }
        }
        if (wave) {
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                fp_part[wave - 1u][0][q * 64u + lane] = a0[q];
                fp_part[wave - 1u][1][q * 64u + lane] = a1[q];
            }
        }
        __syncthreads();
        if (!wave) {
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                for (uint32_t w = 0; w < 3u; w++) {
                    a0[q] += fp_part[w][0][q * 64u + lane];
                    a1[q] += fp_part[w][1][q * 64u + lane];
                }
                if (i0 + q < N) F[(size_t)b * N + i0 + q] = make_ulonglong2(a0[q], a1[q]);
            }
        }
        __syncthreads();
    }
}

// dst[w] += src[w] mod 2^64: the fingerprint table of another site shard
__global__ void __launch_bounds__(256) mlst_add_kernel(unsigned long long *dst, const unsigned long long *src, uint64_t n)
{
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (w < n) dst[w] += src[w];
}

// exclusive prefix sum of one value per thread over the workgroup (blockDim.x a multiple of 64, at most 1024); *total = the sum
__device__ __forceinline__ uint32_t ps_mlst_block_scan(uint32_t v, uint32_t *wave_sums, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= (uint32_t)o) inc += up;
    }
    __syncthreads();                 // (the sums of an earlier scan have been read)
    if (lane == 63u) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t base = 0u, all = 0u;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t s = wave_sums[w];
        base += w < wave ? s : 0u;
        all += s;
    }
    *total = all;
    return base + inc - v;
}

// One workgroup per locus of the band (any grid: the workgroups stride over the loci).  Per locus an open-addressing table of T
// rows (T a power of two >= 2 N, so never full) keyed by the fingerprint: a row claims the first free entry of its probe
// sequence or meets an entry of its own class, where atomicMin leaves the lowest OUTPUT row of the class -- entries are never
// freed, so all rows of a class stop at one entry, and its final content does not depend on the order of the insertions (which
// entry a class takes may).  Then
// rep[b * N + k] = that row; a row that is its own representative opens an allele, numbered by the count of such rows before
// it; ids[g * ldn + k] = the number of k's representative.  slot: the internal row of output row k (nullptr: the same).
// work: per workgroup T + 2 N u32 (table | class sizes | numbers) in global memory, or nullptr with as much dynamic LDS.
// Every probe loop is bounded by T.
__global__ void __launch_bounds__(1024) mlst_canon_kernel(const ulonglong2 *F, uint32_t N, const uint32_t *slot, uint32_t g_lo, uint32_t nb, uint32_t T,
                                                          uint32_t *work, uint32_t *rep, uint16_t *ids, uint32_t ldn, uint32_t *locus_alleles,
                                                          unsigned long long *locus_same)
{
    extern __shared__ uint32_t canon_lds[];
    __shared__ uint32_t canon_wave[16];
    __shared__ unsigned long long canon_same;
    const uint32_t tid = threadIdx.x, bd = blockDim.x;
    uint32_t *tab = work ? work + (size_t)blockIdx.x * ((size_t)T + 2u * (size_t)N) : canon_lds;
    uint32_t *cnt = tab + T, *num = cnt + N;
    const uint32_t per = (N + bd - 1u) / bd;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const ulonglong2 *Fb = F + (size_t)b * N;
        uint32_t *repb = rep + (size_t)b * N;
        for (uint32_t h = tid; h < T; h += bd) ps_mlst_store(tab + h, PS_MLST_EMPTY);
        for (uint32_t k = tid; k < N; k += bd) ps_mlst_store(cnt + k, 0u);
        if (tid == 0u) canon_same = 0ull;
        __syncthreads();
        for (uint32_t k = tid; k < N; k += bd) {
            const ulonglong2 fp = Fb[slot ? slot[k] : k];
            uint32_t h = (uint32_t)(ps_mlst_mix(fp.x + 0x9E3779B97F4A7C15ull * fp.y) >> 32) & (T - 1u);
            for (uint32_t step = 0; step < T; step++) {
                const uint32_t cur = atomicCAS(tab + h, PS_MLST_EMPTY, k);
                if (cur == PS_MLST_EMPTY) break;
                const ulonglong2 fc = Fb[slot ? slot[cur] : cur];       // (cur < N: only rows are stored)
                if (fc.x == fp.x && fc.y == fp.y) {
                    atomicMin(tab + h, k);
                    break;
                }
                h = (h + 1u) & (T - 1u);
            }
        }
        __syncthreads();
        for (uint32_t k = tid; k < N; k += bd) {
            const ulonglong2 fp = Fb[slot ? slot[k] : k];
            uint32_t h = (uint32_t)(ps_mlst_mix(fp.x + 0x9E3779B97F4A7C15ull * fp.y) >> 32) & (T - 1u), r = k;
            for (uint32_t step = 0; step < T; step++) {
                const uint32_t cur = ps_mlst_load(tab + h);
                if (cur >= N) break;                                     // (never: k's class has its entry before any free one)
                const ulonglong2 fc = Fb[slot ? slot[cur] : cur];
                if (fc.x == fp.x && fc.y == fp.y) {
                    r = cur;
                    break;
                }
                h = (h + 1u) & (T - 1u);
            }
            ps_mlst_store(repb + k, r);
            atomicAdd(cnt + r, 1u);
        }
        __syncthreads();
        // the rows [tid * per, (tid + 1) * per) in order: the representatives among them, numbered behind those of the rows before
        const uint32_t k_lo = min(N, tid * per), k_hi = min(N, k_lo + per);
        uint32_t mine = 0u;
        unsigned long long same = 0ull;
        for (uint32_t k = k_lo; k < k_hi; k++) mine += ps_mlst_load(repb + k) == k ? 1u : 0u;
        uint32_t alleles = 0u;
        uint32_t next = ps_mlst_block_scan(mine, canon_wave, &alleles);
        for (uint32_t k = k_lo; k < k_hi; k++) {
            if (ps_mlst_load(repb + k) != k) continue;
            const unsigned long long c = ps_mlst_load(cnt + k);
            same += c * (c - 1ull) / 2ull;
            ps_mlst_store(num + k, next++);
        }
        if (same) atomicAdd(&canon_same, same);
        __syncthreads();
        uint16_t *idg = ids + (size_t)(g_lo + b) * ldn;
        for (uint32_t k = tid; k < N; k += bd) idg[k] = (uint16_t)ps_mlst_load(num + ps_mlst_load(repb + k));
        if (tid == 0u) {
            locus_alleles[g_lo + b] = alleles;
            locus_same[g_lo + b] = canon_same;
        }
        __syncthreads();
    }
}

// The second pass: every (band locus, output row k) whose representative r is another row compares the bytes of the two rows
// over the sites of the locus that this handle holds; *bad += the entries that differ.  Grid: x = the 256-row chunks, y
// strides over the band's loci.  A wave whose rows are all their own representatives loads nothing but `rep`.
__global__ void __launch_bounds__(256) mlst_verify_kernel(const uint8_t *state, uint32_t pitch, uint32_t N, uint64_t col_offset, uint64_t ncols,
                                                          const unsigned long long *bounds, const uint32_t *slot, uint32_t g_lo, uint32_t nb,
                                                          const uint32_t *rep, unsigned long long *bad)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t nbad = 0u;
    for (uint32_t b = blockIdx.y; b < nb; b += gridDim.y) {
        const uint64_t b_lo = bounds[g_lo + b], b_hi = bounds[g_lo + b + 1u], end = col_offset + ncols;
        const uint64_t lo = b_lo > col_offset ? b_lo : col_offset, hi = b_hi < end ? b_hi : end;
        const uint32_t r = k < N ? rep[(size_t)b * N + k] : k;
        if (k < N && r != k && r < N) {
            const uint32_t ik = slot ? slot[k] : k, ir = slot ? slot[r] : r;      // (both below N <= pitch)
            bool differ = false;
            for (uint64_t s = lo; s < hi; s++) {
                const uint8_t *row = state + (size_t)(s - col_offset) * pitch;
                differ = differ || row[ik] != row[ir];
            }
            nbad += differ ? 1u : 0u;
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) nbad += (uint32_t)__shfl_xor((int)nbad, o, 64);
    if (lane == 0u && nbad) atomicAdd(bad, (unsigned long long)nbad);
}

typedef uint16_t ps_mlst_u16x2 __attribute__((ext_vector_type(2)));

// All pairs i < j of output rows over the u16 allele numbers ids[locus * ldn + row] (ldn a multiple of 64, the loci padded with
// zero rows to a multiple of 2 x PS_MLST_CHUNK: a pad locus differs nowhere).  Any grid: the workgroups stride over the 64 x 64
// tiles on and right of the diagonal; those left of it are never computed.  A thread holds a 4 x 4 micro-tile; the numbers of two loci share a dword, staged
// in LDS, so that XOR, a packed min with (1, 1) and a packed u16 add count two loci of a pair in three vector instructions
// (a half counts at most 32768 loci).  Per pair d = the loci that differ: bins[d dist_bins / (n_loci + 1)] (u32 in dynamic
// LDS, flushed as u64 atomics), the words, st[j] = min(st[j], i) where d = 0 (equality is transitive: the lowest row of a
// class reaches all of it) and, with adj != nullptr, bit j of row i of the upper-triangular adjacency matrix of
// pair_edge_kernel (W = ceil(N / 64) words per row, zeroed by the caller) where d <= complex_max.  Pad rows and columns are
// masked.
__global__ void __launch_bounds__(256) mlst_pair_kernel(const uint16_t *ids, uint32_t ldn, uint32_t N, uint32_t n_loci, uint32_t dist_bins,
                                                        uint32_t complex_max, unsigned long long *hist, unsigned long long *words, uint32_t *st,
                                                        unsigned long long *adj)
{
    extern __shared__ uint32_t mlst_bins[];
    __shared__ __attribute__((aligned(16))) uint32_t sI[PS_MLST_CHUNK][PS_MLST_TILE], sJ[PS_MLST_CHUNK][PS_MLST_TILE];
    __shared__ unsigned long long mlst_acc[PS_MLST_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, tx = tid & 15u, ty = tid >> 4;
    for (uint32_t b = tid; b < dist_bins; b += 256u) mlst_bins[b] = 0u;
    if (tid < (uint32_t)PS_MLST_WORDS) mlst_acc[tid] = 0ull;
    const uint32_t nt = (N + PS_MLST_TILE - 1u) / PS_MLST_TILE, W = (N + 63u) >> 6;
    const uint32_t ndw = ((n_loci + 2u * PS_MLST_CHUNK - 1u) / (2u * PS_MLST_CHUNK)) * PS_MLST_CHUNK;      // dwords per row, pad included
    unsigned long long sum = 0ull, ident = 0ull, edges = 0ull;
    uint32_t dmax = 0u, dmin = 0xFFFFFFFFu;
    const uint32_t one = 0x00010001u;
    // the tiles on and right of the diagonal, row after row: tile row bi holds nt - bi of them
    for (uint32_t t = blockIdx.x; t < nt * (nt + 1u) / 2u; t += gridDim.x) {
        uint32_t bi = 0u, rest = t;
        while (rest >= nt - bi) rest -= nt - bi++;          // (at most nt steps, the same for the whole workgroup)
        const uint32_t bj = bi + rest;
        ps_mlst_u16x2 d[4][4];
#pragma unroll
        for (uint32_t r = 0; r < 4u; r++)
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) d[r][q] = (ps_mlst_u16x2){ 0, 0 };
        // staging: a thread takes the rows 2 xp and 2 xp + 1 of the dwords cs and cs + 8 of a chunk, one dword load per locus and
        // side (the ids of two neighbouring rows; every offset is a multiple of 4 bytes and below ldn), and holds the next chunk
        // in registers while the workgroup counts the current one
        static_assert(PS_MLST_TILE == 64u && PS_MLST_CHUNK == 16u, "256 threads stage 2 x 2 x 16 x 64 ids");
        const uint32_t xp = tid & 31u, cs = tid >> 5;
        const uint16_t *colI = ids + bi * PS_MLST_TILE + 2u * xp, *colJ = ids + bj * PS_MLST_TILE + 2u * xp;
        uint32_t nI[2][2], nJ[2][2];
        auto fetch = [&](uint32_t c0) {
#pragma unroll
            for (uint32_t u = 0; u < 2u; u++) {
                const size_t row = (size_t)(2u * (c0 + cs + 8u * u)) * ldn;
                nI[u][0] = *(const uint32_t *)(colI + row);
                nI[u][1] = *(const uint32_t *)(colI + row + ldn);
                nJ[u][0] = *(const uint32_t *)(colJ + row);
                nJ[u][1] = *(const uint32_t *)(colJ + row + ldn);
            }
        };
        fetch(0u);
        for (uint32_t c0 = 0; c0 < ndw; c0 += PS_MLST_CHUNK) {
            __syncthreads();                    // (the chunk before has been read; the first time: the bins are zero)
#pragma unroll
            for (uint32_t u = 0; u < 2u; u++) {
                *(uint2 *)&sI[cs + 8u * u][2u * xp] = make_uint2((nI[u][0] & 0xFFFFu) | (nI[u][1] << 16), (nI[u][0] >> 16) | (nI[u][1] & 0xFFFF0000u));
                *(uint2 *)&sJ[cs + 8u * u][2u * xp] = make_uint2((nJ[u][0] & 0xFFFFu) | (nJ[u][1] << 16), (nJ[u][0] >> 16) | (nJ[u][1] & 0xFFFF0000u));
            }
            __syncthreads();
            if (c0 + PS_MLST_CHUNK < ndw) fetch(c0 + PS_MLST_CHUNK);
#pragma unroll 8
            for (uint32_t c = 0; c < PS_MLST_CHUNK; c++) {
                const uint4 a = *(const uint4 *)&sI[c][ty * 4u], v = *(const uint4 *)&sJ[c][tx * 4u];
                const uint32_t av[4] = { a.x, a.y, a.z, a.w }, bv[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                for (uint32_t r = 0; r < 4u; r++)
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++) {
                        // (said in so many words: the compiler expands a packed min with a constant into compares and selects)
                        uint32_t ne;
                        asm("v_pk_min_u16 %0, %1, %2" : "=v"(ne) : "v"(av[r] ^ bv[q]), "v"(one));
                        d[r][q] += __builtin_bit_cast(ps_mlst_u16x2, ne);
                    }
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < 4u; r++) {
            const uint32_t i = bi * PS_MLST_TILE + ty * 4u + r;
            unsigned long long bits = 0ull;
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                const uint32_t j = bj * PS_MLST_TILE + tx * 4u + q;
                if (!(i < j && j < N)) continue;
                const uint32_t dd = (uint32_t)d[r][q].x + (uint32_t)d[r][q].y;
                atomicAdd(&mlst_bins[(uint32_t)(((uint64_t)dd * dist_bins) / (n_loci + 1u))], 1u);
                sum += dd;
                dmax = max(dmax, dd);
                dmin = min(dmin, dd);
                if (dd == 0u) {
                    ident++;
                    atomicMin(st + j, i);
                }
                if (dd <= complex_max) {
                    edges++;
                    bits |= 1ull << (tx * 4u + q);
                }
            }
            if (adj && bits) atomicOr(adj + (size_t)i * W + bj, bits);
        }
    }
    uint32_t inv = 0xFFFFFFFFu - dmin;          // (0 for a thread without a pair)
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        ident += __shfl_xor(ident, o, 64);
        edges += __shfl_xor(edges, o, 64);
        dmax = max(dmax, (uint32_t)__shfl_xor((int)dmax, o, 64));
        inv = max(inv, (uint32_t)__shfl_xor((int)inv, o, 64));
    }
    __syncthreads();                            // (a workgroup without a tile: the zeroed words)
    if (lane == 0u) {
        if (sum) atomicAdd(&mlst_acc[PS_MLST_SUM], sum);
        if (ident) atomicAdd(&mlst_acc[PS_MLST_IDENT], ident);
        if (edges) atomicAdd(&mlst_acc[PS_MLST_EDGES], edges);
        atomicMax(&mlst_acc[PS_MLST_MAX], (unsigned long long)dmax);
        atomicMax(&mlst_acc[PS_MLST_MININV], (unsigned long long)inv);
    }
    __syncthreads();
    if (tid == (uint32_t)PS_MLST_MAX || tid == (uint32_t)PS_MLST_MININV) {
        if (mlst_acc[tid]) atomicMax(&words[tid], mlst_acc[tid]);
    } else if (tid < (uint32_t)PS_MLST_BAD && mlst_acc[tid]) {
        atomicAdd(&words[tid], mlst_acc[tid]);
    }
    for (uint32_t b = tid; b < dist_bins; b += 256u) {
        const uint32_t v = mlst_bins[b];
        if (v) atomicAdd(&hist[b], (unsigned long long)v);
    }
}
