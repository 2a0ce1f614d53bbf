// cluster_kernels.h -- the kernels of ps_strain_clusters (docs/STRAIN_CLUSTERS.md) and the integer edge rule they share with
// the host restatement (ps_clusters_from_counts).
//
// pair_edge_kernel takes the per-band input of pair_hist_kernel -- the u32 Hamming numerators h(i, j) of rows [lo, lo + nrows)
// against all N columns, the u16 accessory intersections of the same rows, the rows' gene counts -- and writes row i of the
// upper-triangular adjacency bit matrix: W = ceil(N / 64) u64 words per row, bit j of row i set iff j > i and (i, j) is an
// edge.  cluster_hook_kernel and cluster_jump_kernel contract the matrix to labels L[N]: L[i] <= i, L[i] always a member
// of i's component, labels only ever decrease (atomicMin), so the fixed point -- L constant on components and equal to the
// smallest row -- does not depend on the order of the atomics or on the launch geometry.
#pragma once

#include <stdint.h>

enum { PS_CL_EDGES = 0, PS_CL_UNDEF, PS_CL_WORDS };

struct ps_cl_args {
    uint32_t d_max;      // core criterion: d = h / 2 <= d_max (d is below 2^31: a larger core_max_d is clamped)
    uint32_t num, den;   // accessory criterion: b != 0 and a den <= num b, num <= den <= 2^24
    uint64_t cg;         // core genes
};

// a < 2^33 and den <= 2^24: a den stays in 64 bits; num b, with b = U + core_genes of any size, takes 128
template <bool CORE, bool ACC>
__host__ __device__ __forceinline__ bool ps_cl_edge(uint32_t h, uint32_t in, uint32_t un, const ps_cl_args &a, bool *undefined)
{
    bool edge = true;
    *undefined = false;
    if (CORE) edge = (h >> 1) <= a.d_max;
    if (ACC) {
        const uint64_t b = (uint64_t)un + a.cg;
        *undefined = b == 0ull;
        edge = edge && b != 0ull && (unsigned __int128)((uint64_t)(un - in) * a.den) <= (unsigned __int128)a.num * b;
    }
    return edge;
}

__device__ __forceinline__ uint32_t ps_cl_load(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Grid as pair_hist_kernel: x = workgroups of four waves striding over the 256-column chunks of a row, y strides over the
// band's rows; any grid is valid.  A wave takes a chunk: lane l the columns l + 64 q (q = 0..3), so four ballots are the
// chunk's four finished words, stored by lanes 0..3.  Chunks wholly left of the diagonal are never read and their words
// never written (adj is zeroed per call).  In == nullptr: no accessory genes (I = U = 0 for every pair).
template <bool CORE, bool ACC>
__global__ void __launch_bounds__(256) pair_edge_kernel(const uint32_t *C, uint64_t ldc, const uint16_t *In, uint32_t ldi,
                                                        const uint32_t *rowcnt, uint32_t N, uint32_t lo, uint32_t nrows,
                                                        ps_cl_args a, unsigned long long *adj, unsigned long long *words)
{
    __shared__ unsigned long long cl_acc[PS_CL_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < (uint32_t)PS_CL_WORDS) cl_acc[tid] = 0ull;
    __syncthreads();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (tid >> 6)));
    const uint32_t nwaves = gridDim.x * 4u, nchunk = (N + 255u) >> 8, W = (N + 63u) >> 6;
    unsigned long long n_edges = 0, n_undef = 0;      // (wave-uniform: popcounts of ballots)
    for (uint32_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const uint32_t i = lo + r;
        if (i + 1u >= N) break;                 // (rows ascend: nothing right of the diagonal from here on, pad rows included)
        const uint32_t ci = (ACC && In) ? rowcnt[i] : 0u;
        for (uint32_t c = ((i + 1u) >> 8) + wave; c < nchunk; c += nwaves) {
            unsigned long long bits[4];
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                const uint32_t j = (c << 8) + (q << 6) + lane;
                const bool pair = j > i && j < N;       // (j < N <= ldc, ldi and the entries of rowcnt: every load stays inside its row)
                uint32_t h = 0u, in = 0u, cj = 0u;
                if (pair) {
                    if (CORE) h = C[(size_t)r * ldc + j];
                    if (ACC && In) {
                        in = In[(size_t)r * ldi + j];
                        cj = rowcnt[j];
                    }
                }
                bool undefined;
                const bool edge = ps_cl_edge<CORE, ACC>(h, in, ci + cj - in, a, &undefined) && pair;
                bits[q] = __ballot(edge);
                n_edges += (unsigned long long)__popcll(bits[q]);
                if (ACC) n_undef += (unsigned long long)__popcll(__ballot(undefined && pair));
            }
            const uint32_t w = (c << 2) + lane;
            if (lane < 4u && w < W) adj[(size_t)i * W + w] = lane == 0u ? bits[0] : lane == 1u ? bits[1] : lane == 2u ? bits[2] : bits[3];
        }
    }
    // per wave (the ballots), then per workgroup, then one global atomic per word
    if (lane == 0u) {
        if (n_edges) atomicAdd(&cl_acc[PS_CL_EDGES], n_edges);
        if (n_undef) atomicAdd(&cl_acc[PS_CL_UNDEF], n_undef);
    }
    __syncthreads();
    if (tid < (uint32_t)PS_CL_WORDS && cl_acc[tid]) atomicAdd(&words[tid], cl_acc[tid]);
}

__global__ void __launch_bounds__(256) cluster_init_kernel(uint32_t *L, uint32_t N)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < N) L[i] = i;
}

// One wave per row i (any grid: the waves stride over the rows): m = min(L[i], L[j] over the set bits j of the row), then
// atomicMin of m into L[i] and into every L[j] above it; *changed is raised if a label moved.  A lane's loops run over the
// words of one row and the at most 64 bits of a word.
__global__ void __launch_bounds__(256) cluster_hook_kernel(const unsigned long long *adj, uint32_t N, uint32_t *L, uint32_t *changed)
{
    const uint32_t lane = threadIdx.x & 63u, W = (N + 63u) >> 6;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    bool moved = false;
    for (uint32_t i = wave; i + 1u < N; i += gridDim.x * 4u) {
        const unsigned long long *row = adj + (size_t)i * W;
        const uint32_t w0 = (i + 1u) >> 6;
        uint32_t m = ps_cl_load(L + i);
        for (uint32_t w = w0 + lane; w < W; w += 64u)
            for (unsigned long long bits = row[w]; bits; bits &= bits - 1ull)
                m = min(m, ps_cl_load(L + (w << 6) + (uint32_t)__builtin_ctzll(bits)));      // (bits at or past N are never set)
#pragma unroll
        for (int o = 32; o; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o, 64));
        if (lane == 0u) moved = atomicMin(L + i, m) > m || moved;
        for (uint32_t w = w0 + lane; w < W; w += 64u)
            for (unsigned long long bits = row[w]; bits; bits &= bits - 1ull) {
                uint32_t *p = L + (w << 6) + (uint32_t)__builtin_ctzll(bits);
                if (ps_cl_load(p) > m) moved = atomicMin(p, m) > m || moved;
            }
    }
    if (moved) *changed = 1u;
}

// Pointer jumping: L[i] <- the end of the chain i -> L[i] -> L[L[i]] ...  A step goes to a strictly smaller row (L[x] <= x and
// the loop stops at L[x] == x), so the loop takes at most i steps, whatever the other threads store meanwhile.
__global__ void __launch_bounds__(256) cluster_jump_kernel(uint32_t N, uint32_t *L)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const uint32_t l0 = ps_cl_load(L + i);
    uint32_t l = l0;
    for (uint32_t p = ps_cl_load(L + l); p < l; p = ps_cl_load(L + l)) l = p;
    if (l < l0) atomicMin(L + i, l);
}
