// Where does the wave sweep stand between its two ceilings?  The sweep's skeleton -- out of place, nontemporal 16-byte row
// loads, rows staged in wave-private LDS, the 16-byte-per-lane byte gather, nontemporal stores, 3 rows per wave and trip --
// with a dial for the vector-ALU work per row: R rounds of Philox4x32 per lane and row (~7 VALU instructions each; the real
// kernel issues ~195 VALU wave-instructions per row, i.e. R ~ 28).  time(R) tells which ceiling binds at the operating point:
// flat in R = the memory skeleton, rising = the vector ALUs.
//   hipcc --offload-arch=gfx950 -O3 -o sweep_skeleton sweep_skeleton.hip && ./sweep_skeleton [blocks per CU = 7]
// ./sweep_skeleton gens [chunk | transposed | both] [blocks per CU = 4]: the two lane mappings of the gather over two
// generations per pass with sorted parents (skeleton_gens; profiles/sweep_transposed_gather.md 1)
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void philox_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0, uint32_t k1)
{
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
}

template <int ROWS, int R, bool GATHER>
__global__ void __launch_bounds__(256, 8) skeleton(const uint8_t *x, uint8_t *y, const uint32_t *idx, uint32_t rows, uint32_t pitch, uint32_t seed)
{
    __shared__ __attribute__((aligned(16))) uint8_t buf[4][ROWS * 1024];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    uint32_t pidx[16];
#pragma unroll
    for (int k = 0; k < 16; k++) pidx[k] = idx[lane * 16 + k];
    for (uint32_t r0 = wave * ROWS; r0 < rows; r0 += nwaves * ROWS) {
        u32x4 v[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS; k++)
            v[k] = __builtin_nontemporal_load((const u32x4 *)(x + (size_t)min(r0 + k, rows - 1u) * pitch + lane * 16u));
#pragma unroll
        for (int k = 0; k < ROWS; k++) *(u32x4 *)(buf[w] + k * 1024 + lane * 16u) = v[k];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < ROWS; k++) {
            uint32_t o[4];
            if (GATHER) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    uint32_t t = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) t |= (uint32_t)buf[w][k * 1024 + pidx[4 * j + b]] << (8 * b);
                    o[j] = t;
                }
            } else {
                const u32x4 t = *(const u32x4 *)(buf[w] + k * 1024 + lane * 16u);
                o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
            }
            // the dial: R Philox rounds keyed on (row, lane); the result touches one bit of the row so that nothing is dead
            uint32_t c0 = r0 + k, c1 = lane, c2 = seed, c3 = 1u, k0 = seed, k1 = 0x9E3779B9u;
#pragma unroll
            for (int r = 0; r < R; r++) { philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
            if (R) o[0] ^= (c0 ^ c1 ^ c2 ^ c3) & 1u;
            if (r0 + k < rows) {
                u32x4 s = { o[0], o[1], o[2], o[3] };
                __builtin_nontemporal_store(s, (u32x4 *)(y + (size_t)(r0 + k) * pitch + lane * 16u));
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// the same with the next trip's row loads issued BEFORE this trip's gather and ALU work (register double buffer)
template <int ROWS, int R>
__global__ void __launch_bounds__(256, 8) skeleton_prefetch(const uint8_t *x, uint8_t *y, const uint32_t *idx, uint32_t rows, uint32_t pitch, uint32_t seed)
{
    __shared__ __attribute__((aligned(16))) uint8_t buf[4][ROWS * 1024];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    uint32_t pidx[16];
#pragma unroll
    for (int k = 0; k < 16; k++) pidx[k] = idx[lane * 16 + k];
    u32x4 v[ROWS], n[ROWS];
    uint32_t r0 = wave * ROWS;
    if (r0 < rows) {
#pragma unroll
        for (int k = 0; k < ROWS; k++) v[k] = __builtin_nontemporal_load((const u32x4 *)(x + (size_t)min(r0 + k, rows - 1u) * pitch + lane * 16u));
    }
    for (; r0 < rows; r0 += nwaves * ROWS) {
        const uint32_t rn = r0 + nwaves * ROWS;
#pragma unroll
        for (int k = 0; k < ROWS; k++) *(u32x4 *)(buf[w] + k * 1024 + lane * 16u) = v[k];
        if (rn < rows) {
#pragma unroll
            for (int k = 0; k < ROWS; k++) n[k] = __builtin_nontemporal_load((const u32x4 *)(x + (size_t)min(rn + k, rows - 1u) * pitch + lane * 16u));
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < ROWS; k++) {
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t t = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) t |= (uint32_t)buf[w][k * 1024 + pidx[4 * j + b]] << (8 * b);
                o[j] = t;
            }
            uint32_t c0 = r0 + k, c1 = lane, c2 = seed, c3 = 1u, k0 = seed, k1 = 0x9E3779B9u;
#pragma unroll
            for (int r = 0; r < R; r++) { philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
            if (R) o[0] ^= (c0 ^ c1 ^ c2 ^ c3) & 1u;
            if (r0 + k < rows) {
                u32x4 s = { o[0], o[1], o[2], o[3] };
                __builtin_nontemporal_store(s, (u32x4 *)(y + (size_t)(r0 + k) * pitch + lane * 16u));
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < ROWS; k++) v[k] = n[k];
    }
}

// The gather forms of the real kernel's generation loop: GENS generations applied to the LDS rows between one load and one
// store, 4 rows per wave and trip, 4 workgroups per CU.  TRANSPOSED false: lane l gathers the 16 children of its own chunk
// (16 l + k) and stores them with one ds_write_b128.  true: lane l gathers the child dwords l + 64 m (children
// 4 (l + 64 m) + b), stores them with four ds_write_b32, and the chunk owner reads its 16 bytes back (ds_read_b128) for the
// per-chunk work before its ds_write_b128 -- the read-modify-write the mutations of the real kernel need.
__device__ __forceinline__ void lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int R, int GENS, bool TRANSPOSED>
__global__ void __launch_bounds__(256, 4) skeleton_gens(const uint8_t *x, uint8_t *y, const uint32_t *idx, uint32_t rows, uint32_t pitch, uint32_t seed)
{
    constexpr int ROWS = 4;
    __shared__ __attribute__((aligned(16))) uint8_t buf[4][ROWS * 1024];
    const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    uint32_t pidx[GENS][16];
#pragma unroll
    for (int g = 0; g < GENS; g++)
#pragma unroll
        for (int k = 0; k < 16; k++)
            pidx[g][k] = idx[g * 1024 + (TRANSPOSED ? 4 * (lane + 64 * (k >> 2)) + (k & 3) : lane * 16 + k)];
    for (uint32_t r0 = wave * ROWS; r0 < rows; r0 += nwaves * ROWS) {
#pragma unroll
        for (int k = 0; k < ROWS; k++)
            *(u32x4 *)(buf[w] + k * 1024 + lane * 16u) = __builtin_nontemporal_load((const u32x4 *)(x + (size_t)min(r0 + k, rows - 1u) * pitch + lane * 16u));
        lds_fence();
#pragma unroll
        for (int g = 0; g < GENS; g++) {
#pragma unroll
            for (int k = 0; k < ROWS; k++) {
                uint8_t *row = buf[w] + k * 1024;
                uint32_t o[4];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    uint32_t t = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++) t |= (uint32_t)row[pidx[g][4 * j + b]] << (8 * b);
                    o[j] = t;
                }
                lds_fence();
                if (TRANSPOSED) {
#pragma unroll
                    for (int m = 0; m < 4; m++) *(uint32_t *)(row + 4u * (lane + 64u * m)) = o[m];
                    lds_fence();
                    const u32x4 t = *(const u32x4 *)(row + lane * 16u);
                    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
                }
                uint32_t c0 = r0 + k, c1 = lane, c2 = seed + g, c3 = 1u, k0 = seed, k1 = 0x9E3779B9u;
#pragma unroll
                for (int r = 0; r < R; r++) { philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
                if (R) o[0] ^= (c0 ^ c1 ^ c2 ^ c3) & 1u;
                const u32x4 s = { o[0], o[1], o[2], o[3] };
                *(u32x4 *)(row + lane * 16u) = s;
                __builtin_amdgcn_sched_barrier(0);
            }
            lds_fence();
        }
#pragma unroll
        for (int k = 0; k < ROWS; k++)
            if (r0 + k < rows)
                __builtin_nontemporal_store(*(const u32x4 *)(buf[w] + k * 1024 + lane * 16u), (u32x4 *)(y + (size_t)(r0 + k) * pitch + lane * 16u));
        lds_fence();
    }
}

// 1000 sorted draws of 1000 equally likely parents per generation (ps_sim's children in ascending parent order); the 24
// cells past them gather the row's first padding byte
static void sorted_parents(uint32_t *h, uint32_t s)
{
    uint32_t cnt[1000] = { 0 };
    for (int i = 0; i < 1000; i++) { s = s * 1664525u + 1013904223u; cnt[(s >> 8) % 1000u]++; }
    int n = 0;
    for (uint32_t p = 0; p < 1000; p++)
        for (uint32_t c = 0; c < cnt[p]; c++) h[n++] = p;
    for (; n < 1024; n++) h[n] = 1000;
}

int main(int argc, char **argv)
{
    // ./sweep_skeleton gens [chunk | transposed | both] [blocks per CU = 4]: the two gather forms over two generations per pass
    const bool gens = argc > 1 && !strcmp(argv[1], "gens");
    const char *form = gens && argc > 2 ? argv[2] : "both";
    const int bpc = gens ? (argc > 3 ? atoi(argv[3]) : 4) : argc > 1 ? atoi(argv[1]) : 7;
    const uint32_t rows = 1200000, pitch = 1024;
    const size_t bytes = (size_t)rows * pitch;
    uint8_t *x, *y;
    uint32_t *idx;
    hipMalloc(&x, bytes);
    hipMalloc(&y, bytes);
    hipMemset(x, 1, bytes);
    hipMemset(y, 1, bytes);
    hipMalloc(&idx, 2 * 1024 * 4);
    uint32_t h[2 * 1024], s = 12345;
    for (int i = 0; i < 1024; i++) { s = s * 1664525u + 1013904223u; h[i] = (s >> 8) % 1000u; }
    if (gens) {
        sorted_parents(h, 12345u);
        sorted_parents(h + 1024, 54321u);
    }
    hipMemcpy(idx, h, sizeof(h), hipMemcpyHostToDevice);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    auto time = [&](const char *name, auto launch) {
        for (int i = 0; i < 5; i++) launch();
        hipDeviceSynchronize();
        hipEventRecord(e0);
        const int n = 40;
        for (int i = 0; i < n; i++) launch();
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        ms /= n;
        printf("{\"variant\": \"%s\", \"blocks_per_cu\": %d, \"ms\": %.4f, \"TBps\": %.3f}\n", name, bpc, ms, 2.0 * bytes / ms / 1e9);
    };
#define RUNG(R_, T_) time((T_) ? "2 generations, transposed gather, R=" #R_ : "2 generations, chunk gather, R=" #R_, [&] { hipLaunchKernelGGL((skeleton_gens<R_, 2, T_>), dim3(256 * bpc), dim3(256), 0, 0, x, y, idx, rows, pitch, 7u); })
    if (gens) {
        if (strcmp(form, "transposed")) { RUNG(15, false); RUNG(20, false); }
        if (strcmp(form, "chunk")) { RUNG(15, true); RUNG(20, true); }
        return 0;
    }
#define RUN(R_, G_) time((G_) ? "gather, R=" #R_ : "no gather, R=" #R_, [&] { hipLaunchKernelGGL((skeleton<3, R_, G_>), dim3(256 * bpc), dim3(256), 0, 0, x, y, idx, rows, pitch, 7u); })
    RUN(0, false);
    RUN(0, true);
    RUN(5, true);
    RUN(10, true);
    RUN(15, true);
    RUN(20, true);
    RUN(25, true);
    RUN(30, true);
    RUN(40, true);
#define RUNP(R_) time("gather + prefetch, R=" #R_, [&] { hipLaunchKernelGGL((skeleton_prefetch<3, R_>), dim3(256 * bpc), dim3(256), 0, 0, x, y, idx, rows, pitch, 7u); })
    RUNP(0);
    RUNP(10);
    RUNP(20);
    RUNP(25);
    return 0;
}
