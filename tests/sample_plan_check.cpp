// sample_plan_check.cpp -- the launch arithmetic of the core gather of the isolate samples (pansim_amd/csrc/sample_plan.h) held to
// its invariants on the host: a program of its own, built with the address and undefined-behaviour sanitizers by
// tests/test_isolate_samples.py.  For every (source pitch, rows, offset, end of the owned range, sites, forced form) it replays
// which thread of which workgroup owns which 16-byte chunk and which sites, exactly as core_gather_rows_kernel indexes them, and
// checks that every chunk of [off, own_end) and every site is owned once, and that the block, the grid and the LDS are within the
// limits of the device.
#include <cstdio>
#include <vector>

#include "../pansim_amd/csrc/sample_plan.h"

static int bad = 0;

static void fail(const char *what, uint32_t pitch_in, uint32_t n, uint32_t off, uint32_t own_end, uint64_t L, int form)
{
    printf("BAD %s: pitch_in %u n %u off %u own_end %u L %llu form %d\n", what, pitch_in, n, off, own_end, (unsigned long long)L, form);
    bad++;
}

static void check(int form, uint32_t pitch_in, uint32_t n, uint32_t off, uint32_t own_end, uint64_t L)
{
    const gather_plan g = core_gather_plan(form, pitch_in, n, off, own_end, L);
#define REQUIRE(c) do { if (!(c)) { fail(#c, pitch_in, n, off, own_end, L, form); return; } } while (0)
    REQUIRE(g.direct == core_gather_direct(form, pitch_in, n));
    REQUIRE(g.direct || pitch_in <= PS_GATHER_LDS_PITCH);
    REQUIRE(g.ch == 1 || g.ch == 2 || g.ch == PS_GATHER_MAX_CHUNKS);
    REQUIRE(!g.direct || g.ch == 1);
    REQUIRE(g.tx >= 1 && g.sy >= 1 && (uint64_t)g.tx * g.sy <= 1024);
    REQUIRE(g.lds == (g.direct ? 0u : g.sy * pitch_in) && g.lds <= 160u * 1024u);
    REQUIRE(g.tiles >= 1 && g.runs >= 1 && g.runs <= 65535u);
    REQUIRE(g.sites_per_wg >= g.sy && g.sites_per_wg % g.sy == 0);
    // the sites: run r takes [r per, min((r + 1) per, L))
    REQUIRE((uint64_t)g.runs * g.sites_per_wg >= L && (uint64_t)(g.runs - 1) * g.sites_per_wg < L);
    // the chunks: thread tx of tile t owns off / 16 + (t ch + k) TX + tx for k < ch, as the kernel computes them
    const uint64_t c0 = off / 16u, c_end = ((uint64_t)own_end + 15u) / 16u;
    REQUIRE(c_end - c0 <= (1u << 22));
    std::vector<uint8_t> owned(c_end - c0, 0);
    for (uint64_t t = 0; t < g.tiles; t++)
        for (uint32_t k = 0; k < g.ch; k++)
            for (uint32_t tx = 0; tx < g.tx; tx++) {
                const uint64_t c = c0 + (t * g.ch + k) * g.tx + tx;
                if (c >= c_end) continue;
                REQUIRE(owned[c - c0] == 0);
                owned[c - c0] = 1;
            }
    for (uint8_t o : owned) REQUIRE(o == 1);
    // no tile is empty
    REQUIRE(c0 + (uint64_t)(g.tiles - 1) * g.ch * g.tx < c_end);
#undef REQUIRE
}

int main()
{
    const uint32_t pops[] = { 1, 2, 7, 64, 65, 127, 128, 129, 300, 1000, 1024, 1030, 2049, 4096, 8192, 16385, 65408, 65536, 65537, 100000, 1u << 20 };
    const uint64_t sites[] = { 1, 2, 3, 130, 1001, 4096, 4097, 1200000, 1ull << 32 };
    unsigned long long plans = 0;
    for (uint32_t N : pops) {
        const uint32_t pitch_in = (N + 127u) / 128u * 128u;
        for (uint32_t total : pops) {
            const uint32_t pitch_out = (total + 127u) / 128u * 128u;
            // a part of n rows at every kind of offset inside an output row of `total` rows, with and without the pad
            const uint32_t offs[] = { 0, 1, 3, 15, 16, 17, total / 2, total - 1 };
            for (uint32_t off : offs) {
                if (off >= total) continue;
                const uint32_t ns[] = { 1, 3, 16, (total - off) / 2, total - off };
                for (uint32_t n : ns) {
                    if (n < 1 || off + n > total) continue;
                    for (int last = 0; last < 2; last++) {
                        if (last && off + n != total) continue;
                        const uint32_t own_end = last ? pitch_out : off + n;
                        for (uint64_t L : sites)
                            for (int form = 0; form < 3; form++) {
                                check(form, pitch_in, n, off, own_end, L);
                                plans++;
                            }
                    }
                }
            }
        }
    }
    // the switch itself: rows that do not fit are direct whatever is asked; else the key decides; else 48 n < pitch
    if (!core_gather_direct(1, 65664, 65537) || core_gather_direct(1, 1024, 1) || !core_gather_direct(2, 1024, 1024) || !core_gather_direct(0, 1024, 21)
        || core_gather_direct(0, 1024, 22)) {
        printf("BAD switch\n");
        bad++;
    }
    if (bad) return 1;
    printf("every plan holds (%llu plans)\n", plans);
    return 0;
}
