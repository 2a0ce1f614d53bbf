// The scratch layouts of the device read-outs (scratch_layout of pansim_amd/csrc/readout_common.h, regions added in the order of
// cluster_scratch, tree_scratch_get, knn_scratch_get, gen_scratch_get and ld_scratch_get) against the offset arithmetic these
// functions were first written with, which this program keeps written out: every region has to keep its size, alignment and
// order, since the kernels see the same addresses modulo the base.  Host only, no device:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o readout_layout_check tests/readout_layout_check.cpp
// (tests/test_readout_layout.py does both)
//   ./readout_layout_check        (prints every offset and total; exit status 1 on a mismatch)
#define PS_READOUT_LAYOUT_ONLY
#include "../pansim_amd/csrc/readout_common.h"

#include <cstdio>
#include <initializer_list>
#include <vector>

static int bad = 0;

static void row(const char *what, uint64_t n, const std::vector<uint64_t> &got, const std::vector<uint64_t> &want)
{
    printf("%-22s N=%-5llu", what, (unsigned long long)n);
    for (uint64_t o : got) printf(" %llu", (unsigned long long)o);
    const bool ok = got == want;
    printf(ok ? "\n" : "   MISMATCH, expected");
    if (!ok) {
        for (uint64_t o : want) printf(" %llu", (unsigned long long)o);
        printf("\n");
        bad++;
    }
}

int main()
{
    const uint64_t CL_WORDS = 2, TR_ARRAYS = 12, CK_WORDS = 2, LD_WORDS = 8, LD_MAX_LAGS = 32;     // (as the kernel headers have them)
    for (uint64_t N : { 1ull, 2ull, 63ull, 64ull, 65ull, 1025ull }) {
        {   // strain clusters: words | changed | labels | adjacency bit matrix -> offsets, total
            scratch_layout lay;
            std::vector<uint64_t> got = { lay.add(CL_WORDS * 8, 8), lay.add(8, 8), lay.add(N * 4, 8), lay.add(N * ((N + 63) / 64) * 8, 8) };
            got.push_back(lay.bytes);
            const uint64_t W = (N + 63) / 64, head = (CL_WORDS + 1) * 8, lab = (N * 4 + 7) & ~7ull;
            row("strain clusters", N, got, { 0, CL_WORDS * 8, head, head + lab, head + lab + N * W * 8 });
        }
        for (int acc = 0; acc < 2; acc++) {   // linkage tree: count | 12 arrays | matrix
            scratch_layout lay;
            const uint64_t ldm = (N + 63) & ~63ull;
            std::vector<uint64_t> got = { lay.add(16, 16) };
            for (uint64_t k = 0; k < TR_ARRAYS; k++) got.push_back(lay.add(N * 4, 16));
            got.push_back(lay.add(N * ldm * (acc ? 2 : 4), 16));
            got.push_back(lay.bytes);
            const uint64_t lab = (N * 4 + 15) & ~15ull, head = 16 + TR_ARRAYS * lab;
            std::vector<uint64_t> want = { 0 };
            for (uint64_t k = 0; k < TR_ARRAYS; k++) want.push_back(16 + k * lab);
            want.push_back(head);
            want.push_back(head + N * ldm * (acc ? 2 : 4));
            row(acc ? "linkage tree (acc)" : "linkage tree (core)", N, got, want);
        }
        for (int acc = 0; acc < 2; acc++)     // nearest neighbours: out_row | j | num | (den)
            for (uint64_t k : { 1ull, 8ull, 128ull }) {
                scratch_layout lay;
                std::vector<uint64_t> got = { lay.add(N * 4, 16), lay.add(N * k * 4, 16), lay.add(N * k * 4, 16) };
                if (acc) got.push_back(lay.add(N * k * 4, 16));
                got.push_back(lay.bytes);
                const uint64_t head = (N * 4 + 15) & ~15ull, list = (N * k * 4 + 15) & ~15ull;
                std::vector<uint64_t> want = { 0, head, head + list };
                if (acc) want.push_back(head + 2 * list);
                want.push_back(head + (acc ? 3 : 2) * list);
                row(acc ? "neighbours (acc)" : "neighbours (core)", N, got, want);
            }
        for (uint64_t levels : { 1ull, 11ull }) {   // genealogy: table | the clock's words, sums and bins
            const uint64_t nt = 33, nbins = nt * 64, extra = levels == 1 ? 0 : (CK_WORDS + 2 * nt + nbins) * 8;
            scratch_layout lay;
            std::vector<uint64_t> got = { lay.add(levels * N * 4, 16), lay.add(extra, 1) };
            got.push_back(lay.bytes);
            const uint64_t tab = (levels * N * 4 + 15) & ~15ull;
            row(levels == 1 ? "genealogy (comb)" : "genealogy (clock)", N, got, { 0, tab, tab + extra });
        }
        for (uint64_t K : { 1ull, 2ull })           // linkage disequilibrium of M = N loci among N individuals, 64 x 1 bins
            for (int first = 0; first < 2; first++) {
                const uint64_t M = N, nbins = 64;
                const uint64_t Mpad = ((M > 1 ? M : 1) + 127) & ~127ull, WP = ((N + 31) / 32 + 7) & ~7ull, ldi = Mpad + 128;
                uint64_t band = ((64ull << 20) / ldi) & ~255ull;
                band = band < 256 ? 256 : band;
                band = band < Mpad ? band : Mpad;
                const uint64_t n_words = (LD_WORDS + LD_MAX_LAGS + nbins + 1) & ~1ull, row_words = Mpad * WP;
                scratch_layout lay;
                std::vector<uint64_t> got;
                const uint64_t o_words = lay.add(first ? n_words * 8 : 0, 8);      // (the three of part 0 are empty on the others)
                if (first) got.push_back(o_words);
                for (int k = 0; k < 3; k++) got.push_back(lay.add(Mpad * 4, 4));
                got.push_back(lay.add(row_words * 4, 4));
                const uint64_t o_land = lay.add(first && K > 1 ? row_words * 4 : 0, 4), o_in = lay.add(first ? band * ldi * 2 : 0, 2);
                if (first) got.insert(got.end(), { o_land, o_in });
                got.push_back(lay.bytes);
                // part 0: words | sel | cnt | idx | rows | landing rows | one band of n11; the others: sel | cnt | rows
                uint64_t bytes = (3 * Mpad + row_words) * 4;
                if (first) bytes += n_words * 8 + (K > 1 ? row_words * 4 : 0) + band * ldi * 2;
                const uint64_t base = first ? 2 * n_words * 4 : 0;
                std::vector<uint64_t> want;
                if (first) want.push_back(0);
                for (uint64_t k = 0; k < 4; k++) want.push_back(base + k * Mpad * 4);
                if (first) {
                    const uint64_t land = base + (3 * Mpad + row_words) * 4;
                    want.push_back(land);
                    want.push_back(land + (K > 1 ? row_words * 4 : 0));
                }
                want.push_back(bytes);
                row(first ? (K > 1 ? "ld (part 0 of 2)" : "ld (one part)") : "ld (another part)", N, got, want);
            }
    }
    printf(bad ? "%d layouts differ\n" : "every layout matches\n", bad);
    return bad ? 1 : 0;
}
