// Stand-alone check of the grouped GEMM's tile table (csrc/gemm_group.h): every (problem, m tile, n tile) of a launch is dealt to
// exactly one workgroup, exactly once, and nothing a workgroup is dealt lies outside its problem.  Built with
// -fsanitize=address,undefined and run by tests/test_group_table_host.py.
#include "gemm_group.h"

#include <cstdio>
#include <vector>

static int failures = 0;

static void check(const char* name, int n, const int* M, const int* N, const int* K, int BM, int BN, int max_grid) {
    const gemm::GroupTable t = gemm::group_build(n, M, N, K, BM, BN);
    const int grid = gemm::group_grid(t, max_grid);
    auto fail = [&](const char* what, long a, long b) {
        std::printf("FAIL %s: %s (%ld, %ld)\n", name, what, a, b);
        ++failures;
    };
    if (grid % 8 != 0 || grid > max_grid) fail("grid", grid, max_grid);
    // problems kept: those with tiles, most k-tiles first, the caller's index in src
    long want_tiles = 0;
    for (int i = 0; i < n; ++i) want_tiles += (long)((M[i] + BM - 1) / BM) * ((N[i] + BN - 1) / BN) * (K[i] >= 32);
    if (gemm::group_total_tiles(t) != want_tiles) fail("total tiles", gemm::group_total_tiles(t), want_tiles);
    std::vector<std::vector<int>> seen(gemm::GROUP_MAX);
    for (int i = 0; i < t.n; ++i) {
        if (i > 0 && t.p[i - 1].nk < t.p[i].nk) fail("order", t.p[i - 1].nk, t.p[i].nk);
        if (t.p[i].src < 0 || t.p[i].src >= n || t.p[i].nk != K[t.p[i].src] / 32) fail("src", i, t.p[i].src);
        seen[i].assign((size_t)t.p[i].tiles_m * t.p[i].tiles_n, 0);
    }
    long dealt = 0;
    for (int b = 0; b < grid; ++b) {
        const int mine = gemm::group_my_tiles(t, grid, b);
        int last_nk = 1 << 30;
        for (int i = 0; i < mine; ++i) {
            int p = -1, mt = -1, nt = -1;
            if (!gemm::group_tile(t, b & 7, (b >> 3) + i * (grid >> 3), &p, &mt, &nt)) {
                fail("tile past the queue", b, i);
                continue;
            }
            if (p < 0 || p >= t.n || mt < 0 || mt >= t.p[p].tiles_m || nt < 0 || nt >= t.p[p].tiles_n) {
                fail("tile outside its problem", b, i);
                continue;
            }
            if (t.p[p].nk > last_nk) fail("a longer tile after a shorter one", b, i);
            last_nk = t.p[p].nk;
            ++seen[p][(size_t)mt * t.p[p].tiles_n + nt];
            ++dealt;
        }
    }
    if (dealt != want_tiles) fail("tiles dealt", dealt, want_tiles);
    for (int i = 0; i < t.n; ++i)
        for (size_t k = 0; k < seen[i].size(); ++k)
            if (seen[i][k] != 1) fail("tile not dealt exactly once", i, (long)k);
    if (want_tiles == 0 && grid != 0) fail("empty launch", grid, 0);
    std::printf("%-28s problems %d tiles %ld grid %d\n", name, t.n, want_tiles, grid);
}

int main() {
    {   // the benchmark's filters: all-pass (K = 2 x 256), source, noise
        const int N[3] = {256, 512, 256}, K[3] = {512, 512, 256};
        for (int rows : {11008, 8256, 8192 + 37, 8192}) {
            const int M[3] = {rows, rows, rows};
            check("combsub 64x64", 3, M, N, K, 64, 64, 768);
            check("combsub 128x64", 3, M, N, K, 128, 64, 512);
        }
    }
    {   // two problems (the sinusoid synthesiser's filters), the short one listed first
        const int M[2] = {8256, 8256}, N[2] = {256, 256}, K[2] = {256, 512};
        check("sins", 2, M, N, K, 64, 64, 768);
    }
    {
        const int M[1] = {8229}, N[1] = {512}, K[1] = {512};
        check("one problem", 1, M, N, K, 64, 64, 768);
    }
    {
        const int M[3] = {0, 0, 0}, N[3] = {256, 512, 256}, K[3] = {512, 512, 256};
        check("zero rows", 3, M, N, K, 64, 64, 768);
    }
    {   // one problem without rows among two with
        const int M[3] = {100, 0, 100}, N[3] = {256, 512, 256}, K[3] = {256, 512, 512};
        check("one empty problem", 3, M, N, K, 64, 64, 768);
    }
    {   // fewer tiles than workgroups, fewer than XCDs, a single tile
        const int N[3] = {256, 512, 256}, K[3] = {512, 512, 256};
        for (int rows : {1, 63, 64, 65, 300, 700}) {
            const int M[3] = {rows, rows, rows};
            check("few tiles", 3, M, N, K, 64, 64, 768);
        }
        const int M1[1] = {5}, N1[1] = {7}, K1[1] = {32};
        check("single tile", 1, M1, N1, K1, 64, 64, 768);
    }
    {   // every row-tile count modulo 8, odd column counts, a small grid (many rounds)
        for (int tm = 1; tm <= 40; ++tm) {
            const int M[3] = {64 * tm - 3, 64 * tm - 3, 64 * tm - 3}, N[3] = {129, 65, 511}, K[3] = {256, 512, 256};
            check("sweep", 3, M, N, K, 64, 64, 64);
        }
    }
    if (failures) std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
