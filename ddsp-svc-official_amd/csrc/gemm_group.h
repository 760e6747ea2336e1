// Tile table of a grouped GEMM launch: up to GROUP_MAX problems (own operands, own k-tile count, own epilogue) walked by ONE
// persistent kernel (gemm_f32.h, kernel_dma_group).  Plain C++ with no HIP in it: the host builds the table, the kernel and a
// stand-alone host program (tests/group_table_host.cpp) read it through the same functions.
//
// Order.  Workgroup b runs on XCD b & 7 (gridDim.x is a multiple of 8).  Each XCD keeps, per problem, the queue that the
// XCD-aware order of kernel_dma gives it: the row blocks x, x + 8, ... with ALL their column tiles (the A rows of a row block
// are fetched into one L2), then its share of the leftover tiles_m % 8 row blocks, dealt round-robin.  The XCD's queue of the
// launch is these per-problem queues one after the other, problems with the most k-tiles first; workgroup (x, j) takes entries
// j, j + gridDim.x / 8, ... of it.  Long tiles are so dealt first, one per workgroup, and the short ones fill the tail.
#pragma once

#if defined(__HIPCC__)
#define GEMM_GROUP_HD __host__ __device__ inline
#else
#define GEMM_GROUP_HD inline
#endif

namespace gemm {

constexpr int GROUP_MAX = 3;

struct GroupProblem {
    int tiles_m, tiles_n;   // tiles of BM rows / BN columns
    int nk;                 // k-tiles (of 32) per tile
    int src;                // index of this problem in the caller's list (the table is sorted by nk)
};

struct GroupTable {
    int n;                  // problems, in dealing order
    GroupProblem p[GROUP_MAX];
};

// entries of problem i in XCD x's queue
GEMM_GROUP_HD int group_queue_len(const GroupProblem& p, int x) {
    const int left = (p.tiles_m % 8) * p.tiles_n;
    return (p.tiles_m / 8) * p.tiles_n + (left > x ? (left - x + 7) / 8 : 0);
}

GEMM_GROUP_HD int group_queue_len(const GroupTable& t, int x) {
    int q = 0;
    for (int i = 0; i < t.n; ++i) q += group_queue_len(t.p[i], x);
    return q;
}

// entry q of XCD x's queue -> (problem in dealing order, m tile, n tile); false past the end of the queue
GEMM_GROUP_HD bool group_tile(const GroupTable& t, int x, int q, int* prob, int* mt, int* nt) {
    for (int i = 0; i < t.n; ++i) {
        const GroupProblem& p = t.p[i];
        const int len = group_queue_len(p, x);
        if (q >= len) {
            q -= len;
            continue;
        }
        const int own = (p.tiles_m / 8) * p.tiles_n;
        *prob = i;
        if (q < own) {
            *mt = x + 8 * (q / p.tiles_n);
            *nt = q % p.tiles_n;
        } else {
            const int u = (q - own) * 8 + x;
            *mt = (p.tiles_m / 8) * 8 + u / p.tiles_n;
            *nt = u % p.tiles_n;
        }
        return true;
    }
    return false;
}

// tiles of workgroup b in a launch of `grid` workgroups (grid % 8 == 0): entries b / 8 + i * (grid / 8), i < count, of XCD
// b & 7's queue
GEMM_GROUP_HD int group_my_tiles(const GroupTable& t, int grid, int b) {
    const int len = group_queue_len(t, b & 7), j = b >> 3, stride = grid >> 3;
    return j < len ? (len - j + stride - 1) / stride : 0;
}

// Table of `n` problems of M[i] rows, N[i] columns and K[i] (a multiple of 32) on BM x BN tiles: most k-tiles first, equal
// counts in the caller's order.  Problems without tiles (no rows, no columns) are left out.
inline GroupTable group_build(int n, const int* M, const int* N, const int* K, int BM, int BN) {
    GroupTable t;
    t.n = 0;
    for (int i = 0; i < GROUP_MAX; ++i) t.p[i] = GroupProblem{0, 0, 0, 0};
    for (int i = 0; i < n && i < GROUP_MAX; ++i) {
        GroupProblem p{(M[i] + BM - 1) / BM, (N[i] + BN - 1) / BN, K[i] / 32, i};
        if (p.tiles_m <= 0 || p.tiles_n <= 0 || p.nk <= 0) continue;
        int at = t.n++;
        for (; at > 0 && t.p[at - 1].nk < p.nk; --at) t.p[at] = t.p[at - 1];
        t.p[at] = p;
    }
    return t;
}

inline long group_total_tiles(const GroupTable& t) {
    long s = 0;
    for (int i = 0; i < t.n; ++i) s += (long)t.p[i].tiles_m * t.p[i].tiles_n;
    return s;
}

// workgroups to launch: at most max_grid (a multiple of 8), no more than the longest XCD queue can feed
inline int group_grid(const GroupTable& t, int max_grid) {
    int longest = 0;
    for (int x = 0; x < 8; ++x) {
        const int len = group_queue_len(t, x);
        longest = len > longest ? len : longest;
    }
    const int grid = 8 * longest;
    return grid < max_grid ? grid : max_grid;
}

}  // namespace gemm
