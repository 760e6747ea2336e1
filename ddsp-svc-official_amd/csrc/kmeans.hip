// a18: k-means reduction of a unit index (`infer_offline.UnitIndex.reduce`): a voice's hundreds of thousands of stored units
// become some 10 000 centres before the index is served.  THE RULE is stated in include/ddsp_amd.h at ddsp_units_kmeans_assign
// and in numpy fp64 and Python integers in tests/kmeans_cases.py.  One Lloyd iteration is ddsp_units_index_norms (retrieve.hip),
// then the two entry points of this file; nothing here allocates, synchronises or reads back.
//
// ASSIGN.  The product is N x K x C with an arg-min epilogue: queries are plentiful and k is 1, which is not the shape the
// search of retrieve.hip serves.  A workgroup (4 waves) owns a tile of 128 entries and marches over ALL centres in stages of
// 128 centres; a stage streams through the LDS in slices of 32 channels (coalesced 16-byte loads, rows padded to 36 floats as
// in the search; the next slice is fetched into registers while the products of this one run).  Wave (we, wc) forms entries
// we * 64 .. + 64 against centres wc * 64 .. + 64 as 2 x 2 tiles of v_mfma_f32_32x32x2_f32 - four independent accumulators,
// 16 FLOP per byte read from the LDS - with the centres as A and the entries as B, so a lane's 16 accumulators of a tile are 16
// centres of ONE entry (column = lane & 31) and the running (t, id) minimum of an entry stays in two registers per entry tile.
// The k order of the products is the search's fixed permutation of the channels, the same for both operands.  Four lanes see
// an entry (2 centre halves x 2 lane halves); at the end thread e merges the four through the LDS, compares with the previous
// assignment, stores one int32, and the workgroup adds its moved count with one atomic.
// UPDATE.  Sums are exact: q = rint(x * 2^shift) as int64, added with 64-bit integer atomics, so the order of the additions
// does not reach the bits.  A group of C / 4 threads walks 32 neighbouring entries, keeps the sum of a run of equal assignment
// in registers and adds it once when the assignment changes.  Finalise divides once in fp64.
#include "common.h"
#include "unit_order.h"

#include <climits>
#include <cmath>

namespace {

constexpr int KM_ET = 128;           // entries of a workgroup's tile: 64 per wave row
constexpr int KM_CT = 128;           // centres of a stage: 64 per wave column
constexpr int KM_KC = 32;            // channels of a slice
constexpr int KM_LD = KM_KC + 4;     // floats of an LDS row
constexpr int KM_THREADS = 256;
constexpr int KM_RUN = 32;           // entries a group of the update walks

// (two waves per SIMD: 234 registers, none spilled, no scratch; without the bound the compiler takes one wave)
__global__ void __launch_bounds__(KM_THREADS, 2) kmeans_assign_kernel(const float* __restrict__ vec, int64_t N, int C,
                                                                      const float* __restrict__ cen, const float* __restrict__ cnrm,
                                                                      int K, int32_t* __restrict__ assign, int32_t* __restrict__ moved) {
    __shared__ float xs[KM_ET * KM_LD];
    __shared__ float cs[KM_CT * KM_LD];
    __shared__ float ns[KM_CT];                                            // the stage's norms
    __shared__ float mt[4 * KM_ET];                                        // the four minima of every entry, for the merge
    __shared__ int mi[4 * KM_ET];
    __shared__ int nmoved;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int we = wave >> 1, wc = wave & 1;
    const int64_t e0 = (int64_t)blockIdx.x * KM_ET;
    const int lq = tid >> 3, lc = 4 * (tid & 7);                           // the staging loads: row of the slice, channel in it
    if (tid == 0) nmoved = 0;
    float best_t[2] = {INFINITY, INFINITY};
    int best_j[2] = {INT_MAX, INT_MAX};
    f32x4 xv[4], cv[4];
    float nv = 0.f;
    // slice (j0, c0) into registers: rows p * 32 + lq of both tiles, 16 bytes each; what lies outside is zero.  Both tiles are
    // addressed as a workgroup-uniform base plus ONE 32-bit offset per row, (p * 32 + lq) * C + c < 2^17, the same for the
    // entries and the centres: no per-row 64-bit pointers are kept across the stage loop
    const float* __restrict__ xbase = vec + e0 * C;
    const int nx = (int)(N - e0 < KM_ET ? N - e0 : KM_ET);                 // rows of this tile that exist
    auto fetch = [&](int64_t j0, int c0) {
        const int c = c0 + lc;
        const float* __restrict__ cbase = cen + j0 * C;
        const int nk = (int)(K - j0 < KM_CT ? K - j0 : KM_CT);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int row = p * 32 + lq;
            const int o = row * C + c;
            xv[p] = cv[p] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (row < nx && c < C) xv[p] = *(const f32x4*)(xbase + o);
            if (row < nk && c < C) cv[p] = *(const f32x4*)(cbase + o);
        }
        if (c0 == 0 && tid < KM_CT) nv = tid < nk ? cnrm[j0 + tid] : 0.f;
    };
    fetch(0, 0);
    for (int64_t j0 = 0; j0 < K; j0 += KM_CT) {                           // (64 bits: j0 + 128 may pass 2^31)
        f32x16 acc[2][2];                                                  // [centre tile][entry tile]
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
        for (int c0 = 0; c0 < C; c0 += KM_KC) {
            __syncthreads();                                               // the slice before this one has been read
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                *(f32x4*)&xs[(p * 32 + lq) * KM_LD + lc] = xv[p];
                *(f32x4*)&cs[(p * 32 + lq) * KM_LD + lc] = cv[p];
            }
            if (c0 == 0 && tid < KM_CT) ns[tid] = nv;                      // (read only after this stage's last slice)
            __syncthreads();
            if (c0 + KM_KC < C) fetch(j0, c0 + KM_KC);                     // the next slice, in flight under the products
            else if (j0 + KM_CT < K) fetch(j0 + KM_CT, 0);
#pragma unroll 2                                                           // (unrolled fully the kernel spills 14 registers)
            for (int kk = 0; kk < KM_KC; kk += 8) {
                f32x4 a[2], b[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    a[h] = *(const f32x4*)&cs[(wc * 64 + h * 32 + lr) * KM_LD + kk + 4 * lh];
                    b[h] = *(const f32x4*)&xs[(we * 64 + h * 32 + lr) * KM_LD + kk + 4 * lh];
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                        for (int et = 0; et < 2; ++et)
                            acc[ct][et] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ct][s], b[et][s], acc[ct][et], 0, 0, 0);
            }
        }
        // C/D map of the 32x32 MFMA: column (the entry) = lane & 31, row (the centre) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        // a lane meets its centres in ascending id, tile by tile and stage by stage
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jl = wc * 64 + ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (j0 + jl < K) {
                    const int j = (int)(j0 + jl);
                    const float n = ns[jl];
#pragma unroll
                    for (int et = 0; et < 2; ++et) {
                        const float t = n - 2.f * acc[ct][et][r];
                        if (before(t, j, best_t[et], best_j[et])) {        // (false for a NaN score: it is never selected)
                            best_t[et] = t;
                            best_j[et] = j;
                        }
                    }
                }
            }
    }
#pragma unroll
    for (int et = 0; et < 2; ++et) {
        const int e = we * 64 + et * 32 + lr;
        mt[(wc * 2 + lh) * KM_ET + e] = best_t[et];
        mi[(wc * 2 + lh) * KM_ET + e] = best_j[et];
    }
    __syncthreads();
    if (tid < KM_ET) {
        bool diff = false;
        if (e0 + tid < N) {
            float bt = mt[tid];
            int bj = mi[tid];
#pragma unroll
            for (int l = 1; l < 4; ++l) {
                const float t = mt[l * KM_ET + tid];
                const int j = mi[l * KM_ET + tid];
                if (before(t, j, bt, bj)) {
                    bt = t;
                    bj = j;
                }
            }
            if (bj >= K) bj = -1;                                          // no score was a number: the entry belongs to no centre
            diff = assign[e0 + tid] != bj;
            assign[e0 + tid] = bj;
        }
        const int n = __popcll(__ballot(diff));
        if (lane == 0 && n) atomicAdd(&nmoved, n);
    }
    __syncthreads();
    if (tid == 0 && nmoved) atomicAdd(moved, nmoved);
}

// Threads q + g * C4 of a workgroup (q < C4 = C / 4) form group g; it walks entries [first, first + KM_RUN) and owns channels
// 4 q .. 4 q + 3 of each.  A run of equal assignment is summed in registers and leaves with four atomics (and one for the count).
__global__ void __launch_bounds__(KM_THREADS) kmeans_accumulate_kernel(const float* __restrict__ vec, int64_t N, int C,
                                                                       const int32_t* __restrict__ assign, int K, int shift,
                                                                       unsigned long long* __restrict__ sum, int32_t* __restrict__ count) {
    const int C4 = C >> 2, groups = KM_THREADS / C4;
    const int g = threadIdx.x / C4, q = threadIdx.x % C4;
    if (g >= groups) return;
    const int64_t first = ((int64_t)blockIdx.x * groups + g) * KM_RUN;
    const int64_t last = first + KM_RUN < N ? first + KM_RUN : N;
    long long acc[4] = {0, 0, 0, 0};
    int cur = -1, len = 0;
    auto flush = [&]() {
        if (cur >= 0 && cur < K) {                                         // tested before it forms an address
            unsigned long long* __restrict__ s = sum + ((int64_t)cur * C + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) atomicAdd(s + i, (unsigned long long)acc[i]);
            if (q == 0) atomicAdd(count + cur, len);
        }
        acc[0] = acc[1] = acc[2] = acc[3] = 0;
        len = 0;
    };
    for (int64_t e = first; e < last; ++e) {
        const int a = assign[e];
        if (a != cur) {
            flush();
            cur = a;
        }
        const f32x4 x = *(const f32x4*)(vec + e * C + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += __double2ll_rn(ldexp((double)x[i], shift));
        ++len;
    }
    flush();
}

__global__ void __launch_bounds__(KM_THREADS) kmeans_finalise_kernel(float* __restrict__ cen, int64_t KC, int C, int shift,
                                                                     const long long* __restrict__ sum, const int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    if (i >= KC) return;
    const int n = count[i / C];
    if (n > 0) cen[i] = (float)ldexp((double)sum[i] / (double)n, -shift);  // an empty centre keeps its bits
}

bool kmeans_shape_ok(int64_t N, int64_t C, int64_t K) {
    return N >= 1 && N < (1ll << 31) && K >= 1 && K <= N && C >= 4 && C <= 1024 && C % 4 == 0;
}

}  // namespace

extern "C" int ddsp_units_kmeans_assign(ddsp_ctx* ctx, void* stream, const float* vec, int64_t N, int64_t C, const float* cen,
                                        const float* cnrm, int64_t K, int32_t* assign, int32_t* moved) {
    DDSP_REQUIRE(ctx, ctx && vec && cen && cnrm && assign && moved, "ddsp_units_kmeans_assign: null argument");
    DDSP_REQUIRE(ctx, kmeans_shape_ok(N, C, K), "ddsp_units_kmeans_assign: bad shape (1 <= K <= N < 2^31, C a multiple of 4 in 4..1024)");
    DDSP_REQUIRE(ctx, (((uintptr_t)vec | (uintptr_t)cen) & 15) == 0, "ddsp_units_kmeans_assign: vec and cen must be 16-byte aligned");
    DDSP_ENTER_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)ceil_div64(N, KM_ET)), dim3(KM_THREADS), 0, st, vec, N, (int)C, cen, cnrm,
                       (int)K, assign, moved);
    ddsp_prof_end(ctx, st, 2.0 * (double)N * (double)K * (double)C,
                  4.0 * ((double)N * (double)(C + 2) + (double)K * (double)(C + 1) * (double)ceil_div64(N, KM_ET)));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_units_kmeans_update(ddsp_ctx* ctx, void* stream, const float* vec, int64_t N, int64_t C, const int32_t* assign,
                                        int64_t K, int shift, float* cen, int32_t* count, void* workspace, int64_t workspace_bytes) {
    DDSP_REQUIRE(ctx, ctx && vec && assign && cen && count && workspace, "ddsp_units_kmeans_update: null argument");
    DDSP_REQUIRE(ctx, kmeans_shape_ok(N, C, K), "ddsp_units_kmeans_update: bad shape (1 <= K <= N < 2^31, C a multiple of 4 in 4..1024)");
    DDSP_REQUIRE(ctx, (((uintptr_t)vec | (uintptr_t)cen) & 15) == 0, "ddsp_units_kmeans_update: vec and cen must be 16-byte aligned");
    DDSP_REQUIRE(ctx, shift >= -97 && shift <= 210, "ddsp_units_kmeans_update: shift must be 62 - E - L of the rule, in -97..210");
    DDSP_REQUIRE(ctx, workspace_bytes >= K * C * 8 && ((uintptr_t)workspace & 15) == 0,
                 "ddsp_units_kmeans_update: the workspace must hold K * C * 8 bytes and be 16-byte aligned");
    DDSP_ENTER_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    DDSP_HIP(ctx, hipMemsetAsync(workspace, 0, (size_t)(K * C * 8), st));
    DDSP_HIP(ctx, hipMemsetAsync(count, 0, (size_t)(K * 4), st));
    const int64_t groups = KM_THREADS / (C / 4);
    hipLaunchKernelGGL(kmeans_accumulate_kernel, dim3((unsigned)ceil_div64(N, groups * KM_RUN)), dim3(KM_THREADS), 0, st, vec, N, (int)C,
                       assign, (int)K, shift, (unsigned long long*)workspace, count);
    hipLaunchKernelGGL(kmeans_finalise_kernel, dim3((unsigned)ceil_div64(K * C, KM_THREADS)), dim3(KM_THREADS), 0, st, cen, K * C, (int)C,
                       shift, (const long long*)workspace, count);
    ddsp_prof_end(ctx, st, 2.0 * (double)N * (double)C, 4.0 * (double)N * (double)(C + 1) + 20.0 * (double)K * (double)C);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
