// a17: unit retrieval (`infer_offline.UnitIndexBank`, offline jobs with an index, realtime.StreamBank(indices=...)): every
// frame's unit vector is blended with a weighted mean of its nearest stored units of a voice's index, in place, between the
// units encoder and the synthesiser.  Two launches, no allocation, no synchronisation: graph-capturable.
//
// THE RULE (include/ddsp_amd.h at ddsp_units_retrieve states it too; tests/retrieval_cases.py is the same in numpy fp64).
// A bank holds X indices in one arena: off (X + 1) int64 row offsets, vec (N_total, C) fp32, nrm (N_total) fp32 with
// nrm[i] = sum_c vec[i][c]^2 (ddsp_units_index_norms).  Row b has the setting j = owner[b] of J (b itself without a table;
// outside [0, J): a padding row, none): it names index index_of_row[j] (outside [0, X): none) and a ratio r = ratio_of_row[j].
// For a frame x of a row with index x_i of N entries, k_eff = min(k, N):
//     t_i   = nrm[i] - 2 * <x, vec[i]>                       (ranks as the squared distance does)
//     the k_eff entries with the smallest (t, id) are selected, in that order
//     s_j   = sum_c (x[c] - vec[j][c])^2                     (recomputed directly in fp32, not derived from t)
//     w_j   = 1 / max(s_j, 1e-12)^2, normalised to sum 1
//     out   = x + r * (sum_j w_j vec[j] - x)
// Rows without an index, rows with r == 0 and frames at or past a row's count keep their bits: they are never stored.  A row
// that names an index with r not finite or outside [0, 1] keeps its bits too and raises the device error word.  An index id,
// the offsets behind it and every entry id are tested before they form an address.
//
// SEARCH.  A workgroup (4 waves) takes one tile of 32 query frames of one row and one CHUNK of the row's index; the chunk
// count is the grid's y extent, chosen on the host from N_max and the CU count so that one 75-frame row still covers the
// device, and the chunk length follows in the kernel from the row's own N.  The chunk streams through the LDS in stages of 128
// entries x 32 channels (coalesced 16-byte loads, rows padded to 36 floats), the queries' slice beside it.  Scores come from
// the matrix pipe in fp32 - v_mfma_f32_32x32x2_f32, entries as A and queries as B, so a lane's 16 accumulators are 16 entries
// of ONE query (column = lane & 31) - and need no trip through the LDS: each lane keeps a running top-k by (t, id) of what it
// sees, as a sorted column of the workgroup's LDS list (slot-major: conflict-free), compared first against the list's worst
// in a register.  Eight lanes see a query (4 waves x 2 lane halves); thread q merges their lists at the end and writes k
// candidates (t, id) per (query, chunk) to the caller's workspace.  The k order of the products is a fixed permutation of the
// channels, the same for both operands.
// MERGE AND BLEND.  One wave per query: k rounds of "the smallest (t, id) above the last one" over the chunks' candidates
// (ids are unique, so the order is total), then the k vectors are gathered with 16-byte loads twice - once for s_j, once for
// the weighted mean - and out, nn_id and nn_dist are stored.
#include "common.h"
#include "unit_order.h"

#include <cfloat>
#include <climits>
#include <cmath>

namespace {

constexpr int RT_QT = 32;            // queries of a tile
constexpr int RT_ET = 128;           // entries of a stage: 32 per wave
constexpr int RT_KC = 32;            // channels of a slice
constexpr int RT_LD = RT_KC + 4;     // floats of an LDS row
constexpr int RT_KMAX = 16;
constexpr int RT_THREADS = 256;
constexpr int RT_MAX_CHUNKS = 1024;

// The index of a row and whether the row is served: tested in the same way by both kernels.
struct RowIndex {
    bool on;
    int64_t base, n;
    float r;
};

__device__ __forceinline__ RowIndex retrieve_row(int64_t row, const int32_t* __restrict__ owner, int64_t J,
                                                 const int32_t* __restrict__ index_of_row, const float* __restrict__ ratio_of_row,
                                                 int64_t X, const int64_t* __restrict__ off, int64_t N_total, bool& bad) {
    RowIndex ri = {false, 0, 0, 0.f};
    bad = false;
    const int64_t j = owner ? (int64_t)owner[row] : row;
    if (j < 0 || j >= J) return ri;                                        // a padding row of a row table: it has no setting
    row = j;
    const int64_t x = (int64_t)index_of_row[row];
    if (x < 0 || x >= X) return ri;                                        // tested before any address is formed
    const int64_t a = off[x], b = off[x + 1];
    if (!(a >= 0 && a < b && b <= N_total)) return ri;                     // (a broken arena serves nobody)
    const float r = ratio_of_row[row];
    if (!(r >= 0.f && r <= 1.f)) {
        bad = true;
        return ri;
    }
    if (r == 0.f) return ri;
    ri.on = true;
    ri.base = a;
    ri.n = b - a;
    ri.r = r;
    return ri;
}

__global__ void __launch_bounds__(RT_THREADS) retrieve_search_kernel(
    const float* __restrict__ units, int Fr, int C, int qtiles, const int32_t* __restrict__ n_frames,
    const int32_t* __restrict__ owner, int64_t J, const int32_t* __restrict__ index_of_row,
    const float* __restrict__ ratio_of_row, int64_t X, const int64_t* __restrict__ off,
    int64_t N_total, const float* __restrict__ vec, const float* __restrict__ nrm, int k, float* __restrict__ ws_t,
    int32_t* __restrict__ ws_id) {
    __shared__ float qs[RT_QT * RT_LD];
    __shared__ float es[RT_ET * RT_LD];
    extern __shared__ float lists[];                                       // k x 256 scores, then k x 256 ids
    float* lt = lists;
    int* li = (int*)(lists + (size_t)k * RT_THREADS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int64_t row = blockIdx.x / qtiles;
    const int q0 = (int)(blockIdx.x % qtiles) * RT_QT;
    const int chunk = blockIdx.y, nchunk = gridDim.y;
    bool bad;
    const RowIndex ri = retrieve_row(row, owner, J, index_of_row, ratio_of_row, X, off, N_total, bad);
    if (!ri.on) return;                                                    // (uniform over the workgroup, like the next)
    const int nf = ddsp_row_frames(n_frames, row, Fr);
    if (q0 >= nf) return;
    const int64_t clen = ((ri.n + nchunk - 1) / nchunk + RT_ET - 1) / RT_ET * RT_ET;
    const int64_t e0 = (int64_t)chunk * clen;
    const int64_t e1 = e0 + clen < ri.n ? e0 + clen : ri.n;                // (an empty chunk: e1 <= e0, only padding is written)
    for (int j = 0; j < k; ++j) {
        lt[j * RT_THREADS + tid] = INFINITY;
        li[j * RT_THREADS + tid] = INT_MAX;
    }
    float worst_t = INFINITY;
    int worst_i = INT_MAX;
    const bool mine = q0 + lr < nf;                                        // this lane's query exists
    const int lq = tid >> 3, lc = 4 * (tid & 7);                           // the staging loads: row of the slice, channel in it
    const float* __restrict__ xrow = units + ((int64_t)row * Fr + q0 + lq) * C;
    const float* __restrict__ vbase = vec + ri.base * C;
    for (int64_t s0 = e0; s0 < e1; s0 += RT_ET) {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < C; c0 += RT_KC) {
            const int c = c0 + lc;
            f32x4 qv = {0.f, 0.f, 0.f, 0.f}, ev[4];
            if (q0 + lq < nf && c < C) qv = *(const f32x4*)(xrow + c);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int64_t e = s0 + p * 32 + lq;
                ev[p] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (e < e1 && c < C) ev[p] = *(const f32x4*)(vbase + e * C + c);
            }
            __syncthreads();                                               // the slice before this one has been read
            *(f32x4*)&qs[lq * RT_LD + lc] = qv;
#pragma unroll
            for (int p = 0; p < 4; ++p) *(f32x4*)&es[(p * 32 + lq) * RT_LD + lc] = ev[p];
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < RT_KC; kk += 8) {
                const f32x4 a = *(const f32x4*)&es[(wave * 32 + lr) * RT_LD + kk + 4 * lh];
                const f32x4 b = *(const f32x4*)&qs[lr * RT_LD + kk + 4 * lh];
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
            }
        }
        // C/D map of the 32x32 MFMA: column (the query) = lane & 31, row (the entry) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t e = s0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (mine && e < e1) {
                const float t = nrm[ri.base + e] - 2.f * acc[r];
                const int id = (int)e;
                if (before(t, id, worst_t, worst_i)) {                     // (false for a NaN score: it is never selected)
                    int pos = k - 1;
                    while (pos > 0) {
                        const float pt = lt[(pos - 1) * RT_THREADS + tid];
                        const int pi = li[(pos - 1) * RT_THREADS + tid];
                        if (!before(t, id, pt, pi)) break;
                        lt[pos * RT_THREADS + tid] = pt;
                        li[pos * RT_THREADS + tid] = pi;
                        --pos;
                    }
                    lt[pos * RT_THREADS + tid] = t;
                    li[pos * RT_THREADS + tid] = id;
                    worst_t = lt[(k - 1) * RT_THREADS + tid];
                    worst_i = li[(k - 1) * RT_THREADS + tid];
                }
            }
        }
    }
    __syncthreads();
    if (tid < RT_QT && q0 + tid < nf) {                                    // the eight sorted lists of query tid -> one
        int head[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) head[l] = 0;
        const int64_t o = (((int64_t)row * Fr + q0 + tid) * nchunk + chunk) * k;
        for (int j = 0; j < k; ++j) {
            float bt = INFINITY;
            int bi = INT_MAX, bl = -1;
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                if (head[l] < k) {
                    const int col = l * 32 + tid;                          // wave l >> 1, lane half l & 1, lane tid of the half
                    const float t = lt[head[l] * RT_THREADS + col];
                    const int i = li[head[l] * RT_THREADS + col];
                    if (before(t, i, bt, bi)) {
                        bt = t;
                        bi = i;
                        bl = l;
                    }
                }
            }
#pragma unroll
            for (int l = 0; l < 8; ++l) head[l] += (l == bl);
            ws_t[o + j] = bt;
            ws_id[o + j] = bi;
        }
    }
}

__device__ __forceinline__ void wave_first(float& t, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t2 = __shfl_xor(t, o, 64);
        const int i2 = __shfl_xor(i, o, 64);
        if (before(t2, i2, t, i)) {
            t = t2;
            i = i2;
        }
    }
}

__global__ void __launch_bounds__(RT_THREADS) retrieve_blend_kernel(
    float* __restrict__ units, int64_t rows, int Fr, int C, const int32_t* __restrict__ n_frames,
    const int32_t* __restrict__ owner, int64_t J, const int32_t* __restrict__ index_of_row,
    const float* __restrict__ ratio_of_row, int64_t X, const int64_t* __restrict__ off,
    int64_t N_total, const float* __restrict__ vec, int k, int nchunk, const float* __restrict__ ws_t,
    const int32_t* __restrict__ ws_id, int32_t* __restrict__ nn_id, float* __restrict__ nn_dist, int* err) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (q >= rows * Fr) return;                                            // (uniform over the wave; no workgroup barrier below)
    const int64_t row = q / Fr;
    const int f = (int)(q % Fr);
    bool bad;
    const RowIndex ri = retrieve_row(row, owner, J, index_of_row, ratio_of_row, X, off, N_total, bad);
    if (bad && f == 0 && lane == 0) __hip_atomic_store(err, DDSP_DEV_ERR_RETRIEVE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (!ri.on || f >= ddsp_row_frames(n_frames, row, Fr)) {               // the frame keeps its bits
        if (lane < k) {
            if (nn_id) nn_id[q * k + lane] = -1;
            if (nn_dist) nn_dist[q * k + lane] = 0.f;
        }
        return;
    }
    const int ncand = nchunk * k;
    const float* __restrict__ ct = ws_t + q * ncand;
    const int32_t* __restrict__ ci = ws_id + q * ncand;
    int sel[RT_KMAX];
    float pt = -INFINITY;
    int pi = -1;
#pragma unroll
    for (int j = 0; j < RT_KMAX; ++j) {
        sel[j] = -1;
        if (j < k) {
            float bt = INFINITY;
            int bi = INT_MAX;
            for (int c = lane; c < ncand; c += 64) {
                const float t = ct[c];
                const int i = ci[c];
                if (before(pt, pi, t, i) && before(t, i, bt, bi)) {
                    bt = t;
                    bi = i;
                }
            }
            wave_first(bt, bi);
            if (bi >= 0 && (int64_t)bi < ri.n) sel[j] = bi;                // tested before it forms an address; padding is INT_MAX
            pt = bt;
            pi = bi;
        }
    }
    const int C4 = C >> 2;
    float* __restrict__ xp = units + q * C;
    const float* __restrict__ vbase = vec + ri.base * C;
    f32x4 x[4], y[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        x[p] = y[p] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (lane + 64 * p < C4) x[p] = *(const f32x4*)(xp + 4 * (lane + 64 * p));
    }
    float w[RT_KMAX], sum = 0.f;
#pragma unroll
    for (int j = 0; j < RT_KMAX; ++j) {
        w[j] = 0.f;
        if (j < k && sel[j] >= 0) {
            const float* __restrict__ v = vbase + (int64_t)sel[j] * C;
            float s = 0.f;
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (lane + 64 * p < C4) {
                    const f32x4 d = x[p] - *(const f32x4*)(v + 4 * (lane + 64 * p));
                    s += d[0] * d[0];
                    s += d[1] * d[1];
                    s += d[2] * d[2];
                    s += d[3] * d[3];
                }
            s = wave_sum(s);
            const float m = fmaxf(s, 1e-12f);
            w[j] = 1.f / (m * m);
            sum += w[j];
            if (lane == 0 && nn_dist) nn_dist[q * k + j] = s;
        } else if (j < k && lane == 0 && nn_dist) {
            nn_dist[q * k + j] = 0.f;
        }
        if (j < k && lane == 0 && nn_id) nn_id[q * k + j] = sel[j];
    }
#pragma unroll
    for (int j = 0; j < RT_KMAX; ++j)
        if (j < k && sel[j] >= 0) {
            const float* __restrict__ v = vbase + (int64_t)sel[j] * C;
            const float wn = w[j] / sum;
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (lane + 64 * p < C4) y[p] += wn * *(const f32x4*)(v + 4 * (lane + 64 * p));
        }
    if (sel[0] < 0) return;                                                // (no entry at all: nothing to blend with)
#pragma unroll
    for (int p = 0; p < 4; ++p)
        if (lane + 64 * p < C4) *(f32x4*)(xp + 4 * (lane + 64 * p)) = x[p] + ri.r * (y[p] - x[p]);
}

// nrm[i] = sum_c vec[i][c]^2: one wave per entry, a lane adds the squares of its float4s in ascending channel order, then
// the butterfly of wave_sum - a fixed order
__global__ void __launch_bounds__(RT_THREADS) index_norms_kernel(const float* __restrict__ vec, int64_t N, int C, float* __restrict__ nrm) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= N) return;
    float s = 0.f;
    for (int c4 = lane; c4 < (C >> 2); c4 += 64) {
        const f32x4 v = *(const f32x4*)(vec + i * C + 4 * c4);
        s += v[0] * v[0];
        s += v[1] * v[1];
        s += v[2] * v[2];
        s += v[3] * v[3];
    }
    s = wave_sum(s);
    if (lane == 0) nrm[i] = s;
}

// The device's CU count, a constant of the context: the runtime is asked once
int retrieve_cus(ddsp_ctx* ctx, int64_t* out) {
    if (ctx->cu_count <= 0) {
        int cus = 0;
        DDSP_HIP(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
        ctx->cu_count = cus > 0 ? cus : 256;
    }
    *out = ctx->cu_count;
    return DDSP_OK;
}

// The most chunks any call may take: one per stage of the largest index
int64_t retrieve_most_chunks(int64_t N_max) {
    const int64_t most = ceil_div64(N_max, RT_ET);
    return most > RT_MAX_CHUNKS ? RT_MAX_CHUNKS : most;
}

// The chunks of a call: enough workgroups for two per CU, at most one chunk per stage of the largest index
int retrieve_chunks(ddsp_ctx* ctx, int64_t rows, int64_t Fr, int64_t N_max, int* out) {
    int64_t cus;
    int rc;
    if ((rc = retrieve_cus(ctx, &cus))) return rc;
    int64_t n = ceil_div64(2 * cus, rows * ceil_div64(Fr, RT_QT));
    const int64_t most = retrieve_most_chunks(N_max);
    if (n > most) n = most;
    if (n < 1) n = 1;
    *out = (int)n;
    return DDSP_OK;
}

bool retrieve_shape_ok(int64_t rows, int64_t Fr, int k, int64_t N_max) {
    return rows >= 1 && Fr >= 1 && rows * Fr < (1ll << 31) && k >= 1 && k <= RT_KMAX && N_max >= 1 && N_max < (1ll << 31);
}

}  // namespace

extern "C" int ddsp_units_retrieve_workspace(ddsp_ctx* ctx, int64_t rows, int64_t Fr, int k, int64_t N_max, int64_t* bytes) {
    DDSP_REQUIRE(ctx, ctx && bytes, "ddsp_units_retrieve_workspace: null argument");
    DDSP_REQUIRE(ctx, retrieve_shape_ok(rows, Fr, k, N_max),
                 "ddsp_units_retrieve_workspace: bad shape (rows, Fr, N_max >= 1, rows * Fr and N_max < 2^31, 1 <= k <= 16)");
    // rows * chunks of a call is at most rows * most and, since chunks = ceil(2 CUs / (rows * tiles)) < 2 CUs / (rows * tiles) + 1,
    // below ceil(2 CUs / tiles) + rows: the smaller of the two grows with rows, which rows * chunks itself does not (the ceil),
    // so a workspace sized for R rows serves every call of at most R rows - the widths of a bank's ladder
    int64_t cus;
    int rc;
    if ((rc = retrieve_cus(ctx, &cus))) return rc;
    const int64_t a = rows * retrieve_most_chunks(N_max), b = ceil_div64(2 * cus, ceil_div64(Fr, RT_QT)) + rows;
    *bytes = (a < b ? a : b) * Fr * k * 8;
    return DDSP_OK;
}

extern "C" int ddsp_units_index_norms(ddsp_ctx* ctx, void* stream, const float* vec, int64_t N, int64_t C, float* nrm) {
    DDSP_REQUIRE(ctx, ctx && vec && nrm, "ddsp_units_index_norms: null argument");
    DDSP_REQUIRE(ctx, N >= 1 && N < (1ll << 31) && C >= 4 && C <= 1024 && C % 4 == 0,
                 "ddsp_units_index_norms: bad shape (1 <= N < 2^31, C a multiple of 4 in 4..1024)");
    DDSP_ENTER_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(index_norms_kernel, dim3((unsigned)ceil_div64(N, RT_THREADS / 64)), dim3(RT_THREADS), 0, st, vec, N, (int)C, nrm);
    ddsp_prof_end(ctx, st, 2.0 * (double)N * (double)C, 4.0 * (double)N * (double)(C + 1));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_units_retrieve(ddsp_ctx* ctx, void* stream, float* units, int64_t rows, int64_t Fr, int64_t C,
                                   const int32_t* n_frames, const int32_t* owner, int64_t J, const int32_t* index_of_row,
                                   const float* ratio_of_row, int64_t X,
                                   const int64_t* off, const float* vec, const float* nrm, int64_t N_total, int64_t N_max, int k,
                                   void* workspace, int64_t workspace_bytes, int32_t* nn_id, float* nn_dist) {
    DDSP_REQUIRE(ctx, ctx && units && index_of_row && ratio_of_row && off && vec && nrm && workspace,
                 "ddsp_units_retrieve: null argument");
    DDSP_REQUIRE(ctx, C >= 4 && C <= 1024 && C % 4 == 0, "ddsp_units_retrieve: C must be a multiple of 4 in 4..1024");
    DDSP_REQUIRE(ctx, retrieve_shape_ok(rows, Fr, k, N_max) && J >= 1 && J < (1ll << 31) && (owner || J >= rows) && X >= 1 && X < (1ll << 31) && N_total >= N_max && N_total < (1ll << 31),
                 "ddsp_units_retrieve: bad shape (rows, Fr, X >= 1, 1 <= N_max <= N_total < 2^31, 1 <= k <= 16)");
    int rc, nchunk;
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    DDSP_ENTER_DEVICE(ctx);
    if ((rc = retrieve_chunks(ctx, rows, Fr, N_max, &nchunk))) return rc;
    const int64_t cand = rows * Fr * nchunk * k;
    DDSP_REQUIRE(ctx, workspace_bytes >= cand * 8, "ddsp_units_retrieve: the workspace is smaller than ddsp_units_retrieve_workspace says");
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* ws_t = (float*)workspace;
    int32_t* ws_id = (int32_t*)workspace + cand;
    const int qtiles = (int)ceil_div64(Fr, RT_QT);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(retrieve_search_kernel, dim3((unsigned)(rows * qtiles), (unsigned)nchunk), dim3(RT_THREADS),
                       (size_t)k * RT_THREADS * 8, st, units, (int)Fr, (int)C, qtiles, n_frames, owner, J, index_of_row, ratio_of_row, X, off,
                       N_total, vec, nrm, k, ws_t, ws_id);
    hipLaunchKernelGGL(retrieve_blend_kernel, dim3((unsigned)ceil_div64(rows * Fr, RT_THREADS / 64)), dim3(RT_THREADS), 0, st, units,
                       rows, (int)Fr, (int)C, n_frames, owner, J, index_of_row, ratio_of_row, X, off, N_total, vec, k, nchunk, ws_t, ws_id, nn_id,
                       nn_dist, dev_err);
    ddsp_prof_end(ctx, st, 2.0 * (double)rows * (double)Fr * (double)N_max * (double)C,
                  4.0 * ((double)N_max * (double)(C + 1) * (double)(rows * qtiles) + 2.0 * (double)rows * (double)Fr * (double)C));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
