// A speaker timeline in FILE time -> the per-frame mix weights of one ragged render group, in one launch (reference: a
// `spk_mix_dict` whose values are (B, Frame, 1) tensors, `x = x + v * self.spk_embed(id - 1)` in `Unit2Control.forward`; there
// the caller builds the weight tensors of every slice on the host).
//
// Row r of the group's table is (file, start_frame, n_frames, start_sample, n_samples, job), `job_table`'s columns.  Job j owns
// the breakpoints bp_off[j] .. bp_off[j + 1] - 1: bp_frame (P) their positions in file frames, strictly increasing inside a job,
// bp_w (P, K) the weights of the job's K slots there, job_ids (J, K) the slots' 1-based speaker ids.  Frame t < n_frames of
// row r is file frame f = start_frame + t; its weights are the piecewise-linear interpolation of the job's breakpoints at f -
// the first breakpoint's before it, the last one's after it -, found by binary search and computed in fp64 as
//   w0 + (w1 - w0) * ((f - f0) / (f1 - f0))
// then rounded to fp32 (at a breakpoint, and between two equal weights, that IS the breakpoint's fp32 value).  Frames
// t >= n_frames get exact zeros.  A job outside [0, J), or one whose breakpoint range is empty or leaves [0, P), is tested before
// it forms an address: the row is then a padding row, ids 1 and weights 0.  grid (gx, R): the workgroups of a row share its
// N_max * K weights grid-strided; 4 B written per element, the breakpoints come from the cache.
#include "common.h"

namespace {

struct TimelineArgs {
    const int32_t* table;     // (R, 6)
    const int32_t* bp_off;    // (J + 1)
    const int32_t* bp_frame;  // (P)
    const float* bp_w;        // (P, K)
    const int32_t* job_ids;   // (J, K)
    int64_t J, P, N_max;
    int K;
    int32_t* ids_rows;        // (R, K)
    float* w_rows;            // (R, N_max, K)
};

__global__ void __launch_bounds__(256) mix_timeline_kernel(TimelineArgs a) {
    const int64_t r = blockIdx.y;
    const int32_t* __restrict__ row = a.table + 6 * r;
    const int64_t sf = row[1], job = row[5];
    int64_t nf = row[2];
    int64_t lo = 0, hi = 0;
    bool ok = job >= 0 && job < a.J;
    if (ok) {
        lo = a.bp_off[job];
        hi = a.bp_off[job + 1];
        ok = lo >= 0 && lo < hi && hi <= a.P;
    }
    if (!ok || nf < 0) nf = 0;
    if (nf > a.N_max) nf = a.N_max;
    if (blockIdx.x == 0 && threadIdx.x < a.K) a.ids_rows[r * a.K + threadIdx.x] = ok ? a.job_ids[job * a.K + threadIdx.x] : 1;
    float* __restrict__ out = a.w_rows + r * a.N_max * a.K;
    const int64_t total = a.N_max * a.K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t t = i / a.K;
        const int k = (int)(i - t * a.K);
        float w = 0.f;
        if (t < nf) {   // (nf > 0 only for a checked job: lo < hi inside [0, P])
            const int64_t f = sf + t;
            // the first breakpoint of the job behind f: [p, q) shrinks to it
            int64_t p = lo, q = hi;
            while (p < q) {
                const int64_t mid = (p + q) >> 1;
                if (a.bp_frame[mid] > f) q = mid;
                else p = mid + 1;
            }
            if (p == lo) {
                w = a.bp_w[lo * a.K + k];
            } else if (p == hi) {
                w = a.bp_w[(hi - 1) * a.K + k];
            } else {
                const int64_t f0 = a.bp_frame[p - 1], f1 = a.bp_frame[p];
                const double w0 = a.bp_w[(p - 1) * a.K + k], w1 = a.bp_w[p * a.K + k];
                w = f1 > f0 ? (float)(w0 + (w1 - w0) * ((double)(f - f0) / (double)(f1 - f0))) : (float)w0;
            }
        }
        out[i] = w;
    }
}

}  // namespace

extern "C" int ddsp_mix_timeline(ddsp_ctx* ctx, void* stream, const int32_t* table, int64_t R, int64_t J, const int32_t* bp_off,
                                 const int32_t* bp_frame, const float* bp_w, int64_t P, const int32_t* job_ids, int K,
                                 int64_t N_max, int32_t* ids_rows, float* w_rows) {
    DDSP_REQUIRE(ctx, ctx && (R == 0 || table) && bp_off && bp_frame && bp_w && job_ids && (R == 0 || (ids_rows && w_rows)),
                 "ddsp_mix_timeline: null argument");
    DDSP_REQUIRE(ctx, R >= 0 && R <= 65535 && J >= 1 && J < (1ll << 31) && P >= 1 && P < (1ll << 31) && K >= 1 && K <= 16 &&
                          N_max >= 1 && N_max < (1ll << 26),
                 "ddsp_mix_timeline: bad shape (R <= 65535, 1 <= K <= 16)");
    int rc;
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    if (R == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    TimelineArgs a;
    a.table = table;
    a.bp_off = bp_off;
    a.bp_frame = bp_frame;
    a.bp_w = bp_w;
    a.job_ids = job_ids;
    a.J = J;
    a.P = P;
    a.N_max = N_max;
    a.K = K;
    a.ids_rows = ids_rows;
    a.w_rows = w_rows;
    int64_t gx = ceil_div64(N_max * K, 256 * 4);
    const int64_t cap = ceil_div64(2048, R);
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(mix_timeline_kernel, dim3((unsigned)gx, (unsigned)R), dim3(256), 0, st, a);
    ddsp_prof_end(ctx, st, 0.0, 4.0 * (double)R * (double)N_max * (double)K);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
