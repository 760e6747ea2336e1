// a15: the formant shift (`forward_formant`, offline jobs with a formant, realtime.StreamBank(formant=True)): a warp of the
// spectral-envelope columns of the control matrix along the frequency axis, in place, between the control network and the
// filter synthesis.  One launch, one pass over the warped columns.
//
// THE RULE (include/ddsp_amd.h at ddsp_ctrl_warp states it too).  A segment is n consecutive columns of a control row with an
// origin o: 0 for magnitude bins (bin j lies at j * df), 1 for harmonics (column j is harmonic j + 1).  For a factor a > 0 the
// warped segment is the envelope read at f / a, in fp32, one rounding per operation, nothing contracted:
//     p  = fl(fl(float(j + o) / a) - float(o));   p = min(max(p, 0), float(n - 1))
//     i0 = (int)floor(p);  i1 = min(i0 + 1, n - 1);  t = p - float(i0)                  (exact)
//     out[j] = (t == 0) ? in[i0] : fl(in[i0] + fl(fl(in[i1] - in[i0]) * t))
// t == 0 SELECTS: a == 1, every exact hit and every clamped end return the input's bits (-0.0, inf and NaN included).
//
// One workgroup per row of the matrix.  The row's factor is uniform over the workgroup: factor[row] (per frame), factor[row / Fr]
// (per batch row) or factor[slot_of_row[row / Fr]] (through a row table whose entry is tested against [0, S) before it forms an
// address; one outside is a padding row, factor 1).  A frame at or past its batch row's count (n_frames) has factor 1 whatever
// the array holds.  A factor of exactly 1 leaves the row untouched (what the rule gives).  A factor that is not finite or not > 0
// leaves the row untouched as well and raises the context's device error word: no address depends on the factor's value.
// In place, output j reads inputs other than j: a segment is staged in the LDS - the whole of it, behind a barrier - before its
// first store, and a row belongs to one workgroup, so no workgroup reads what another writes.  Rows are not 16-byte aligned in
// general (CombSubFast: 3 * 513 floats), so both the staging loads and the stores run a scalar head up to the first 16-byte
// boundary of the row's own address, 16-byte vectors over the body and a scalar tail.
#include "common.h"

namespace {

constexpr int WARP_MAX_SEG = 3;
constexpr int WARP_MAX_N = 4096;   // columns of one segment: the LDS stage, 16 KiB

struct WarpArgs {
    float* ctrl;                   // (rows, sum)
    int64_t sum, Fr;
    int n_seg;
    int first[WARP_MAX_SEG], n[WARP_MAX_SEG], origin[WARP_MAX_SEG];
    const float* factor;           // (rows) per frame, (B) per batch row, (S) behind the row table
    int per_frame;
    const int32_t* slot_of_row;    // (B) or null
    int64_t S;
    const int32_t* n_frames;       // (B) or null
    int* err;
};

__global__ void __launch_bounds__(256) ctrl_warp_kernel(WarpArgs a) {
    __shared__ __attribute__((aligned(16))) float stage[WARP_MAX_N];
    const int64_t row = blockIdx.x;
    const int64_t b = row / a.Fr;
    const int fr = (int)(row - b * a.Fr);
    if (fr >= ddsp_row_frames(a.n_frames, b, (int)a.Fr)) return;          // the padding of a ragged batch: factor 1
    int64_t at = a.per_frame ? row : b;
    if (a.slot_of_row) {
        at = (int64_t)a.slot_of_row[b];
        if (at < 0 || at >= a.S) return;                                  // a padding row: factor 1
    }
    const float alpha = a.factor[at];
    if (alpha == 1.0f) return;
    if (!(alpha > 0.0f && alpha <= 3.402823466e+38f)) {                   // NaN, inf, 0, negative: the row keeps its bits
        if (threadIdx.x == 0) __hip_atomic_store(a.err, DDSP_DEV_ERR_FORMANT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    for (int s = 0; s < a.n_seg; ++s) {
        const int n = a.n[s];
        if (n < 2) continue;                                              // one column: a copy
        float* __restrict__ seg = a.ctrl + row * a.sum + a.first[s];
        // head: the columns before the first 16-byte boundary of this segment's address; body: whole vectors behind it
        int head = (int)((16 - ((uintptr_t)seg & 15)) & 15) >> 2;
        head = head < n ? head : n;
        const int n_vec = (n - head) >> 2, tail = head + 4 * n_vec;
        for (int j = threadIdx.x; j < head; j += 256) stage[j] = seg[j];
        for (int v = threadIdx.x; v < n_vec; v += 256) {
            const f32x4 x = *(const f32x4*)(seg + head + 4 * v);
#pragma unroll
            for (int k = 0; k < 4; ++k) stage[head + 4 * v + k] = x[k];
        }
        for (int j = tail + threadIdx.x; j < n; j += 256) stage[j] = seg[j];
        __syncthreads();                                                  // the whole segment is staged before its first store
        const float o = (float)a.origin[s], last = (float)(n - 1);
        auto warped = [&](int j) -> float {
            float p = __fsub_rn(__fdiv_rn((float)(j + a.origin[s]), alpha), o);
            p = fminf(fmaxf(p, 0.0f), last);
            const int i0 = (int)floorf(p);
            const int i1 = i0 + 1 < n ? i0 + 1 : n - 1;
            const float t = __fsub_rn(p, (float)i0);
            const float x0 = stage[i0];
            if (t == 0.0f) return x0;
            return __fadd_rn(x0, __fmul_rn(__fsub_rn(stage[i1], x0), t));
        };
        for (int j = threadIdx.x; j < head; j += 256) seg[j] = warped(j);
        for (int v = threadIdx.x; v < n_vec; v += 256) {
            f32x4 y;
#pragma unroll
            for (int k = 0; k < 4; ++k) y[k] = warped(head + 4 * v + k);
            *(f32x4*)(seg + head + 4 * v) = y;
        }
        for (int j = tail + threadIdx.x; j < n; j += 256) seg[j] = warped(j);
        __syncthreads();                                                  // the stage is free for the next segment
    }
}

}  // namespace

extern "C" int ddsp_ctrl_warp(ddsp_ctx* ctx, void* stream, float* ctrl, int64_t rows, int64_t sum, const int32_t* segments,
                              int n_seg, const float* factor, int per_frame, int64_t Fr, const int32_t* slot_of_row, int64_t S,
                              const int32_t* n_frames) {
    DDSP_REQUIRE(ctx, ctx && segments && factor && (rows == 0 || ctrl), "ddsp_ctrl_warp: null argument");
    DDSP_REQUIRE(ctx, rows >= 0 && rows < (1ll << 31) && sum >= 1 && sum < (1ll << 31) && Fr >= 1 && Fr < (1ll << 31) &&
                          rows % Fr == 0 && n_seg >= 1 && n_seg <= WARP_MAX_SEG,
                 "ddsp_ctrl_warp: bad shape (rows a multiple of Fr, 1 to 3 segments)");
    DDSP_REQUIRE(ctx, slot_of_row ? (S >= 1 && !per_frame) : true,
                 "ddsp_ctrl_warp: a row table goes with S >= 1 factors, one per slot, and not with a factor per frame");
    WarpArgs a;
    for (int s = 0; s < n_seg; ++s) {
        const int64_t first = segments[3 * s], n = segments[3 * s + 1], origin = segments[3 * s + 2];
        DDSP_REQUIRE(ctx, first >= 0 && n >= 1 && n <= WARP_MAX_N && first + n <= sum && (origin == 0 || origin == 1),
                     "ddsp_ctrl_warp: a segment is (first column, n, origin) inside the row, 1 <= n <= 4096, origin 0 or 1");
        a.first[s] = (int)first;
        a.n[s] = (int)n;
        a.origin[s] = (int)origin;
    }
    for (int s = n_seg; s < WARP_MAX_SEG; ++s) a.first[s] = a.n[s] = a.origin[s] = 0;
    int rc;
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    if (rows == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;
    a.ctrl = ctrl;
    a.sum = sum;
    a.Fr = Fr;
    a.n_seg = n_seg;
    a.factor = factor;
    a.per_frame = per_frame ? 1 : 0;
    a.slot_of_row = slot_of_row;
    a.S = S;
    a.n_frames = n_frames;
    a.err = dev_err;
    double cols = 0.0;
    for (int s = 0; s < n_seg; ++s) cols += (double)a.n[s];
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(ctrl_warp_kernel, dim3((unsigned)rows), dim3(256), 0, st, a);
    ddsp_prof_end(ctx, st, 0.0, 8.0 * (double)rows * cols);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
