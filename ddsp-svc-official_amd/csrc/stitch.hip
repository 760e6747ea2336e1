// The stitch of an offline conversion (reference: `main.py:165-173` with `cross_fade`, `main.py:50-57`): S rendered pieces
// placed into one fp64 waveform in one launch.  The reference appends or cross-fades slice after slice on the host, copying
// the whole result each time; here every output sample is a fold over the pieces that cover it (include/ddsp_amd.h states the
// rule), which equals the sequential loop for any overlap because a piece's fade region [p, p + fade) is exactly what the
// earlier pieces already cover of it.
//
// A workgroup owns TILE consecutive output samples, four per thread.  The table's ends p + len are nondecreasing, so the first
// piece that can cover the tile is found by binary search on them; from there the pieces are walked while p lies before the
// tile's end (p is nondecreasing).  Both are uniform over the workgroup.  Per piece a thread reads its four samples as one
// 16-byte load when all four lie inside the piece and the address is 16-byte aligned - which depends on the piece's address
// and p only, so a whole piece takes one path - and sample by sample under a bounds SELECT otherwise: no address outside
// x[0, len) is formed.  The blend is written with the rounded fp64 intrinsics so nothing contracts: it is numpy's
// `(1 - k) * a + k * b` step for step.  Bandwidth-bound: 4 B read and 8 B written per sample, two 16-byte stores per thread.
#include "common.h"

namespace {

constexpr int STITCH_THREADS = 256;
constexpr int STITCH_TILE = 4 * STITCH_THREADS;

typedef double f64x2 __attribute__((ext_vector_type(2)));

// numpy's linspace(0, 1, fade)[j]: arange * step with step = 1 / (fade - 1), the last element set to 1; [0] for fade == 1
__device__ __forceinline__ double fade_weight(int64_t j, int64_t fade, double step) {
    if (fade == 1) return 0.0;
    if (j == fade - 1) return 1.0;
    return __dmul_rn((double)j, step);
}

__device__ __forceinline__ double fold(double v, float x, int64_t j, int64_t fade, double step) {
    if (j >= fade) return (double)x;
    const double k = fade_weight(j, fade, step);
    return __dadd_rn(__dmul_rn(__dsub_rn(1.0, k), v), __dmul_rn(k, (double)x));
}

__global__ void __launch_bounds__(STITCH_THREADS) stitch_kernel(const ddsp_stitch_piece* __restrict__ pieces, int64_t S,
                                                                double* __restrict__ out, int64_t total) {
    const int64_t t_lo = (int64_t)blockIdx.x * STITCH_TILE;
    const int64_t t_hi = t_lo + STITCH_TILE < total ? t_lo + STITCH_TILE : total;
    // first piece whose end lies behind t_lo (ends are nondecreasing): every earlier piece ends at or before the tile
    int64_t lo = 0, hi = S;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (pieces[mid].p + pieces[mid].len > t_lo) hi = mid;
        else lo = mid + 1;
    }
    const int64_t t0 = t_lo + 4 * (int64_t)threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = lo; i < S; ++i) {
        const ddsp_stitch_piece pc = pieces[i];
        if (pc.p >= t_hi) break;
        const int64_t j0 = t0 - pc.p;
        if (j0 >= pc.len || j0 + 3 < 0) continue;   // none of this thread's four samples lies in the piece
        const double step = pc.fade > 1 ? __ddiv_rn(1.0, (double)(pc.fade - 1)) : 0.0;
        if (j0 >= 0 && j0 + 3 < pc.len && (((uintptr_t)(pc.x + j0)) & 15) == 0) {
            const f32x4 x = *(const f32x4*)(pc.x + j0);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fold(v[e], x[e], j0 + e, pc.fade, step);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t j = j0 + e;
                if (j >= 0 && j < pc.len) v[e] = fold(v[e], pc.x[j], j, pc.fade, step);
            }
        }
    }
    if (t0 + 3 < total) {
        *(f64x2*)(out + t0) = (f64x2){v[0], v[1]};
        *(f64x2*)(out + t0 + 2) = (f64x2){v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t0 + e < total) out[t0 + e] = v[e];
    }
}

// ---- 16-bit PCM of the stitched waveform -------------------------------------------------------------------------------------
// numpy's `clip(rint(x * 32768), -32768, 32767).astype(int16)` in one pass over the fp64 waveform, with the largest |x| and the
// number of clipped samples of every span (a span is one output file inside the tensor).  A workgroup owns PCM_TILE consecutive
// samples, four per thread: two 16-byte loads where the four lie before n at a 16-byte aligned address, 8-byte words under a
// bounds select otherwise (a waveform whose base is only 8-byte aligned takes the words throughout), one 8-byte store of the four
// int16 under the same rule.  The spans' ends are nondecreasing, so the first span that can reach the tile is found by binary
// search and the spans are walked while they begin before the tile's end - uniform over the workgroup, usually one span.  Per
// span the threads' maxima and counts are reduced over the wave with shuffles, over the four waves through the LDS, and thread 0
// issues one atomic max (|x| is not negative, so its bit pattern orders as an unsigned integer) and one atomic add.  A span
// entry only decides which samples count and which are zeroed: every address is the thread's own t < n, whatever the table holds.
// Bandwidth-bound: 8 B read and 2 B written per sample.
constexpr int PCM_THREADS = 256;
constexpr int PCM_TILE = 4 * PCM_THREADS;

typedef short i16x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(PCM_THREADS) pcm16_kernel(const double* __restrict__ x, int64_t n,
                                                            const int64_t* __restrict__ spans, int64_t J,
                                                            int16_t* __restrict__ out, unsigned long long* __restrict__ peak,
                                                            unsigned long long* __restrict__ clipped) {
    __shared__ double s_max[PCM_THREADS / 64];
    __shared__ unsigned s_cnt[PCM_THREADS / 64];
    const int64_t t_lo = (int64_t)blockIdx.x * PCM_TILE;
    const int64_t t_hi = t_lo + PCM_TILE < n ? t_lo + PCM_TILE : n;
    const int64_t t0 = t_lo + 4 * (int64_t)threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (t0 + 3 < n && (((uintptr_t)(x + t0)) & 15) == 0) {
        const f64x2 a = *(const f64x2*)(x + t0), b = *(const f64x2*)(x + t0 + 2);
        v[0] = a[0], v[1] = a[1], v[2] = b[0], v[3] = b[1];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t0 + e < n) v[e] = x[t0 + e];
    }
    short q[4];
    bool over[4], covered[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double r = rint(__dmul_rn(v[e], 32768.0));          // round half to even, as numpy's rint
        over[e] = r < -32768.0 || r > 32767.0;
        q[e] = (short)(int)fmin(fmax(r, -32768.0), 32767.0);
        covered[e] = false;
    }
    // first span whose end lies behind t_lo (no table: the one span [0, n))
    int64_t lo = 0, hi = spans ? J : 0;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (spans[2 * mid] + spans[2 * mid + 1] > t_lo) hi = mid;
        else lo = mid + 1;
    }
    for (int64_t s = lo; s < (spans ? J : 1); ++s) {
        const int64_t base = spans ? spans[2 * s] : 0, end = spans ? base + spans[2 * s + 1] : n;
        if (base >= t_hi) break;
        double m = 0.0;
        unsigned c = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t t = t0 + e;
            if (t >= base && t < end && t < n) {
                covered[e] = true;
                m = fmax(m, fabs(v[e]));
                c += over[e] ? 1u : 0u;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            m = fmax(m, __shfl_xor(m, d, 64));
            c += __shfl_xor(c, d, 64);
        }
        if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m, s_cnt[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 1; w < PCM_THREADS / 64; ++w) m = fmax(m, s_max[w]), c += s_cnt[w];
            if (peak) atomicMax(peak + s, (unsigned long long)__double_as_longlong(m));
            if (clipped) atomicAdd(clipped + s, (unsigned long long)c);
        }
        __syncthreads();   // the LDS words serve the next span
    }
    i16x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = covered[e] ? q[e] : (short)0;   // between the spans: exact zeros
    if (t0 + 3 < n && (((uintptr_t)(out + t0)) & 7) == 0) {
        *(i16x4*)(out + t0) = w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (t0 + e < n) out[t0 + e] = w[e];
    }
}

}  // namespace

extern "C" int ddsp_pcm16(ddsp_ctx* ctx, void* stream, const double* x, int64_t n, const int64_t* spans, int64_t J, int16_t* out,
                          double* peak, int64_t* clipped) {
    DDSP_REQUIRE(ctx, ctx && n >= 0 && J >= 0 && (spans || J <= 1), "ddsp_pcm16: negative size, or J spans without a table");
    DDSP_REQUIRE(ctx, ceil_div64(n, PCM_TILE) < (1ll << 31), "ddsp_pcm16: n too large");
    const int64_t n_stats = spans ? J : 1;
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    if (peak && n_stats) DDSP_HIP(ctx, hipMemsetAsync(peak, 0, (size_t)n_stats * sizeof(double), st));
    if (clipped && n_stats) DDSP_HIP(ctx, hipMemsetAsync(clipped, 0, (size_t)n_stats * sizeof(int64_t), st));
    if (n == 0) return DDSP_OK;
    DDSP_REQUIRE(ctx, x && ((uintptr_t)x & 7) == 0 && out && ((uintptr_t)out & 1) == 0, "ddsp_pcm16: x or out is null or misaligned");
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(pcm16_kernel, dim3((unsigned)ceil_div64(n, PCM_TILE)), dim3(PCM_THREADS), 0, st, x, n, spans, spans ? J : 0,
                       out, (unsigned long long*)peak, (unsigned long long*)clipped);
    ddsp_prof_end(ctx, st, 0.0, 10.0 * (double)n);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_stitch(ddsp_ctx* ctx, void* stream, const ddsp_stitch_piece* pieces, int64_t S, double* out, int64_t total) {
    DDSP_REQUIRE(ctx, ctx && S >= 0 && total >= 0 && (S == 0 || pieces), "ddsp_stitch: null table or negative size");
    if (total == 0) return DDSP_OK;
    DDSP_REQUIRE(ctx, out && ((uintptr_t)out & 15) == 0, "ddsp_stitch: out is null or not 16-byte aligned");
    DDSP_REQUIRE(ctx, ceil_div64(total, STITCH_TILE) < (1ll << 31), "ddsp_stitch: total too large");
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(stitch_kernel, dim3((unsigned)ceil_div64(total, STITCH_TILE)), dim3(STITCH_THREADS), 0, st, pieces, S, out,
                       total);
    ddsp_prof_end(ctx, st, 0.0, 12.0 * (double)total);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
