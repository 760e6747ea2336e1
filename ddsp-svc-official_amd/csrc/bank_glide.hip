// a14: the speaker glide of a stream bank (realtime.StreamBank, `glide_breakpoints=`): the per-frame mix weights of one call's
// rows from per-SLOT state, and the advance of those slots' clocks, in one launch per block.
//
// A slot owns a clock (device samples pushed into it since its timeline started), a breakpoint count bp_n[s] (0: no timeline), the
// breakpoint times bp_t[s] (P_max) in device samples, strictly increasing, and the weights bp_w[s] (P_max, K) there.  Row r of the
// call is slot s = rows ? rows[r] : r, tested against [0, S) before it forms an address; one outside is a padding row, weights
// (1, 0, ..., 0) in every frame, no clock read or written, no error word.  For a real row c = clock[s] + block is the stream
// position just behind the window's newest sample, and frame t of the window has time tau = (double)(c - n_in) + t * hop.  Without
// a timeline every frame gets spk_w[s]; with one the weights are the breakpoints interpolated at tau as ddsp_mix_timeline
// interpolates them: binary search for the first breakpoint behind tau, the first one's weights before it, the last one's after
// it, and between two  w0 + (w1 - w0) * ((tau - t0) / (t1 - t0))  in fp64, rounded to fp32 (at a breakpoint that IS its fp32
// value).  One workgroup per row: every thread reads the clock into a register, the workgroup meets after its last frame, and only
// then thread 0 stores clock[s] = c.  The host names a slot at most once, so no other workgroup touches that clock; a slot that
// `rows` does not name is neither read nor written.
#include "common.h"

namespace {

struct GlideArgs {
    const int32_t* rows;      // (W) or null
    int64_t* clock;           // (S)
    const int32_t* bp_n;      // (S)
    const int64_t* bp_t;      // (S, P_max)
    const float* bp_w;        // (S, P_max, K)
    const float* spk_w;       // (S, K)
    int S, P_max, K;
    int64_t Fr, n_in, block;
    double hop;
    float* w_frames;          // (W, Fr, K)
};

__global__ void __launch_bounds__(256) bank_glide_kernel(GlideArgs a) {
    const int64_t r = blockIdx.x;
    const int64_t total = a.Fr * a.K;
    float* __restrict__ out = a.w_frames + r * total;
    const int64_t s = a.rows ? (int64_t)a.rows[r] : r;
    if (s < 0 || s >= a.S) {                                      // a padding row: the bank's padding speaker
        for (int64_t i = threadIdx.x; i < total; i += 256) out[i] = i % a.K == 0 ? 1.f : 0.f;
        return;
    }
    const int64_t c = a.clock[s] + a.block;                      // every thread: read before the barrier, stored after it
    int n = a.bp_n[s];
    n = n < 0 ? 0 : (n > a.P_max ? a.P_max : n);
    const int64_t* __restrict__ bt = a.bp_t + s * a.P_max;
    const float* __restrict__ bw = a.bp_w + s * a.P_max * a.K;
    const float* __restrict__ sw = a.spk_w + s * a.K;
    const double first = (double)(c - a.n_in);
    for (int64_t i = threadIdx.x; i < total; i += 256) {
        const int64_t t = i / a.K;
        const int k = (int)(i - t * a.K);
        float w;
        if (n == 0) {
            w = sw[k];
        } else {
            const double tau = first + (double)t * a.hop;
            // the first breakpoint behind tau: [p, q) shrinks to it
            int p = 0, q = n;
            while (p < q) {
                const int mid = (p + q) >> 1;
                if ((double)bt[mid] > tau) q = mid;
                else p = mid + 1;
            }
            if (p == 0) {
                w = bw[k];
            } else if (p == n) {
                w = bw[(n - 1) * a.K + k];
            } else {
                const double t0 = (double)bt[p - 1], t1 = (double)bt[p];
                const double w0 = bw[(p - 1) * a.K + k], w1 = bw[p * a.K + k];
                w = t1 > t0 ? (float)(w0 + (w1 - w0) * ((tau - t0) / (t1 - t0))) : (float)w0;
            }
        }
        out[i] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) a.clock[s] = c;
}

}  // namespace

extern "C" int ddsp_bank_glide(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int S, int64_t* clock, const int32_t* bp_n,
                               const int64_t* bp_t, const float* bp_w, int P_max, const float* spk_w, int K, int64_t Fr,
                               int64_t n_in, int64_t block, double hop, float* w_frames) {
    DDSP_REQUIRE(ctx, ctx && clock && bp_n && bp_t && bp_w && spk_w && (W == 0 || w_frames), "ddsp_bank_glide: null argument");
    DDSP_REQUIRE(ctx, W >= 0 && W <= 65535 && S >= 1 && K >= 1 && K <= 16 && P_max >= 1 && P_max <= 64 && Fr >= 1 &&
                          Fr < ((int64_t)1 << 26) && block >= 1 && n_in >= 1 && hop > 0.0,
                 "ddsp_bank_glide: bad shape (W <= 65535, 1 <= K <= 16, 1 <= P_max <= 64, Fr >= 1, block >= 1)");
    if (W == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    GlideArgs a;
    a.rows = rows;
    a.clock = clock;
    a.bp_n = bp_n;
    a.bp_t = bp_t;
    a.bp_w = bp_w;
    a.spk_w = spk_w;
    a.S = S;
    a.P_max = P_max;
    a.K = K;
    a.Fr = Fr;
    a.n_in = n_in;
    a.block = block;
    a.hop = hop;
    a.w_frames = w_frames;
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(bank_glide_kernel, dim3((unsigned)W), dim3(256), 0, st, a);
    ddsp_prof_end(ctx, st, 0.0, 4.0 * (double)W * (double)Fr * (double)K);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// The KEY glide of a stream bank (`pitch_breakpoints=`): the per-frame f0 factors of one call's rows from per-slot state, and the
// advance of those slots' key clocks - the launch above with a key timeline (key_timeline.h) in place of the mix weights.  A slot
// owns key_clock[s], key_n[s] (0: no timeline), key_t[s] (P_max) in device samples, strictly increasing, and key_semi[s] /
// key_fac[s] (P_max), the breakpoints' semitones and host-formed factors.  Rows, padding rows (factor 1 in every frame, no
// clock touched), the frame times and the clock's read-before / store-after the barrier are those of bank_glide_kernel.  Without
// a timeline every frame gets pitch[s], the slot's one factor.
#include "key_timeline.h"

namespace {

struct KeyGlideArgs {
    const int32_t* rows;      // (W) or null
    int64_t* clock;           // (S)
    const int32_t* key_n;     // (S)
    const int64_t* key_t;     // (S, P_max)
    const float* key_semi;    // (S, P_max)
    const float* key_fac;     // (S, P_max)
    const float* pitch;       // (S)
    int S, P_max;
    int64_t Fr, n_in, block;
    double hop;
    float* pitch_frames;      // (W, Fr)
};

__global__ void __launch_bounds__(256) bank_key_glide_kernel(KeyGlideArgs a) {
    const int64_t r = blockIdx.x;
    float* __restrict__ out = a.pitch_frames + r * a.Fr;
    const int64_t s = a.rows ? (int64_t)a.rows[r] : r;
    if (s < 0 || s >= a.S) {                                      // a padding row: no shift
        for (int64_t t = threadIdx.x; t < a.Fr; t += 256) out[t] = 1.f;
        return;
    }
    const int64_t c = a.clock[s] + a.block;                      // every thread: read before the barrier, stored after it
    int n = a.key_n[s];
    n = n < 0 ? 0 : (n > a.P_max ? a.P_max : n);
    const int64_t* __restrict__ bt = a.key_t + s * a.P_max;
    const float* __restrict__ semi = a.key_semi + s * a.P_max;
    const float* __restrict__ fac = a.key_fac + s * a.P_max;
    const float one = a.pitch[s];
    const double first = (double)(c - a.n_in);
    for (int64_t t = threadIdx.x; t < a.Fr; t += 256)
        out[t] = n == 0 ? one : keytl::factor_at(bt, semi, fac, n, first + (double)t * a.hop);
    __syncthreads();
    if (threadIdx.x == 0) a.clock[s] = c;
}

}  // namespace

extern "C" int ddsp_bank_key_glide(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int S, int64_t* key_clock,
                                   const int32_t* key_n, const int64_t* key_t, const float* key_semi, const float* key_fac,
                                   int P_max, const float* pitch, int64_t Fr, int64_t n_in, int64_t block, double hop,
                                   float* pitch_frames) {
    DDSP_REQUIRE(ctx, ctx && key_clock && key_n && key_t && key_semi && key_fac && pitch && (W == 0 || pitch_frames),
                 "ddsp_bank_key_glide: null argument");
    DDSP_REQUIRE(ctx, W >= 0 && W <= 65535 && S >= 1 && P_max >= 1 && P_max <= 64 && Fr >= 1 && Fr < ((int64_t)1 << 26) &&
                          block >= 1 && n_in >= 1 && hop > 0.0,
                 "ddsp_bank_key_glide: bad shape (W <= 65535, 1 <= P_max <= 64, Fr >= 1, block >= 1)");
    if (W == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    KeyGlideArgs a;
    a.rows = rows;
    a.clock = key_clock;
    a.key_n = key_n;
    a.key_t = key_t;
    a.key_semi = key_semi;
    a.key_fac = key_fac;
    a.pitch = pitch;
    a.S = S;
    a.P_max = P_max;
    a.Fr = Fr;
    a.n_in = n_in;
    a.block = block;
    a.hop = hop;
    a.pitch_frames = pitch_frames;
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(bank_key_glide_kernel, dim3((unsigned)W), dim3(256), 0, st, a);
    ddsp_prof_end(ctx, st, 0.0, 4.0 * (double)W * (double)Fr);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
