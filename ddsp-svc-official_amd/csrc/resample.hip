// SURVEY 8(f) rank 3 - device-side sample-rate conversion: the windowed-sinc polyphase resampler the reference takes
// from torchaudio (`Resample(orig, new, lowpass_filter_width=128)`: gui.py:399-404 between the model's and the audio
// device's rate, enhancer.py:50-53,69-73 around the adaptive-key trick).  torchaudio is a third-party package that is
// not in the image: the algorithm below is its published one (torchaudio.functional.resample, `sinc_interp_hann`,
// rolloff 0.99), PARITY UNPINNED at that boundary; tests hold the kernels to an fp64 evaluation of the same formulas.
//   orig, new reduced by their gcd; base = min(orig, new) * rolloff; width = ceil(lowpass_width * orig / base);
//   tap[p][k] = sinc(pi t) * cos^2(pi t / (2 lowpass_width)) * base / orig,
//       t = clamp((-p / new + (k - width) / orig) * base, -lowpass_width, lowpass_width),   p < new, k < 2 width + orig;
//   out[l * new + p] = sum_k x[l * orig + k - width] * tap[p][k]   (x zero outside [0, T)),  T_out = ceil(new * T / orig).
// The taps are evaluated in fp64 and rounded to fp32 once (torchaudio computes them in fp64 too when no dtype is given);
// the table is cached in the context (one per rate pair), stored [k][phase].  Convolution: a thread owns one phase for 8
// consecutive input frames (8 outputs `new` samples apart): a tap is loaded once - the 256 phases of a workgroup read 1 KB
// rows of the table - and meets the workgroup's input window (7 orig + K samples in the LDS, broadcast reads) eight times.
// (One thread per output with the table stored [phase][k] moved 64 lanes x K floats of table per wave and output: 0.55 ms
// for 10 s of audio, bound by the L2.)  Rate pairs whose window does not fit the LDS take the one-output-per-thread kernel.
#include "common.h"

#include <math.h>

namespace {

__global__ void __launch_bounds__(256) resample_taps_kernel(float* __restrict__ taps, int orig, int nw, int width, int K,
                                                            double base, double lpw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)nw * K) return;
    const int k = (int)(i / nw), p = (int)(i - (int64_t)k * nw);   // stored [k][p]: the phases of a tap are contiguous
    double t = (-(double)p / (double)nw + (double)(k - width) / (double)orig) * base;
    t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
    const double c = cos(t * M_PI / lpw / 2.0);
    const double tp = t * M_PI;
    const double s = tp == 0.0 ? 1.0 : sin(tp) / tp;
    taps[i] = (float)(s * c * c * (base / (double)orig));
}

// Ragged batch (ns != nullptr): row b holds ns[b] samples of its own (held inside 0..T); what follows them is never read
// (the window stops at the row's end, as it does at T for a row resampled alone) and the outputs from
// ceil(new * ns[b] / orig) on are written as 0.
__device__ __forceinline__ int64_t row_samples(const int32_t* __restrict__ ns, int64_t b, int64_t T) {
    if (!ns) return T;
    const int64_t n = ns[b];
    return n < 0 ? 0 : (n > T ? T : n);
}

constexpr int RS_RB = 8;   // input frames per thread of the blocked form

// one output of the one-output-per-thread form: o < the row's own outputs, T the row's own samples
__device__ __forceinline__ float resample_direct_one(const float* __restrict__ xr, const float* __restrict__ taps, int64_t T,
                                                     int64_t o, int orig, int nw, int width, int K) {
    const int64_t l = o / nw;
    const int p = (int)(o - l * nw);
    const float* tp = taps + p;   // [k][phase]
    const int64_t first = l * orig - width;
    int k0 = first < 0 ? (int)(-first) : 0;
    int k1 = first + K > T ? (int)(T - first) : K;
    // four partial sums (the order of a long fp32 sum matters at the 1e-7 level; a blocked sum is closer to the exact
    // value than a running one)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int k = k0;
    for (; k + 3 < k1; k += 4) {
        a0 = fmaf(xr[first + k], tp[(int64_t)k * nw], a0);
        a1 = fmaf(xr[first + k + 1], tp[(int64_t)(k + 1) * nw], a1);
        a2 = fmaf(xr[first + k + 2], tp[(int64_t)(k + 2) * nw], a2);
        a3 = fmaf(xr[first + k + 3], tp[(int64_t)(k + 3) * nw], a3);
    }
    for (; k < k1; ++k) a0 = fmaf(xr[first + k], tp[(int64_t)k * nw], a0);
    return (a0 + a1) + (a2 + a3);
}

__global__ void __launch_bounds__(256) resample_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                       int64_t Tpad, int64_t T_out, int orig, int nw, int width, int K,
                                                       int64_t total, float* __restrict__ out, const int32_t* __restrict__ ns) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / T_out, o = i - b * T_out;
        const int64_t T = row_samples(ns, b, Tpad);
        // (past the row's own outputs: never in a rectangular call)
        out[i] = o >= (nw * T + orig - 1) / orig ? 0.f : resample_direct_one(x + b * Tpad, taps, T, o, orig, nw, width, K);
    }
}

// the work of one workgroup of the blocked form: phases bx * 256 .. of the input frames l0 .. l0 + RS_RB - 1 of row b
__device__ __forceinline__ void resample_blocked_body(const float* __restrict__ x, const float* __restrict__ taps, int64_t Tpad,
                                                      int64_t T_out, int orig, int nw, int width, int K, float* __restrict__ out,
                                                      const int32_t* __restrict__ ns, float* win, int bx, int64_t l0, int64_t b) {
    const int p = bx * 256 + threadIdx.x;
    const int wlen = (RS_RB - 1) * orig + K;
    const int64_t first = l0 * orig - width;
    const float* xr = x + b * Tpad;
    const int64_t T = row_samples(ns, b, Tpad);
    const int64_t T_row = ((int64_t)nw * T + orig - 1) / orig;   // the row's own outputs (T_out in a rectangular call)
    for (int i = threadIdx.x; i < wlen; i += 256) {
        const int64_t pos = first + i;
        win[i] = (pos >= 0 && pos < T) ? xr[pos] : 0.f;
    }
    __syncthreads();
    if (p >= nw) return;
    float acc[RS_RB][2];
#pragma unroll
    for (int r = 0; r < RS_RB; ++r) acc[r][0] = acc[r][1] = 0.f;
    const float* tp = taps + p;
    int k = 0;
    for (; k + 1 < K; k += 2) {
        const float t0 = tp[(int64_t)k * nw], t1 = tp[(int64_t)(k + 1) * nw];
#pragma unroll
        for (int r = 0; r < RS_RB; ++r) {
            acc[r][0] = fmaf(win[r * orig + k], t0, acc[r][0]);
            acc[r][1] = fmaf(win[r * orig + k + 1], t1, acc[r][1]);
        }
    }
    if (k < K) {
        const float t0 = tp[(int64_t)k * nw];
#pragma unroll
        for (int r = 0; r < RS_RB; ++r) acc[r][0] = fmaf(win[r * orig + k], t0, acc[r][0]);
    }
#pragma unroll
    for (int r = 0; r < RS_RB; ++r) {
        const int64_t o = (l0 + r) * nw + p;
        if (o < T_out) out[b * T_out + o] = o < T_row ? acc[r][0] + acc[r][1] : 0.f;
    }
}

__global__ void __launch_bounds__(256) resample_blocked_kernel(const float* __restrict__ x, const float* __restrict__ taps,
                                                               int64_t Tpad, int64_t T_out, int orig, int nw, int width, int K,
                                                               float* __restrict__ out, const int32_t* __restrict__ ns) {
    extern __shared__ float win[];
    resample_blocked_body(x, taps, Tpad, T_out, orig, nw, width, K, out, ns, win, (int)blockIdx.x, (int64_t)blockIdx.y * RS_RB,
                          (int64_t)blockIdx.z);
}

// Keyed batch: row b is resampled with the rate pair pairs[key[b]] of a plan (ddsp_resample_keyed_plan).  The pair is uniform
// over a workgroup, and the grid and the LDS are those of the largest pair of the set: a workgroup that has no output of its
// row's pair returns at once, one past the row's own outputs writes its zeros and stages nothing, and the others run the body
// of the kernel `ddsp_resample` would launch for that pair - the same taps in the same order, so the same bits.
enum { RS_MODE_BLOCKED = 0, RS_MODE_DIRECT = 1, RS_MODE_COPY = 2 };
struct RsPair {
    const float* taps;
    int orig, nw, width, K, mode, pad_;
};

__global__ void __launch_bounds__(256) resample_keyed_kernel(const float* __restrict__ x, const RsPair* __restrict__ pairs, int n_pairs,
                                                             int64_t Tpad, int64_t T_out, float* __restrict__ out,
                                                             const int32_t* __restrict__ ns, const int32_t* __restrict__ key) {
    extern __shared__ float win[];
    const int64_t b = blockIdx.z;
    int k = __builtin_amdgcn_readfirstlane(key[b]);
    k = k < 0 ? 0 : (k >= n_pairs ? n_pairs - 1 : k);   // a garbage key reads no table it should not
    const RsPair pr = pairs[k];
    const int64_t T = row_samples(ns, b, Tpad);
    if (pr.mode == RS_MODE_BLOCKED) {
        const int64_t l0 = (int64_t)blockIdx.y * RS_RB;
        if ((int64_t)blockIdx.x * 256 >= pr.nw || l0 * pr.nw >= T_out) return;   // no output of this pair lives here
        const int64_t T_row = ((int64_t)pr.nw * T + pr.orig - 1) / pr.orig;
        if (l0 * pr.nw >= T_row) {                                              // past the row's own extent
            const int p = blockIdx.x * 256 + threadIdx.x;
            if (p < pr.nw)
                for (int r = 0; r < RS_RB; ++r) {
                    const int64_t o = (l0 + r) * pr.nw + p;
                    if (o < T_out) out[b * T_out + o] = 0.f;
                }
            return;
        }
        resample_blocked_body(x, pr.taps, Tpad, T_out, pr.orig, pr.nw, pr.width, pr.K, out, ns, win, (int)blockIdx.x, l0, b);
        return;
    }
    // the one-output-per-thread form and the copy of an identity pair: the row's workgroups stride over its outputs
    const int64_t G = (int64_t)gridDim.x * gridDim.y * 256;
    const int64_t T_row = pr.mode == RS_MODE_COPY ? T : ((int64_t)pr.nw * T + pr.orig - 1) / pr.orig;
    const float* xr = x + b * Tpad;
    for (int64_t o = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; o < T_out; o += G) {
        float v = 0.f;
        if (o < T_row) v = pr.mode == RS_MODE_COPY ? xr[o] : resample_direct_one(xr, pr.taps, T, o, pr.orig, pr.nw, pr.width, pr.K);
        out[b * T_out + o] = v;
    }
}

int gcd_int(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace

// table kinds 100.. (tables.hip keeps 0..): key n0 = orig / g, n1 = (new / g) * 8192 + lowpass width (both fit an int: the
// reduced rates are < 65536, the width <= 4096).  At most RS_TABLES_MAX tap tables live in a context: `Enhancer.enhance` with
// adaptive_key='auto' asks for two new rate pairs per distinct key, so a long-running server evicts the least recently used
// one (a hipFree, i.e. a device synchronisation, like the first use of any table) instead of filling the cache.
constexpr int TAB_RESAMPLE = 100;
constexpr int RS_TABLES_MAX = 8;

extern "C" int64_t ddsp_resample_length(int64_t T, int orig_freq, int new_freq) {
    if (T < 0 || orig_freq < 1 || new_freq < 1) return -1;
    const int g = gcd_int(orig_freq, new_freq);
    const int64_t o = orig_freq / g, n = new_freq / g;
    return (n * T + o - 1) / o;
}

// n_samples == nullptr is the rectangular batch
extern "C" int ddsp_resample(ddsp_ctx* ctx, void* stream, const float* x, int64_t B, int64_t T, const int32_t* n_samples,
                             int orig_freq, int new_freq, int lowpass_filter_width, float* out) {
    DDSP_REQUIRE(ctx, ctx && x && out, "ddsp_resample: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && T >= 1 && orig_freq >= 1 && new_freq >= 1 && lowpass_filter_width >= 1 &&
                          lowpass_filter_width <= 4096,
                 "ddsp_resample: bad argument");
    if (B == 0) return DDSP_OK;
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    const int g = gcd_int(orig_freq, new_freq);
    const int orig = orig_freq / g, nw = new_freq / g;
    DDSP_REQUIRE(ctx, orig < 65536 && nw < 65536, "ddsp_resample: rate ratio too fine (reduced rates must be < 65536)");
    const double rolloff = 0.99;
    const double base = (double)(orig < nw ? orig : nw) * rolloff;
    const int width = (int)ceil((double)lowpass_filter_width * (double)orig / base);
    const int K = 2 * width + orig;
    DDSP_REQUIRE(ctx, (int64_t)nw * K < (1 << 28), "ddsp_resample: tap table too large");
    float* taps = nullptr;
    const int key0 = orig, key1 = nw * 8192 + lowpass_filter_width;
    const uint64_t now = ++ctx->table_clock;
    int n_rs = 0, lru = -1;
    for (int i = 0; i < ctx->n_tables; ++i) {
        ddsp_table& t = ctx->tables[i];
        if (t.kind != TAB_RESAMPLE) continue;
        ++n_rs;
        if (t.n0 == key0 && t.n1 == key1) {
            taps = t.dev;
            t.last_use = now;
        } else if (lru < 0 || t.last_use < ctx->tables[lru].last_use) {
            lru = i;
        }
    }
    if (!taps) {
        if ((n_rs >= RS_TABLES_MAX || ctx->n_tables >= 64) && lru >= 0) {
            // kernels of earlier calls may still read the evicted table: hipFree waits for the device
            DDSP_HIP(ctx, hipFree(ctx->tables[lru].dev));
            ctx->tables[lru] = ctx->tables[--ctx->n_tables];
        }
        if (ctx->n_tables >= 64) return ddsp_fail(ctx, DDSP_ERR_OOM, "table cache full", "");
        const size_t bytes = (size_t)nw * K * sizeof(float);
        hipError_t e = hipMalloc((void**)&taps, bytes);
        if (e != hipSuccess) return ddsp_fail(ctx, DDSP_ERR_OOM, "resample taps hipMalloc", hipGetErrorString(e));
        hipLaunchKernelGGL(resample_taps_kernel, dim3((unsigned)(((int64_t)nw * K + 255) / 256)), dim3(256), 0, st, taps, orig,
                           nw, width, K, base, (double)lowpass_filter_width);
        DDSP_LAUNCH_CHECK(ctx);
        ddsp_table& t = ctx->tables[ctx->n_tables++];
        t.kind = TAB_RESAMPLE;
        t.n0 = key0;
        t.n1 = key1;
        t.dev = taps;
        t.bytes = bytes;
        t.last_use = now;
    }
    const int64_t T_out = ((int64_t)nw * T + orig - 1) / orig;
    const int64_t total = B * T_out;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    const size_t lds = ((size_t)(RS_RB - 1) * orig + K) * sizeof(float);
    const int64_t n_frames = (T_out + nw - 1) / nw;
    if (lds <= 64 * 1024 && B < 65536 && (n_frames + RS_RB - 1) / RS_RB < 65536)
        hipLaunchKernelGGL(resample_blocked_kernel, dim3((unsigned)((nw + 255) / 256), (unsigned)((n_frames + RS_RB - 1) / RS_RB), (unsigned)B),
                           dim3(256), lds, st, x, taps, T, T_out, orig, nw, width, K, out, n_samples);
    else
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, taps, T, T_out, orig, nw, width, K, total,
                           out, n_samples);
    ddsp_prof_end(ctx, st, 2.0 * total * K, 4.0 * (B * T + total));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// ---- keyed batches: one launch, a rate pair per row ---------------------------------------------------------------------------
// A plan owns the tap tables of its pairs in ONE allocation of its own (descriptors first, then the tables): they are built
// when the plan is, all stay resident while it lives, and the context's LRU of solo tables never sees them.
constexpr int RS_PLAN_MAX_PAIRS = 13;

struct ddsp_resample_plan {
    int device, n_pairs, lowpass;
    int orig_freq[RS_PLAN_MAX_PAIRS], new_freq[RS_PLAN_MAX_PAIRS];
    RsPair host[RS_PLAN_MAX_PAIRS];
    char* dev;         // RsPair[RS_PLAN_MAX_PAIRS], then the tap tables
    int max_nw;
    size_t lds;        // of the largest blocked pair
};

extern "C" int ddsp_resample_keyed_plan(ddsp_ctx* ctx, void* stream, int n_pairs, const int* orig_freq, const int* new_freq,
                                        int lowpass_filter_width, ddsp_resample_plan** plan) {
    DDSP_REQUIRE(ctx, ctx && orig_freq && new_freq && plan, "ddsp_resample_keyed_plan: null argument");
    DDSP_REQUIRE(ctx, n_pairs >= 1 && n_pairs <= RS_PLAN_MAX_PAIRS && lowpass_filter_width >= 1 && lowpass_filter_width <= 4096,
                 "ddsp_resample_keyed_plan: bad argument (1 to 13 pairs)");
    *plan = nullptr;
    ddsp_resample_plan pl = {};
    pl.device = ctx->device;
    pl.n_pairs = n_pairs;
    pl.lowpass = lowpass_filter_width;
    size_t floats[RS_PLAN_MAX_PAIRS] = {}, total = 0;
    double base[RS_PLAN_MAX_PAIRS] = {};
    for (int i = 0; i < n_pairs; ++i) {
        DDSP_REQUIRE(ctx, orig_freq[i] >= 1 && new_freq[i] >= 1, "ddsp_resample_keyed_plan: bad rate");
        pl.orig_freq[i] = orig_freq[i];
        pl.new_freq[i] = new_freq[i];
        RsPair& p = pl.host[i];
        if (orig_freq[i] == new_freq[i]) {   // the row is copied (what the callers of ddsp_resample do for equal rates)
            p.mode = RS_MODE_COPY;
            p.orig = p.nw = 1;
            continue;
        }
        // (the arithmetic of resample_run, so that the tables are the ones ddsp_resample builds)
        const int g = gcd_int(orig_freq[i], new_freq[i]);
        p.orig = orig_freq[i] / g;
        p.nw = new_freq[i] / g;
        DDSP_REQUIRE(ctx, p.orig < 65536 && p.nw < 65536, "ddsp_resample_keyed_plan: rate ratio too fine (reduced rates must be < 65536)");
        base[i] = (double)(p.orig < p.nw ? p.orig : p.nw) * 0.99;
        p.width = (int)ceil((double)lowpass_filter_width * (double)p.orig / base[i]);
        p.K = 2 * p.width + p.orig;
        DDSP_REQUIRE(ctx, (int64_t)p.nw * p.K < (1 << 28), "ddsp_resample_keyed_plan: tap table too large");
        const size_t lds = ((size_t)(RS_RB - 1) * p.orig + p.K) * sizeof(float);
        p.mode = lds <= 64 * 1024 ? RS_MODE_BLOCKED : RS_MODE_DIRECT;
        if (p.mode == RS_MODE_BLOCKED) {
            if (lds > pl.lds) pl.lds = lds;
            if (p.nw > pl.max_nw) pl.max_nw = p.nw;
        }
        floats[i] = ((size_t)p.nw * p.K + 63) & ~(size_t)63;
        total += floats[i];
    }
    if (pl.max_nw < 1) pl.max_nw = 1;
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    const size_t head = (sizeof(RsPair) * RS_PLAN_MAX_PAIRS + 255) & ~(size_t)255;
    hipError_t e = hipMalloc((void**)&pl.dev, head + total * sizeof(float));
    if (e != hipSuccess) return ddsp_fail(ctx, DDSP_ERR_OOM, "resample plan hipMalloc", hipGetErrorString(e));
    float* at = (float*)(pl.dev + head);
    for (int i = 0; i < n_pairs; ++i) {
        RsPair& p = pl.host[i];
        if (p.mode == RS_MODE_COPY) continue;
        p.taps = at;
        at += floats[i];
        hipLaunchKernelGGL(resample_taps_kernel, dim3((unsigned)(((int64_t)p.nw * p.K + 255) / 256)), dim3(256), 0, st,
                           (float*)p.taps, p.orig, p.nw, p.width, p.K, base[i], (double)lowpass_filter_width);
    }
    // the plan may be used on any stream of the device afterwards: wait for the tables here, once
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(pl.dev, pl.host, sizeof(RsPair) * RS_PLAN_MAX_PAIRS, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(pl.dev);
        return ddsp_fail(ctx, DDSP_ERR_HIP, "resample plan tables", hipGetErrorString(e));
    }
    *plan = new ddsp_resample_plan(pl);
    return DDSP_OK;
}

extern "C" void ddsp_resample_keyed_plan_destroy(ddsp_resample_plan* plan) {
    if (!plan) return;
    ddsp_device_guard guard;
    if (guard.enter(plan->device) == hipSuccess) (void)hipFree(plan->dev);   // (hipFree waits for kernels that read the tables)
    delete plan;
}

extern "C" int64_t ddsp_resample_keyed_length(const ddsp_resample_plan* plan, int64_t T) {
    if (!plan || T < 0) return -1;
    int64_t best = 0;
    for (int i = 0; i < plan->n_pairs; ++i) {
        const int64_t n = ddsp_resample_length(T, plan->orig_freq[i], plan->new_freq[i]);
        if (n > best) best = n;
    }
    return best;
}

extern "C" int ddsp_resample_keyed(ddsp_ctx* ctx, void* stream, const ddsp_resample_plan* plan, const float* x, int64_t B, int64_t T,
                                   const int32_t* n_samples, const int32_t* key, float* out) {
    DDSP_REQUIRE(ctx, ctx && plan && x && out && n_samples && key, "ddsp_resample_keyed: null argument");
    DDSP_REQUIRE(ctx, plan->device == ctx->device, "ddsp_resample_keyed: the plan lives on another device");
    DDSP_REQUIRE(ctx, B >= 0 && B < 65536 && T >= 1, "ddsp_resample_keyed: bad argument");
    if (B == 0) return DDSP_OK;
    const int64_t T_out = ddsp_resample_keyed_length(plan, T);
    // the grid of the largest pair: every blocked pair's frames over the padded width, RS_RB to a workgroup
    int64_t gy = 1;
    for (int i = 0; i < plan->n_pairs; ++i) {
        const RsPair& p = plan->host[i];
        if (p.mode != RS_MODE_BLOCKED) continue;
        const int64_t groups = ceil_div64(ceil_div64(T_out, p.nw), RS_RB);
        if (groups > gy) gy = groups;
    }
    DDSP_REQUIRE(ctx, gy < 65536, "ddsp_resample_keyed: rows too long for one launch");
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(resample_keyed_kernel, dim3((unsigned)((plan->max_nw + 255) / 256), (unsigned)gy, (unsigned)B), dim3(256),
                       plan->lds, st, x, (const RsPair*)plan->dev, plan->n_pairs, T, T_out, out, n_samples, key);
    ddsp_prof_end(ctx, st, 0.0, 4.0 * (B * T + B * T_out));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
