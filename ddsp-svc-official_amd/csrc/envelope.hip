// a19: envelope mix (`infer_offline.EnvelopeMix`, offline jobs with an envelope, realtime.StreamBank(envelope=True)): the
// converted output is held to the SOURCE's loudness envelope.  RVC's `change_rms(data1, sr1, data2, sr2, rate)` restated
// (so-vits-svc: "loudness envelope adjustment"); data1 is the source, data2 the output, rate the share of the output's own
// envelope that is kept.  Two entry points: ddsp_envelope_rms (frame RMS of ragged rows) and ddsp_envelope_apply (in place).
//
// THE RULE (include/ddsp_amd.h states it too; tests/envelope_cases.py is the same in numpy fp64), all in fp64, one rounding
// per operation as written, nothing contracted:
//   1. frame RMS as librosa.feature.rms documents it with center=True and 'constant' padding: a row of n samples has
//      N = 1 + n / hop frames, frame i covers [i * hop - win / 2, i * hop + win / 2), samples outside [0, n) count as 0,
//      rms[i] = sqrt(sum x^2 / win), win = m * hop, m even in 2..8;
//   2. both envelopes are interpolated to the output's length n2 as F.interpolate(mode="linear", align_corners=False) does:
//      x = max((t + 0.5) * N / n2 - 0.5, 0), i0 = min(floor(x), N - 1), i1 = min(i0 + 1, N - 1), lam = x - i0,
//      e = (1 - lam) * env[i0] + lam * env[i1];
//   3. e2 = max(e2, 1e-6); g = e1^(1 - rate) * e2^(rate - 1); out[t] = data2[t] * g.
// A row with rate == 1, or without an owner, is selected around: its bits stay and 0^0 is never formed.  e1 == 0 with
// rate < 1 gives a gain of exactly 0 (a silent source silences the output: RVC's behaviour).  A rate that is not finite or
// outside [0, 1], an owner or a source row outside its table, a source count < 1 or a span that leaves the tensor leaves the
// row's bits and raises the device error word.  Every row index, base and count is tested before it forms an address.
//
// RMS.  win = m * hop, so a frame is the sum of m consecutive HOP-BLOCKS [k * hop, (k + 1) * hop) - blocks i - m/2 .. i + m/2 - 1,
// those outside [0, N) are empty - and block N - 1 holds the row's tail (n mod hop samples).  The first kernel forms one fp64
// sum of squares per (row, block), every sample read from memory once: 16-byte loads (four fp32 or two fp64) from the first
// 16-byte boundary at or below the block's start wherever the whole vector lies inside the block, a bounds select at its two
// ends - the padding behind a row's count and between spans is never read.  From a hop of ENV_WIDE_HOP samples on a workgroup
// strides one block (the offline hop of half a second); below it a wave strides a block and a workgroup takes 16 of them (the
// live hop of some hundred samples: a 200 ms window is two workgroups a row, not twenty).  The order of every sum is fixed by
// that shape - a lane's strided terms in ascending order, the xor-butterfly over the wave, ((w0 + w1) + (w2 + w3)) over the
// waves - and there are no floating-point atomics: the same input gives the same bits.  The second kernel forms the frames from
// the block sums in ascending block order.
//
// APPLY.  grid (tiles of 1024 elements, rows).  An element reads its two envelopes straight from memory: a row's envelopes are
// a few KB, every lane of a wave reads the same one or two entries, and they stay in the L1/L2 cache - nothing is staged in the
// LDS.  Two fp64 pow per element; the kernel is bound by the 16 bytes it moves per fp64 element.
#include "common.h"

#include <cfloat>

namespace {

constexpr int ENV_THREADS = 256;
constexpr int ENV_WAVES = ENV_THREADS / 64;
constexpr int ENV_WIDE_HOP = 2048;      // from this hop on a workgroup strides one hop-block
constexpr int ENV_WAVE_BLOCKS = 4;      // below it: hop-blocks per wave, ENV_WAVES * ENV_WAVE_BLOCKS per workgroup
constexpr int ENV_TILE = 4 * ENV_THREADS;

typedef double f64x2 __attribute__((ext_vector_type(2)));

// The rows of a call: an fp32 matrix (R, T) with device counts, or spans (base, count) of an fp64 tensor of `total` elements
struct EnvRows {
    const float* x32;
    int64_t T;
    const int32_t* n32;         // (R,) or null: T for every row
    const double* x64;
    int64_t total;
    const int64_t* spans;       // (R, 2)
};

// -> the row's count (0: nothing of it may be read), `start` its first element; false for a span that leaves the tensor.
// Nothing but the tables is read here, and no address of the signal is formed.
__device__ __forceinline__ bool env_row(const EnvRows& a, int64_t r, int64_t limit, int64_t& start, int64_t& n) {
    if (a.x64 || a.spans) {
        const int64_t base = a.spans[2 * r], count = a.spans[2 * r + 1];
        start = base;
        n = count;
        return base >= 0 && count >= 1 && count <= limit && count <= a.total && base <= a.total - count;
    }
    start = r * a.T;
    n = a.T;
    if (a.n32) {
        const int64_t c = a.n32[r];
        n = c < 0 ? 0 : (c > a.T ? a.T : c);
    }
    return true;
}

__device__ __forceinline__ double sq_d(float v) { return (double)v * (double)v; }   // exact in fp64
__device__ __forceinline__ double sq_d(double v) { return v * v; }

// this thread's share of sum x[j]^2, j in [s0, s1) - a sub-range of the row, s0 <= s1 -, thread `tid` of NT
template <typename T, int NT>
__device__ __forceinline__ double env_sumsq(const T* __restrict__ row, int64_t s0, int64_t s1, int tid) {
    constexpr int V = 16 / (int)sizeof(T);
    const int off = (int)((((uintptr_t)row / sizeof(T)) + (uint64_t)s0) & (V - 1));
    double acc = 0.0;
    for (int64_t s = s0 - off + (int64_t)V * tid; s < s1; s += (int64_t)V * NT) {
        if (s >= s0 && s + V <= s1) {
            if constexpr (V == 4) {
                const f32x4 v = *(const f32x4*)(row + s);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc += sq_d(v[e]);
            } else {
                const f64x2 v = *(const f64x2*)(row + s);
                acc += sq_d(v[0]);
                acc += sq_d(v[1]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int64_t j = s + e;
                if (j >= s0 && j < s1) acc += sq_d(row[j]);
            }
        }
    }
    return acc;
}

struct EnvRmsArgs {
    EnvRows rows;
    int64_t R;
    int hop, m, N_max;
    double* blk;                // (R, N_max): sum of squares per hop-block
    double* env;                // (R, N_max)
    int* err;
};

// grid (N_max or ceil(N_max / 16), R)
template <typename T, bool WIDE>
__global__ void __launch_bounds__(ENV_THREADS) envelope_blocks_kernel(EnvRmsArgs a) {
    __shared__ double part[ENV_WAVES];
    const int64_t r = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t start, n;
    const int64_t limit = (int64_t)a.N_max * a.hop;      // (a longer span has more frames than the envelope holds)
    const bool ok = env_row(a.rows, r, limit + a.hop - 1, start, n) && 1 + n / a.hop <= a.N_max;
    if (!ok) {
        if (blockIdx.x == 0 && tid == 0) __hip_atomic_store(a.err, DDSP_DEV_ERR_ENVELOPE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        n = 0;
    }
    const int N = ok ? (int)(1 + n / a.hop) : 0;
    const T* __restrict__ row = nullptr;
    if (n > 0) {
        if constexpr (sizeof(T) == 4) row = (const T*)a.rows.x32 + start;
        else row = (const T*)a.rows.x64 + start;
    }
    double* __restrict__ out = a.blk + r * a.N_max;
    if constexpr (WIDE) {
        const int k = blockIdx.x;
        double acc = 0.0;
        if (k < N) {
            const int64_t s0 = (int64_t)k * a.hop, s1 = s0 + a.hop < n ? s0 + a.hop : n;
            if (s0 < s1) acc = env_sumsq<T, ENV_THREADS>(row, s0, s1, tid);
        }
        acc = wave_sum_d(acc);
        if (lane == 0) part[wave] = acc;
        __syncthreads();
        if (tid == 0) out[k] = (part[0] + part[1]) + (part[2] + part[3]);
    } else {
#pragma unroll 1
        for (int i = 0; i < ENV_WAVE_BLOCKS; ++i) {
            const int k = (blockIdx.x * ENV_WAVES + wave) * ENV_WAVE_BLOCKS + i;
            if (k >= a.N_max) break;
            double acc = 0.0;
            if (k < N) {
                const int64_t s0 = (int64_t)k * a.hop, s1 = s0 + a.hop < n ? s0 + a.hop : n;
                if (s0 < s1) acc = env_sumsq<T, 64>(row, s0, s1, lane);
            }
            acc = wave_sum_d(acc);
            if (lane == 0) out[k] = acc;
        }
    }
}

// one thread per (row, frame): the m block sums of the frame in ascending order; 0 behind the row's frames
__global__ void __launch_bounds__(ENV_THREADS) envelope_frames_kernel(EnvRmsArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * ENV_THREADS + threadIdx.x;
    if (idx >= a.R * a.N_max) return;
    const int64_t r = idx / a.N_max;
    const int i = (int)(idx - r * a.N_max);
    int64_t start, n;
    const bool ok = env_row(a.rows, r, (int64_t)a.N_max * a.hop + a.hop - 1, start, n) && 1 + n / a.hop <= a.N_max;
    const int N = ok ? (int)(1 + n / a.hop) : 0;
    double v = 0.0;
    if (i < N) {
        const double* __restrict__ b = a.blk + r * a.N_max;
        const int h = a.m / 2;
        const int lo = i - h < 0 ? 0 : i - h, hi = i + h < N ? i + h : N;
        double acc = 0.0;
        for (int k = lo; k < hi; ++k) acc += b[k];
        v = sqrt(acc / (double)((int64_t)a.m * a.hop));
    }
    a.env[idx] = v;
}

struct EnvApplyArgs {
    EnvRows rows;               // the output rows (x32 / x64 are written)
    int64_t R, n_max;
    const double* env2;         // (R, N2_max)
    int N2_max, hop2;
    const double* env1;         // (R_src, N1_max)
    int64_t R_src;
    int N1_max, hop1;
    const int32_t* n_src;       // (R_src,) or null: n_src_all
    int64_t n_src_all;
    const int32_t* src_of_row;  // (R,) or null: row r
    const int32_t* owner;       // (R,) or null: row r
    const double* rate;         // (J,)
    int64_t J;
    int* err;
};

__device__ __forceinline__ double env_at(const double* __restrict__ env, int N, double t05, double n2) {
    const double x = fmax(t05 * (double)N / n2 - 0.5, 0.0);
    const int f = (int)floor(x);
    const int i0 = f < N - 1 ? f : N - 1;
    const int i1 = i0 + 1 < N - 1 ? i0 + 1 : N - 1;
    const double lam = x - (double)i0;
    return (1.0 - lam) * env[i0] + lam * env[i1];
}

template <typename T>
__global__ void __launch_bounds__(ENV_THREADS) envelope_apply_kernel(EnvApplyArgs a) {
    const int64_t r = blockIdx.y;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    // everything up to the loop is uniform over the workgroup
    const int64_t j = a.owner ? (int64_t)a.owner[r] : r;
    if (a.owner && j == -1) return;                                          // a padding row: no owner, no error
    bool bad = j < 0 || j >= a.J;
    double rate = 1.0;
    if (!bad) {
        rate = a.rate[j];
        bad = !(rate >= 0.0 && rate <= 1.0);                                 // (a NaN fails both)
    }
    if (!bad && rate == 1.0) return;                                         // off: selected around
    int64_t s = 0, n1 = 0, start = 0, n2 = 0;
    if (!bad) {
        s = a.src_of_row ? (int64_t)a.src_of_row[r] : r;
        bad = s < 0 || s >= a.R_src;
    }
    if (!bad) {
        n1 = a.n_src ? (int64_t)a.n_src[s] : a.n_src_all;
        bad = n1 < 1;
    }
    if (!bad) bad = !env_row(a.rows, r, a.n_max, start, n2);
    if (bad) {
        if (first) __hip_atomic_store(a.err, DDSP_DEV_ERR_ENVELOPE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    if (n2 < 1) return;                                                      // (a matrix row with a count of 0)
    int64_t N1l = 1 + n1 / a.hop1, N2l = 1 + n2 / a.hop2;                    // (the host has sized env2 for n_max)
    const int N1 = (int)(N1l < a.N1_max ? N1l : a.N1_max), N2 = (int)(N2l < a.N2_max ? N2l : a.N2_max);
    const double* __restrict__ e1 = a.env1 + s * a.N1_max;
    const double* __restrict__ e2 = a.env2 + r * a.N2_max;
    const double up = 1.0 - rate, down = rate - 1.0, n2d = (double)n2;
    T* __restrict__ y;
    if constexpr (sizeof(T) == 4) y = (T*)a.rows.x32 + start;
    else y = (T*)a.rows.x64 + start;
    const int64_t t0 = (int64_t)blockIdx.x * ENV_TILE + threadIdx.x;
#pragma unroll
    for (int e = 0; e < ENV_TILE / ENV_THREADS; ++e) {
        const int64_t t = t0 + (int64_t)e * ENV_THREADS;
        if (t >= n2) break;
        const double t05 = (double)t + 0.5;
        const double v1 = env_at(e1, N1, t05, n2d);
        const double v2 = fmax(env_at(e2, N2, t05, n2d), 1e-6);
        const double g = pow(v1, up) * pow(v2, down);
        y[t] = (T)((double)y[t] * g);
    }
}

}  // namespace

static int env_rows_check(ddsp_ctx* ctx, const void* x32, int64_t T, const void* x64, int64_t total, const int64_t* spans,
                          int64_t R) {
    DDSP_REQUIRE(ctx, (x32 != nullptr) != (x64 != nullptr), "ddsp_envelope: exactly one of the fp32 matrix and the fp64 tensor");
    DDSP_REQUIRE(ctx, R >= 1 && R <= 65535, "ddsp_envelope: bad row count (1 <= R <= 65535)");
    if (x32) DDSP_REQUIRE(ctx, T >= 1 && T < (1ll << 40) && !spans, "ddsp_envelope: the fp32 form takes T >= 1 and no spans");
    else DDSP_REQUIRE(ctx, total >= 1 && spans, "ddsp_envelope: the fp64 form takes total >= 1 and a span table");
    return DDSP_OK;
}

extern "C" int ddsp_envelope_rms(ddsp_ctx* ctx, void* stream, const float* x32, int64_t T, const int32_t* n_samples,
                                 const double* x64, int64_t total, const int64_t* spans, int64_t R, int64_t hop, int m,
                                 int64_t N_max, double* blocks, double* env) {
    DDSP_REQUIRE(ctx, ctx && blocks && env, "ddsp_envelope_rms: null argument");
    int rc;
    if ((rc = env_rows_check(ctx, x32, T, x64, total, spans, R))) return rc;
    DDSP_REQUIRE(ctx, hop >= 1 && hop <= (1ll << 27), "ddsp_envelope_rms: bad hop (1 <= hop <= 2^27)");
    DDSP_REQUIRE(ctx, m >= 2 && m <= 8 && m % 2 == 0, "ddsp_envelope_rms: m must be 2, 4, 6 or 8 (win = m * hop)");
    DDSP_REQUIRE(ctx, N_max >= 1 && N_max < (1ll << 30) && (!x32 || N_max >= 1 + T / hop),
                 "ddsp_envelope_rms: bad N_max (the fp32 form needs N_max >= 1 + T / hop)");
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    DDSP_ENTER_DEVICE(ctx);
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;
    hipStream_t st = (hipStream_t)stream;
    EnvRmsArgs a;
    a.rows = EnvRows{x32, T, n_samples, x64, total, spans};
    a.R = R;
    a.hop = (int)hop;
    a.m = m;
    a.N_max = (int)N_max;
    a.blk = blocks;
    a.env = env;
    a.err = dev_err;
    const bool wide = hop >= ENV_WIDE_HOP;
    const dim3 grid((unsigned)(wide ? N_max : ceil_div64(N_max, ENV_WAVES * ENV_WAVE_BLOCKS)), (unsigned)R);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    if (x32) {
        if (wide) hipLaunchKernelGGL((envelope_blocks_kernel<float, true>), grid, dim3(ENV_THREADS), 0, st, a);
        else hipLaunchKernelGGL((envelope_blocks_kernel<float, false>), grid, dim3(ENV_THREADS), 0, st, a);
    } else {
        if (wide) hipLaunchKernelGGL((envelope_blocks_kernel<double, true>), grid, dim3(ENV_THREADS), 0, st, a);
        else hipLaunchKernelGGL((envelope_blocks_kernel<double, false>), grid, dim3(ENV_THREADS), 0, st, a);
    }
    hipLaunchKernelGGL(envelope_frames_kernel, dim3((unsigned)ceil_div64(R * N_max, ENV_THREADS)), dim3(ENV_THREADS), 0, st, a);
    // (an upper bound for ragged rows: the full width of the matrix, or N_max hops of every span)
    const double samples = x32 ? (double)R * (double)T : (double)R * (double)N_max * (double)hop;
    ddsp_prof_end(ctx, st, 2.0 * samples, samples * (x32 ? 4.0 : 8.0) + (double)R * (double)N_max * (8.0 + 8.0 * (m + 1)));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_envelope_apply(ddsp_ctx* ctx, void* stream, double* y64, int64_t total, const int64_t* spans, float* y32,
                                   int64_t T, const int32_t* n_out, int64_t R, int64_t n_max, const double* env_out,
                                   int64_t N_out_max, int64_t hop_out, const double* env_src, int64_t R_src, int64_t N_src_max,
                                   int64_t hop_src, const int32_t* n_src, int64_t n_src_all, const int32_t* src_of_row,
                                   const int32_t* owner, const double* rate, int64_t J) {
    DDSP_REQUIRE(ctx, ctx && env_out && env_src && rate, "ddsp_envelope_apply: null argument");
    int rc;
    if ((rc = env_rows_check(ctx, y32, T, y64, total, spans, R))) return rc;
    DDSP_REQUIRE(ctx, hop_out >= 1 && hop_out <= (1ll << 27) && hop_src >= 1 && hop_src <= (1ll << 27),
                 "ddsp_envelope_apply: bad hop (1 <= hop <= 2^27)");
    DDSP_REQUIRE(ctx, n_max >= 1 && n_max < (1ll << 40) && (!y32 || n_max == T), "ddsp_envelope_apply: bad n_max (the fp32 form: T)");
    DDSP_REQUIRE(ctx, N_out_max >= 1 + n_max / hop_out && N_out_max < (1ll << 30),
                 "ddsp_envelope_apply: the output's envelope must hold 1 + n_max / hop_out frames");
    DDSP_REQUIRE(ctx, R_src >= 1 && R_src < (1ll << 31) && N_src_max >= 1 && N_src_max < (1ll << 30) && J >= 1 && J < (1ll << 31),
                 "ddsp_envelope_apply: bad shape (R_src, N_src_max, J >= 1)");
    DDSP_REQUIRE(ctx, n_src || (n_src_all >= 1 && N_src_max >= 1 + n_src_all / hop_src),
                 "ddsp_envelope_apply: without source counts, n_src_all >= 1 samples whose frames the source's envelope holds");
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    DDSP_ENTER_DEVICE(ctx);
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;
    hipStream_t st = (hipStream_t)stream;
    EnvApplyArgs a;
    a.rows = EnvRows{y32, T, n_out, y64, total, spans};
    a.R = R;
    a.n_max = n_max;
    a.env2 = env_out;
    a.N2_max = (int)N_out_max;
    a.hop2 = (int)hop_out;
    a.env1 = env_src;
    a.R_src = R_src;
    a.N1_max = (int)N_src_max;
    a.hop1 = (int)hop_src;
    a.n_src = n_src;
    a.n_src_all = n_src_all;
    a.src_of_row = src_of_row;
    a.owner = owner;
    a.rate = rate;
    a.J = J;
    a.err = dev_err;
    const dim3 grid((unsigned)ceil_div64(n_max, ENV_TILE), (unsigned)R);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    if (y32) hipLaunchKernelGGL(envelope_apply_kernel<float>, grid, dim3(ENV_THREADS), 0, st, a);
    else hipLaunchKernelGGL(envelope_apply_kernel<double>, grid, dim3(ENV_THREADS), 0, st, a);
    ddsp_prof_end(ctx, st, 0.0, (double)R * (double)n_max * (y32 ? 8.0 : 16.0));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
