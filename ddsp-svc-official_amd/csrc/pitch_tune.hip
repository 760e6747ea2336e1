// a16: pitch correction (`infer_offline.PitchTune`, offline jobs with a tune, realtime.StreamBank(tune=True)): the f0 of a row
// is pulled toward the notes of a scale, in place, between the analysis (after the key) and the synthesiser.  One launch.
//
// THE RULE (include/ddsp_amd.h at ddsp_f0_tune states it too; tests/pitch_tune_cases.py is the same in numpy fp64).  The owner
// of a row - a job offline, a slot live - has a setting: mask (bit p in 0..11 allows pitch class p, C = 0; only those twelve
// bits count, none of them set: off), a4 Hz, strength s in [0, 1], alpha in (0, 1].  A frame is VOICED when its f0 is finite
// and > 0.  For the frames t < n_b of a row, all in fp64, one rounding per operation, nothing contracted:
//     m_t = 69 + 12 * log2(f_t / a4)
//     n_t = the integer n with bit (n mod 12) of mask set that minimises |n - m_t|, a tie takes the smaller n
//     d_t = n_t - m_t        (|d_t| <= 6; 0 where m_t is not finite, which takes an a4 beyond 1e+-260)
//     c_t = d_t                                  t is the row's first voiced frame, or frame t-1 is unvoiced   (a RESET)
//     c_t = (1 - alpha) * c_(t-1) + alpha * d_t  otherwise
//     out_t = (s * c_t == 0) ? f_t : (float)((double)f_t * exp2(s * c_t / 12))
// Unvoiced frames, frames at or past the row's count, rows whose owner is off (no bit of the mask, or s == 0) and rows whose
// owner index lies outside [0, J) keep their bits: they are never stored.  A setting with a mask whose a4 is not finite or
// not > 0, whose s is outside [0, 1] or whose alpha is outside (0, 1] leaves its rows untouched as well and raises the device
// error word; a setting without a mask is off and is not judged.  No address depends on a setting's value, and the owner index
// is tested before it forms one.
//
// The recurrence is a composition of affine maps c -> A * c + B: a voiced frame behind a voiced one is (1 - alpha, alpha * d),
// a reset is (0, d), an unvoiced frame is (0, 0).  One wave per row, four rows per workgroup, 64 frames per step: every lane
// forms its frame's map, an inclusive shuffle scan composes them ((a2, b2) o (a1, b1) = (a2 * a1, a2 * b1 + b2), six rounds of
// two fp64 shuffles), the carry c of lane 63 reaches the next step by a readlane, and "the previous frame is voiced" crosses the
// step boundary as bit 63 of the step's ballot - taken from the values as they were LOADED, never by reading the row again (a
// voiced frame stays voiced under the rule, so either would do; this one needs no second load).  No thread walks the row:
// a lane sees every 64th frame.  With alpha == 1 every A is exactly 0 and every product above is an exact zero, so c_t is d_t
// bit for bit; otherwise the scan's grouping differs from the serial order by some 1e-15 per composition.
#include "common.h"

#include <cfloat>

namespace {

constexpr int TUNE_WAVES = 4;

__device__ __forceinline__ double readlane63_d(double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)u, 63), hi = __builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), 63);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// d_t of the rule for a voiced frame: the fourteen integers floor(m) - 6 .. floor(m) + 7 hold every candidate within 6 of m,
// ascending, and a strict < keeps the smaller n of a tie
__device__ __forceinline__ double tune_offset(float f, double a4, int mask) {
    const double m = 69.0 + 12.0 * log2((double)f / a4);
    if (!(fabs(m) <= DBL_MAX)) return 0.0;
    const int base = (int)floor(m);                                        // |m| < 2e4 for a finite one
    double best = DBL_MAX, d = 0.0;
#pragma unroll
    for (int k = -6; k <= 7; ++k) {
        const int n = base + k;
        const int pc = ((n % 12) + 12) % 12;
        const double e = (double)n - m;
        if (((mask >> pc) & 1) && fabs(e) < best) {
            best = fabs(e);
            d = e;
        }
    }
    return d;
}

__global__ void __launch_bounds__(64 * TUNE_WAVES) f0_tune_kernel(float* __restrict__ f0, int64_t B, int Fr,
                                                                  const int32_t* __restrict__ n_frames,
                                                                  const int32_t* __restrict__ owner, int64_t J,
                                                                  const int32_t* __restrict__ mask, const double* __restrict__ param,
                                                                  double* __restrict__ corr, int* err) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * TUNE_WAVES + (threadIdx.x >> 6);
    if (row >= B) return;                                                  // (uniform over the wave, as all that follows up to the loop)
    const int64_t j = owner ? (int64_t)owner[row] : row;
    int bits = 0;
    double a4 = 440.0, s = 0.0, alpha = 1.0;
    bool on = j >= 0 && j < J;                                             // tested before any address is formed
    if (on) {
        bits = mask[j] & 0xfff;
        on = bits != 0;
    }
    if (on) {
        a4 = param[3 * j];
        s = param[3 * j + 1];
        alpha = param[3 * j + 2];
        if (!(a4 > 0.0 && a4 <= DBL_MAX) || !(s >= 0.0 && s <= 1.0) || !(alpha > 0.0 && alpha <= 1.0)) {
            if (lane == 0) __hip_atomic_store(err, DDSP_DEV_ERR_TUNE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            on = false;
        } else if (s == 0.0) {
            on = false;
        }
    }
    float* __restrict__ x = f0 + row * Fr;
    double* __restrict__ c_out = corr ? corr + row * Fr : nullptr;
    if (!on) {                                                             // the row keeps its bits; its corrections are 0
        if (c_out)
            for (int t = lane; t < Fr; t += 64) c_out[t] = 0.0;
        return;
    }
    const int n = ddsp_row_frames(n_frames, row, Fr);
    const int end = c_out ? Fr : n;                                        // (behind the count only corr is written)
    const double keep = 1.0 - alpha;
    double carry = 0.0;                                                    // c of the frame before this step
    bool carry_voiced = false;                                             // ... and whether that frame is voiced
    for (int t0 = 0; t0 < end; t0 += 64) {
        const int t = t0 + lane;
        float f = 0.0f;
        if (t < n) f = x[t];
        const bool voiced = t < n && f > 0.0f && f <= FLT_MAX;
        const uint64_t ballot = __ballot(voiced);
        const bool after_voiced = lane ? ((ballot >> (lane - 1)) & 1) != 0 : carry_voiced;
        double a = 0.0, b = 0.0;                                           // unvoiced: the map (0, 0)
        if (voiced) {
            const double d = tune_offset(f, a4, bits);
            a = after_voiced ? keep : 0.0;
            b = after_voiced ? alpha * d : d;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                                 // (a, b) o (a', b') of the lane o below
            const double a1 = __shfl_up(a, o, 64), b1 = __shfl_up(b, o, 64);
            if (lane >= o) {
                b = a * b1 + b;
                a = a * a1;
            }
        }
        const double c = a * carry + b;
        carry = readlane63_d(c);
        carry_voiced = ((ballot >> 63) & 1) != 0;
        if (t < Fr) {
            if (c_out) c_out[t] = voiced ? c : 0.0;
            if (voiced) {
                const double sc = s * c;
                if (sc != 0.0) x[t] = (float)((double)f * exp2(sc / 12.0));
            }
        }
    }
}

}  // namespace

extern "C" int ddsp_f0_tune(ddsp_ctx* ctx, void* stream, float* f0, int64_t B, int64_t Fr, const int32_t* n_frames,
                            const int32_t* owner, int64_t J, const int32_t* mask, const double* param, double* corr) {
    DDSP_REQUIRE(ctx, ctx && f0 && mask && param, "ddsp_f0_tune: null argument");
    DDSP_REQUIRE(ctx, B >= 1 && B < (1ll << 31) && Fr >= 1 && Fr < (1ll << 31) && J >= 1 && J < (1ll << 31),
                 "ddsp_f0_tune: bad shape (B, Fr, J >= 1)");
    int rc;
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    DDSP_ENTER_DEVICE(ctx);
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((B + TUNE_WAVES - 1) / TUNE_WAVES);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(f0_tune_kernel, dim3(blocks), dim3(64 * TUNE_WAVES), 0, st, f0, B, (int)Fr, n_frames, owner, J, mask, param,
                       corr, dev_err);
    ddsp_prof_end(ctx, st, 0.0, (double)B * (double)Fr * (corr ? 16.0 : 8.0));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
