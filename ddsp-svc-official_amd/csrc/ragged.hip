// Ragged batches: what a padded (B, Fr, ...) batch with per-row frame counts n_b needs AROUND the synthesis kernels so that
// every row comes out as if it had been rendered alone at its own length.
//
// The DSP kernels (phase scan, sinusoid bank, frame-varying FIR, spectral OLA) look past a row's end in three ways only:
//   * a frame-rate series is interpolated towards frame min(i + 1, Fr - 1), and frame Fr reuses the filters of frame Fr - 1;
//   * a sample-rate input is read past the row's last sample (filter tails, the half-overlapped last frame);
//   * they write all Fr * hop samples.
// A row whose frame-rate inputs HOLD frame n_b - 1 over its padding, whose sample-rate inputs are 0 from sample n_b * hop
// on and whose outputs are cropped there is therefore computed exactly as the same kernels compute it alone with Fr = n_b:
// x[min(i + 1, n_b - 1)] and x[i + 1] are the same value, a zero sample and a sample that is not there add the same
// nothing.  The kernels below put a batch into that form.  All of them SELECT (`i < n ? x : fill`), never multiply by a
// mask: what the caller left in the padding (NaN, infinities, f0 <= 0) is never read into arithmetic.
// The places where the control network looks across frames take the counts themselves (unit2ctrl_fwd.hip,
// performer_attn*.hip).
#include "common.h"

namespace {

// dst[b][i][:] = i < n_b ? src[b][i][:] : (hold ? src[b][n_b - 1][:] : 0).  In place (dst == src) is fine: the held row is
// only ever rewritten with its own values - which is why src and dst are not declared __restrict__.
__global__ void __launch_bounds__(256) ragged_frames_kernel(const float* src, const int* __restrict__ n_frames,
                                                            int64_t B, int Fr, int C, int hold, float* dst) {
    const int64_t total = B * Fr * C;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int c = (int)(idx % C);
        const int64_t row = idx / C;
        const int i = (int)(row % Fr);
        const int64_t b = row / Fr;
        const int n = ddsp_row_frames(n_frames, b, Fr);
        float v = 0.f;
        if (i < n)
            v = src[idx];
        else if (hold)
            v = src[(b * Fr + (n - 1)) * C + c];
        dst[idx] = v;
    }
}

// The adjoint of the held form, in place on a gradient d (B, Fr, C): frame n_b - 1 was read by every frame behind it, so
// d[b][n_b - 1][:] += sum_{i >= n_b} d[b][i][:], and the padding frames themselves were never an input: d[b][i >= n_b][:] = 0.
// One thread per (row, column) walks the frames in ascending order ((d[n-1] + d[n]) + d[n+1] ...): the same bits on every run.
__global__ void __launch_bounds__(256) ragged_frames_adjoint_kernel(float* __restrict__ d, const int* __restrict__ n_frames,
                                                                    int64_t B, int Fr, int C) {
    const int64_t total = B * C;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / C;
        const int c = (int)(idx - b * C);
        const int n = ddsp_row_frames(n_frames, b, Fr);
        if (n == Fr) continue;
        float* col = d + b * Fr * C + c;
        float acc = col[(int64_t)(n - 1) * C];
        for (int i = n; i < Fr; ++i) {
            acc += col[(int64_t)i * C];
            col[(int64_t)i * C] = 0.f;
        }
        col[(int64_t)(n - 1) * C] = acc;
    }
}

// x[b][t] = 0 for t >= n_b * hop, in up to three (B, Fr * hop) signals; hop % 4 == 0 and 16-byte aligned rows
struct CropArgs {
    float* x[3];
};
__global__ void __launch_bounds__(256) ragged_crop_kernel(CropArgs a, const int* __restrict__ n_frames, int64_t B, int Fr, int hop) {
    const int64_t T4 = (int64_t)Fr * hop / 4, total = B * T4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / T4, t4 = idx - b * T4;
        if (4 * t4 < (int64_t)ddsp_row_frames(n_frames, b, Fr) * hop) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (a.x[k]) ((f32x4*)a.x[k])[idx] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// The unit-noise draw U[0, 1) of a ragged batch, as the synthesis kernels take an injected one (DDSP_EXC_UNIT_NOISE: they
// form 2u - 1): inside a row the caller's draw, or the counter hash of (seed, b, t) (`ddsp_hash32`, as the FIR kernel's
// generator); 0.5 past the row's end, which 2u - 1 turns into exactly 0.
__device__ __forceinline__ float ragged_unit_noise(uint64_t seed, uint64_t idx) {
    return (float)(ddsp_hash32(seed, idx) >> 8) * (1.0f / 16777216.0f);
}
__global__ void __launch_bounds__(256) ragged_noise_kernel(const float* __restrict__ noise, uint64_t seed,
                                                           const int* __restrict__ n_frames, int64_t B, int Fr, int hop,
                                                           float* __restrict__ out) {
    const int64_t T = (int64_t)Fr * hop, total = B * T;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t b = idx / T, t = idx - b * T;
        float v = 0.5f;
        if (t < (int64_t)ddsp_row_frames(n_frames, b, Fr) * hop) v = noise ? noise[idx] : ragged_unit_noise(seed, (uint64_t)idx);
        out[idx] = v;
    }
}

unsigned ragged_grid(int64_t total) {
    int64_t g = ceil_div64(total, 256);
    return (unsigned)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int ddsp_ragged_frames(ddsp_ctx* ctx, void* stream, const float* src, const int32_t* n_frames, int64_t B,
                                  int64_t Fr, int64_t C, int hold, float* dst) {
    DDSP_REQUIRE(ctx, ctx && src && n_frames && dst, "ddsp_ragged_frames: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && Fr >= 1 && C >= 1 && Fr < (1 << 24) && C < (1 << 24), "ddsp_ragged_frames: bad shape");
    if (B == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(ragged_frames_kernel, dim3(ragged_grid(B * Fr * C)), dim3(256), 0, st, src, (const int*)n_frames, B,
                       (int)Fr, (int)C, hold, dst);
    ddsp_prof_end(ctx, st, 0.0, 8.0 * B * Fr * C);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_ragged_frames_adjoint(ddsp_ctx* ctx, void* stream, float* d, const int32_t* n_frames, int64_t B, int64_t Fr,
                                          int64_t C) {
    DDSP_REQUIRE(ctx, ctx && d && n_frames, "ddsp_ragged_frames_adjoint: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && Fr >= 1 && C >= 1 && Fr < (1 << 24) && C < (1 << 24), "ddsp_ragged_frames_adjoint: bad shape");
    if (B == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(ragged_frames_adjoint_kernel, dim3(ragged_grid(B * C)), dim3(256), 0, st, d, (const int*)n_frames, B, (int)Fr,
                       (int)C);
    ddsp_prof_end(ctx, st, 0.0, 8.0 * B * Fr * C);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_ragged_crop(ddsp_ctx* ctx, void* stream, float* x0, float* x1, float* x2, const int32_t* n_frames,
                                int64_t B, int64_t Fr, int hop) {
    DDSP_REQUIRE(ctx, ctx && x0 && n_frames, "ddsp_ragged_crop: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && Fr >= 1 && hop >= 4 && hop % 4 == 0 && Fr * (int64_t)hop < (1 << 28), "ddsp_ragged_crop: bad shape (hop % 4 == 0)");
    DDSP_REQUIRE(ctx, (((uintptr_t)x0 | (uintptr_t)x1 | (uintptr_t)x2) % 16) == 0, "ddsp_ragged_crop: signals must be 16-byte aligned");
    if (B == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(ragged_crop_kernel, dim3(ragged_grid(B * Fr * hop / 4)), dim3(256), 0, st, CropArgs{{x0, x1, x2}},
                       (const int*)n_frames, B, (int)Fr, hop);
    ddsp_prof_end(ctx, st, 0.0, 4.0 * B * Fr * hop);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_ragged_noise(ddsp_ctx* ctx, void* stream, const float* noise, uint64_t noise_seed, const int32_t* n_frames,
                                 int64_t B, int64_t Fr, int hop, float* out) {
    DDSP_REQUIRE(ctx, ctx && n_frames && out, "ddsp_ragged_noise: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && Fr >= 1 && hop >= 1 && Fr * (int64_t)hop < (1 << 28), "ddsp_ragged_noise: bad shape");
    if (B == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(ragged_noise_kernel, dim3(ragged_grid(B * Fr * hop)), dim3(256), 0, st, noise, noise_seed,
                       (const int*)n_frames, B, (int)Fr, hop, out);
    ddsp_prof_end(ctx, st, 0.0, 8.0 * B * Fr * hop);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
