// a14: the row movers of a stream bank's active set (realtime.StreamBank, `active=`): a call that advances only A of the S slots
// runs them as a compact batch of W >= A rows.  A device row table `rows` (W) int32 says which slot every compact row is
// (-1: padding).  ddsp_bank_gather pushes the new blocks into the named slots' windows and copies what the chain reads of a slot
// (the pushed window, the SOLA buffer, the speaker mix, the pitch, the enhancer's key request) to the compact row;
// ddsp_bank_scatter brings the spliced SOLA buffers back.  The table is device data: a captured graph reads it at replay time,
// so the active set changes by one small upload, and nothing is ever read back.
// An entry is bounds-tested against S before it forms an address; one outside [0, S) is padding.  A slot not named in `rows`
// is neither read nor written.
//
// The row movers of a bank with a model per slot (`models=`): the analysis runs once over the call's R rows, then every model
// renders its own rows as a compact batch of W rows.  Here `rows` (W) indexes the CALL'S row batch, not slots.
// ddsp_bank_features_gather copies the units, f0, volume, injected noise and speaker mix of the named rows to the compact
// tensors in one launch (padding: zeros, speaker 1 with weight 1); ddsp_bank_signal_scatter writes the gated signal of every
// real compact row into the call's (R, T) signal.
#include "common.h"

#include <algorithm>

namespace {

// 16-byte path: V = 4 floats per access where every row starts on a 16-byte boundary and every length is a multiple of 4
// (the entry point decides), else V = 1.  Plain vector loads and stores either way.
template <int V> struct row_vec { typedef float type; };
template <> struct row_vec<4> { typedef f32x4 type; };

// dst[0, n) = src[0, n) by the gridDim.x workgroups of a row (n a multiple of V)
template <int V>
__device__ __forceinline__ void row_copy(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
    typedef typename row_vec<V>::type T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n / V; i += (int64_t)gridDim.x * 256)
        ((T*)dst)[i] = ((const T*)src)[i];
}

// the slot of compact row r, or -1 for padding (an entry outside [0, S) included)
__device__ __forceinline__ int bank_slot(const int32_t* __restrict__ rows, int r, int S) {
    const int s = rows[r];
    return s >= 0 && s < S ? s : -1;
}

// Launch 1 of the gather (grid (x, W)): cwindow[r] = append(window[s][block:], block_in[r]) - the pushed window, written
// OUTSIDE the windows, so no workgroup reads what another writes - and the compact rows of the small tables.  Padding: a
// zero window and buffer, speaker 1 with weight 1, pitch 1, key request 0.
template <int V>
__global__ void __launch_bounds__(256) bank_gather_kernel(const int32_t* __restrict__ rows, int S, const float* __restrict__ window,
                                                          int64_t n_in, const float* __restrict__ block_in, int64_t block,
                                                          float* __restrict__ cwindow, const float* __restrict__ sola, int xfade,
                                                          float* __restrict__ csola, const int32_t* __restrict__ mix_ids,
                                                          const float* __restrict__ mix_w, int K, int32_t* __restrict__ cmix_ids,
                                                          float* __restrict__ cmix_w, const float* __restrict__ pitch,
                                                          float* __restrict__ cpitch, const int32_t* __restrict__ request,
                                                          int32_t* __restrict__ crequest) {
    typedef typename row_vec<V>::type T;
    const int r = blockIdx.y;
    const int s = bank_slot(rows, r, S);
    const int64_t keep = n_in - block;
    float* __restrict__ cw = cwindow + r * n_in;
    float* __restrict__ cs = csola + (int64_t)r * xfade;
    if (s < 0) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_in; i += (int64_t)gridDim.x * 256) cw[i] = 0.f;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < xfade; i += (int64_t)gridDim.x * 256) cs[i] = 0.f;
    } else {
        const T* __restrict__ old = (const T*)(window + s * n_in + block);
        const T* __restrict__ neu = (const T*)(block_in + r * block);
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_in / V; i += (int64_t)gridDim.x * 256)
            ((T*)cw)[i] = i < keep / V ? old[i] : neu[i - keep / V];
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < xfade; i += (int64_t)gridDim.x * 256)
            cs[i] = sola[(int64_t)s * xfade + i];
    }
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < K) {
            cmix_ids[r * K + threadIdx.x] = s < 0 ? 1 : mix_ids[s * K + threadIdx.x];
            cmix_w[r * K + threadIdx.x] = s < 0 ? (threadIdx.x == 0 ? 1.f : 0.f) : mix_w[s * K + threadIdx.x];
        }
        if (threadIdx.x == 64) cpitch[r] = s < 0 ? 1.f : pitch[s];
        if (threadIdx.x == 128 && request) crequest[r] = s < 0 ? 0 : request[s];
    }
}

// Launch 2 of the gather (stream order: after every read of launch 1): window[s] = cwindow[r].  Together the two launches are
// the shift of ddsp_stream_push with the compact window as the staging copy; no launch reads what it writes.
template <int V>
__global__ void __launch_bounds__(256) bank_rows_back_kernel(const int32_t* __restrict__ rows, int S, const float* __restrict__ crow,
                                                             int64_t n, float* __restrict__ row) {
    const int r = blockIdx.y;
    const int s = bank_slot(rows, r, S);
    if (s < 0) return;
    row_copy<V>(row + s * n, crow + r * n, n);
}

// n floats of one row: dst = src, or zeros when src is null (a padding row); 16-byte accesses when `vec` (the entry point
// decides per segment), single words otherwise
__device__ __forceinline__ void seg_move(float* __restrict__ dst, const float* __restrict__ src, int64_t n, bool vec) {
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if (vec) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        for (int64_t i = first; i < n / 4; i += step) ((f32x4*)dst)[i] = src ? ((const f32x4*)src)[i] : zero;
    } else {
        for (int64_t i = first; i < n; i += step) dst[i] = src ? src[i] : 0.f;
    }
}

enum { VEC_UNITS = 1, VEC_FRAMES = 2, VEC_NOISE = 4 };

// The one launch of the features gather (grid (x, W)): compact row r takes what the synthesiser reads of row s = rows[r] of the
// call's batch.  The compact tensors lie outside the batch (the entry point checks it), so nothing is read that is written.
__global__ void __launch_bounds__(256) bank_features_gather_kernel(
    const int32_t* __restrict__ rows, int R, int64_t n_units, int64_t Fr, int64_t T, int vec, const float* __restrict__ units,
    const float* __restrict__ f0, const float* __restrict__ volume, const float* __restrict__ noise,
    const int32_t* __restrict__ mix_ids, const float* __restrict__ mix_w, int K, float* __restrict__ cunits,
    float* __restrict__ cf0, float* __restrict__ cvolume, float* __restrict__ cnoise, int32_t* __restrict__ cmix_ids,
    float* __restrict__ cmix_w) {
    const int r = blockIdx.y;
    const int s = bank_slot(rows, r, R);                         // tested before any address of the batch is formed
    const bool real = s >= 0;
    seg_move(cunits + r * n_units, real ? units + s * n_units : nullptr, n_units, vec & VEC_UNITS);
    seg_move(cf0 + r * Fr, real ? f0 + s * Fr : nullptr, Fr, vec & VEC_FRAMES);
    seg_move(cvolume + r * Fr, real ? volume + s * Fr : nullptr, Fr, vec & VEC_FRAMES);
    if (cnoise) seg_move(cnoise + r * T, real ? noise + s * T : nullptr, T, vec & VEC_NOISE);
    if (blockIdx.x == 0 && (int)threadIdx.x < K) {
        cmix_ids[r * K + threadIdx.x] = real ? mix_ids[s * K + threadIdx.x] : 1;
        cmix_w[r * K + threadIdx.x] = real ? mix_w[s * K + threadIdx.x] : (threadIdx.x == 0 ? 1.f : 0.f);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// [a, a + na) and [b, b + nb) share no element
bool apart(const float* a, int64_t na, const float* b, int64_t nb) { return a + na <= b || b + nb <= a; }

// row[rows[r]] = crow[r] (n floats each) for every compact row that is no padding: the body of both scatters
int rows_back(ddsp_ctx* ctx, hipStream_t st, const int32_t* rows, int W, int S, const float* crow, int64_t n, float* row) {
    DDSP_ENTER_DEVICE(ctx);
    const bool vec = n % 4 == 0 && aligned16(crow) && aligned16(row);
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(n, vec ? 1024 : 256), 1024);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    if (vec)
        hipLaunchKernelGGL(bank_rows_back_kernel<4>, dim3(gx, W), dim3(256), 0, st, rows, S, crow, n, row);
    else
        hipLaunchKernelGGL(bank_rows_back_kernel<1>, dim3(gx, W), dim3(256), 0, st, rows, S, crow, n, row);
    ddsp_prof_end(ctx, st, 0.0, 8.0 * W * (double)n);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

}  // namespace

extern "C" int ddsp_bank_gather(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int S, float* window, int64_t n_in,
                                const float* block_in, int64_t block, float* cwindow, const float* sola_buffer, int xfade,
                                float* csola, const int32_t* mix_ids, const float* mix_w, int K, int32_t* cmix_ids, float* cmix_w,
                                const float* pitch, float* cpitch, const int32_t* request, int32_t* crequest) {
    DDSP_REQUIRE(ctx, ctx && rows && window && block_in && cwindow && sola_buffer && csola && mix_ids && mix_w && cmix_ids && cmix_w &&
                          pitch && cpitch && (request == nullptr) == (crequest == nullptr),
                 "ddsp_bank_gather: null argument");
    DDSP_REQUIRE(ctx, S >= 1 && S <= DDSP_MAX_STREAMS && W >= 1 && W <= S, "ddsp_bank_gather: 1 <= W <= S <= 4096");
    DDSP_REQUIRE(ctx, block >= 1 && block < n_in && n_in < ((int64_t)1 << 31), "ddsp_bank_gather: 1 <= block < n_in < 2^31");
    DDSP_REQUIRE(ctx, xfade >= 1 && K >= 1 && K <= 16, "ddsp_bank_gather: xfade >= 1, 1 <= K <= 16");
    DDSP_REQUIRE(ctx, apart(cwindow, W * n_in, window, S * n_in) && apart(block_in, W * block, window, S * n_in) &&
                          apart(block_in, W * block, cwindow, W * n_in) && apart(csola, (int64_t)W * xfade, sola_buffer, (int64_t)S * xfade),
                 "ddsp_bank_gather: the compact rows and the blocks lie outside the bank's rows and each other");
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    const bool vec = n_in % 4 == 0 && block % 4 == 0 && aligned16(window) && aligned16(block_in) && aligned16(cwindow);
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(n_in, vec ? 1024 : 256), 1024);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    if (vec) {
        hipLaunchKernelGGL(bank_gather_kernel<4>, dim3(gx, W), dim3(256), 0, st, rows, S, (const float*)window, n_in, block_in, block,
                           cwindow, sola_buffer, xfade, csola, mix_ids, mix_w, K, cmix_ids, cmix_w, pitch, cpitch, request, crequest);
        hipLaunchKernelGGL(bank_rows_back_kernel<4>, dim3(gx, W), dim3(256), 0, st, rows, S, (const float*)cwindow, n_in, window);
    } else {
        hipLaunchKernelGGL(bank_gather_kernel<1>, dim3(gx, W), dim3(256), 0, st, rows, S, (const float*)window, n_in, block_in, block,
                           cwindow, sola_buffer, xfade, csola, mix_ids, mix_w, K, cmix_ids, cmix_w, pitch, cpitch, request, crequest);
        hipLaunchKernelGGL(bank_rows_back_kernel<1>, dim3(gx, W), dim3(256), 0, st, rows, S, (const float*)cwindow, n_in, window);
    }
    ddsp_prof_end(ctx, st, 0.0, 4.0 * W * (4.0 * n_in + 2.0 * xfade));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_bank_scatter(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int S, const float* csola, int xfade,
                                 float* sola_buffer) {
    DDSP_REQUIRE(ctx, ctx && rows && csola && sola_buffer, "ddsp_bank_scatter: null argument");
    DDSP_REQUIRE(ctx, S >= 1 && S <= DDSP_MAX_STREAMS && W >= 1 && W <= S && xfade >= 1, "ddsp_bank_scatter: 1 <= W <= S <= 4096, xfade >= 1");
    DDSP_REQUIRE(ctx, apart(csola, (int64_t)W * xfade, sola_buffer, (int64_t)S * xfade),
                 "ddsp_bank_scatter: the compact buffers lie outside the bank's");
    return rows_back(ctx, (hipStream_t)stream, rows, W, S, csola, xfade, sola_buffer);
}

extern "C" int ddsp_bank_features_gather(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int R, int64_t Fr, int64_t C,
                                         int64_t T, const float* units, const float* f0, const float* volume, const float* noise,
                                         const int32_t* mix_ids, const float* mix_w, int K, float* cunits, float* cf0,
                                         float* cvolume, float* cnoise, int32_t* cmix_ids, float* cmix_w) {
    DDSP_REQUIRE(ctx, ctx && rows && units && f0 && volume && mix_ids && mix_w && cunits && cf0 && cvolume && cmix_ids && cmix_w &&
                          (noise == nullptr) == (cnoise == nullptr),
                 "ddsp_bank_features_gather: null argument");
    DDSP_REQUIRE(ctx, R >= 1 && R <= DDSP_MAX_STREAMS && W >= 1 && W <= DDSP_MAX_STREAMS, "ddsp_bank_features_gather: 1 <= W, R <= 4096");
    DDSP_REQUIRE(ctx, Fr >= 1 && C >= 1 && T >= 1 && Fr * C < ((int64_t)1 << 31) && T < ((int64_t)1 << 31),
                 "ddsp_bank_features_gather: 1 <= Fr * C, T < 2^31");
    DDSP_REQUIRE(ctx, K >= 1 && K <= 16, "ddsp_bank_features_gather: 1 <= K <= 16");
    const int64_t n_units = Fr * C;
    DDSP_REQUIRE(ctx, apart(cunits, W * n_units, units, R * n_units) && apart(cf0, W * Fr, f0, R * Fr) &&
                          apart(cvolume, W * Fr, volume, R * Fr) && (!noise || apart(cnoise, W * T, noise, R * T)) &&
                          apart(cmix_w, (int64_t)W * K, mix_w, (int64_t)R * K) &&
                          apart((const float*)cmix_ids, (int64_t)W * K, (const float*)mix_ids, (int64_t)R * K),
                 "ddsp_bank_features_gather: the compact tensors lie outside the batch's");
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    const int vec = (n_units % 4 == 0 && aligned16(units) && aligned16(cunits) ? VEC_UNITS : 0) |
                    (Fr % 4 == 0 && aligned16(f0) && aligned16(cf0) && aligned16(volume) && aligned16(cvolume) ? VEC_FRAMES : 0) |
                    (noise && T % 4 == 0 && aligned16(noise) && aligned16(cnoise) ? VEC_NOISE : 0);
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(std::max(n_units, noise ? T : (int64_t)0), 1024), 1024);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(bank_features_gather_kernel, dim3(gx, W), dim3(256), 0, st, rows, R, n_units, Fr, T, vec, units, f0, volume,
                       noise, mix_ids, mix_w, K, cunits, cf0, cvolume, cnoise, cmix_ids, cmix_w);
    ddsp_prof_end(ctx, st, 0.0, 8.0 * W * (double)(n_units + 2 * Fr + (noise ? T : 0)));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_bank_signal_scatter(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int R, const float* csig, int64_t T,
                                        float* sig) {
    DDSP_REQUIRE(ctx, ctx && rows && csig && sig, "ddsp_bank_signal_scatter: null argument");
    DDSP_REQUIRE(ctx, R >= 1 && R <= DDSP_MAX_STREAMS && W >= 1 && W <= DDSP_MAX_STREAMS && T >= 1 && T < ((int64_t)1 << 31),
                 "ddsp_bank_signal_scatter: 1 <= W, R <= 4096, 1 <= T < 2^31");
    DDSP_REQUIRE(ctx, apart(csig, W * T, sig, R * T), "ddsp_bank_signal_scatter: the compact signal lies outside the batch's");
    return rows_back(ctx, (hipStream_t)stream, rows, W, R, csig, T, sig);
}
