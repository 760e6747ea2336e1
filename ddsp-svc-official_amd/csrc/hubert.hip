// HuBERT units encoders on gfx950: HuBERT-Soft (reference encoder/hubert/model.py `HubertSoft.units`, ddsp/vocoder.py:140-229)
// and the HuBERT-base form of fairseq (`extract_features(..., output_layer=n)` with or without `final_proj`: the reference's
// ContentVec / HuBERT-base classes, ddsp/vocoder.py:231-332).  One network, one body (hubert_run); the base form differs in
// three run-time choices: no input padding, the number of transformer layers, and its attention projections, which arrive
// as three matrices per layer and are packed into the QKV operand with the other prepared weights.
//
// Activations are frame-major (frames x channels) fp32 throughout.  Every contraction but conv0 and the attention is a call of
// the library's GEMM (gemm_f32.h) in the context's product arithmetic:
//   * the strided convolutions are plain GEMMs over OVERLAPPING rows: A(m, k) = x[m * stride * Cin + k], k = tap * Cin + ci,
//     lda = stride * Cin <= K (the LDS-DMA kernel clamps rows to M - 1, so its reads end at x[(M-1)*lda + K - 1], inside the
//     input); the weights are repacked once to (Cout, tap * Cin + ci);
//   * the positional convolution (groups 16, 48 channels, 128 taps, padding 64) is one implicit GEMM per (utterance, group)
//     over a zero-padded group-major copy of the activations: A(m, k) = xg[m * 48 + k], k = tap * 48 + ci, K = 6144;
//     its weight norm (one norm per tap, weight_norm(dim=2)) is folded once into the packed weights.
// The conv0 / GroupNorm front, the LayerNorms and the softmax attention are the kernels of this file.
#include "gemm_f32.h"

#include <algorithm>
#include <math.h>
#include <stddef.h>

namespace {

constexpr int HC = 512;                              // conv channels
constexpr int HD = 768;                              // model width
constexpr int HFF = 3072;                            // feed-forward width
constexpr int HU = 256;                              // units
constexpr int HHEADS = 12, HDH = 64;                 // heads x head dim
constexpr int POS_K = 128, POS_G = 16, POS_C = 48;   // positional conv: taps, groups, channels per group
constexpr int POS_KK = POS_K * POS_C;                // its GEMM K
constexpr int GN_PARTS = 1024;                       // frame ranges of the GroupNorm statistics (blocks of conv0_kernel per utterance)
constexpr int CONV_TAPS[6] = {3, 3, 3, 3, 2, 2};
constexpr int HPAD = 40;                             // HuBERT-Soft: (400 - 320) / 2 zeros on each side of the audio (the base form: 0)

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

// ---- GEMM epilogues --------------------------------------------------------------------------------------
struct EpiGelu {   // C[z] = gelu(acc + bias[n]), batch z at C + z * sC
    float* C;
    int64_t ldc;
    const float* bias;
    int64_t sC;
    __device__ __forceinline__ float col(int n) const { return bias ? bias[n] : 0.f; }
    __device__ __forceinline__ void operator()(int z, int m, int n, float v, float cb) const {
        C[(int64_t)z * sC + (int64_t)m * ldc + n] = gelu_erf(v + cb);
    }
    static constexpr bool kStore4 = true;
    __device__ __forceinline__ bool vec_ok() const { return ((uintptr_t)C % 16) == 0 && ldc % 4 == 0 && sC % 4 == 0; }
    __device__ __forceinline__ void store4(int z, int m, int n, f32x4 v) const {
        if (bias) v += *(const gemm::f32x4_u*)(bias + n);
        f32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = gelu_erf(v[i]);
        *(f32x4*)(C + (int64_t)z * sC + (int64_t)m * ldc + n) = r;
    }
};

// positional conv, batch z = utterance * 16 + group: y[b*L + m][g*48 + n] = x[..] + gelu(acc + bias[g*48 + n])
struct EpiPos {
    float* y;
    const float* x;
    const float* bias;
    int L;
    __device__ __forceinline__ float col(int) const { return 0.f; }
    __device__ __forceinline__ void operator()(int z, int m, int n, float v, float) const {
        const int b = z / POS_G, c = (z % POS_G) * POS_C + n;
        const int64_t o = ((int64_t)b * L + m) * HD + c;
        y[o] = x[o] + gelu_erf(v + bias[c]);
    }
};

// ---- ragged batches: per-row counts -----------------------------------------------------------------------
// cnt[b][0] = the row's own samples (held inside 0..T), cnt[b][1..7] = the frames after conv0 and after each strided
// convolution (frames_of on the device; a row too short for the stack, which the caller refuses, counts 0 from there on)
constexpr int HCNT = 8;
__global__ void hub_counts_kernel(const int32_t* __restrict__ n_samples, int64_t B, int64_t T, int pad, int32_t* __restrict__ cnt) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int64_t n = n_samples[b];
    n = n < 0 ? 0 : (n > T ? T : n);
    int32_t* c = cnt + b * HCNT;
    c[0] = (int32_t)n;
    int64_t f = n + 2 * pad < 10 ? 0 : (n + 2 * pad - 10) / 5 + 1;   // (pad 40: at least 15)
    c[1] = (int32_t)f;
    for (int i = 0; i < 6; ++i) {
        const int kt = i < 4 ? 3 : 2;
        f = f < kt ? 0 : (f - kt) / 2 + 1;
        c[i + 2] = (int32_t)f;
    }
}

// ---- conv0 (1 -> 512, kernel 10, stride 5, no bias) + GroupNorm(512, 512) statistics ------------------------
// grid (GN_PARTS, B), block 512 = one channel per thread; the block walks frames [T0*p/P, T0*(p+1)/P) and writes the
// fp64 sum and sum of squares of its channel over them (reduced in a fixed order by gn_finalize_kernel)
// RAGGED (cnt != nullptr): samples past the row's own n_b are SELECTED as 0 (the padding may hold NaN), so the 40 zeros
// a solo call pads with fall out of the same bounds test (`pad` zeros on each side, uniform over the launch: 40, or 0 for
// the base form, where only the row's end is selected); the block walks the row's own t0_b frames partitioned as a solo
// call partitions them (the fp64 sums then add in the same order, empty partitions included).  Frames t0_b..T0-1 of the
// padded buffer, which no frame of the row ever reads, are written by the blocks' second loop so that everything
// downstream of them is finite; they stay out of the statistics.
template <bool RAGGED>
__global__ void __launch_bounds__(512) conv0_kernel(const float* __restrict__ wav, int64_t T, const float* __restrict__ w0,
                                                    float* __restrict__ y, int64_t T0, double* __restrict__ part,
                                                    const int32_t* __restrict__ cnt, int pad) {
    const int b = blockIdx.y, p = blockIdx.x, c = threadIdx.x;
    float w[10];
#pragma unroll
    for (int t = 0; t < 10; ++t) w[t] = w0[c * 10 + t];
    const int64_t n = RAGGED ? (int64_t)cnt[b * HCNT] : T;       // samples of the row
    const int64_t tb = RAGGED ? (int64_t)cnt[b * HCNT + 1] : T0;   // its conv0 frames
    const int64_t f0 = tb * p / GN_PARTS, f1 = tb * (p + 1) / GN_PARTS;
    const float* x = wav + (int64_t)b * T;
    float* yb = y + (int64_t)b * T0 * HC;
    auto frame = [&](int64_t f) {
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 10; ++t) {
            const int64_t i = f * 5 + t - pad;
            const float xv = (i >= 0 && i < n) ? x[i] : 0.f;
            acc = fmaf(w[t], xv, acc);
        }
        yb[f * HC + c] = acc;
        return acc;
    };
    double s = 0.0, ss = 0.0;
    for (int64_t f = f0; f < f1; ++f) {
        const float acc = frame(f);
        s += (double)acc;
        ss += (double)acc * (double)acc;
    }
    double* pp = part + ((int64_t)b * GN_PARTS + p) * 2 * HC;
    pp[c] = s;
    pp[HC + c] = ss;
    if (RAGGED) {
        const int64_t r = T0 - tb;
        for (int64_t f = tb + r * p / GN_PARTS; f < tb + r * (p + 1) / GN_PARTS; ++f) frame(f);
    }
}

// per (utterance, channel): scale = gamma / sqrt(var + eps), shift = beta - mean * scale (biased variance, fp64).  grid (8, B),
// block 1024: 64 channels x 16 slices of the GN_PARTS partial sums, the slices added in a fixed order
// (cnt: the per-row counts of a ragged batch, whose statistics divide by the row's own t0_b; nullptr: T0)
__global__ void __launch_bounds__(1024) gn_finalize_kernel(const double* __restrict__ part, int64_t T0, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ aff,
                                                           const int32_t* __restrict__ cnt) {
    __shared__ double red[2][16][64];
    if (cnt) T0 = cnt[blockIdx.y * HCNT + 1];
    const int b = blockIdx.y, cl = threadIdx.x & 63, sl = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    double s = 0.0, ss = 0.0;
    for (int p = sl; p < GN_PARTS; p += 16) {
        const double* pp = part + ((int64_t)b * GN_PARTS + p) * 2 * HC;
        s += pp[c];
        ss += pp[HC + c];
    }
    red[0][sl][cl] = s;
    red[1][sl][cl] = ss;
    __syncthreads();
    if (sl != 0) return;
    s = 0.0;
    ss = 0.0;
    for (int i = 0; i < 16; ++i) {
        s += red[0][i][cl];
        ss += red[1][i][cl];
    }
    const double mean = s / (double)T0;
    double var = ss / (double)T0 - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double sc = (double)gamma[c] / sqrt(var + 1e-5);
    aff[(b * HC + c) * 2] = (float)sc;
    aff[(b * HC + c) * 2 + 1] = (float)((double)beta[c] - mean * sc);
}

// y = gelu(y * scale[c] + shift[c]) in place over (B, T0, 512)
__global__ void __launch_bounds__(256) gn_apply_kernel(float* __restrict__ y, int64_t T0, int64_t n4, const float* __restrict__ aff) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t e = i * 4;
        const int64_t b = e / (T0 * HC);
        const int c = (int)(e % HC);
        f32x4 v = *(f32x4*)(y + e);
        const float* a = aff + (b * HC + c) * 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = gelu_erf(fmaf(v[j], a[2 * j], a[2 * j + 1]));
        *(f32x4*)(y + e) = v;
    }
}

// ---- LayerNorm over C columns (eps 1e-5) of x (+ r): one wave per row, in place allowed --------------------
template <int C>
__global__ void __launch_bounds__(256) layernorm_kernel(const float* x, const float* __restrict__ r, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* y, int64_t rows) {
    constexpr int NV = C / 256;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int64_t o = row * C + (i * 64 + lane) * 4;
        v[i] = *(const f32x4*)(x + o);
        if (r) v[i] += *(const f32x4*)(r + o);
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(s) * (1.f / C);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        v[i] -= mean;
        q += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) * (1.f / C) + 1e-5f);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (i * 64 + lane) * 4;
        const f32x4 g = *(const f32x4*)(gamma + c), bb = *(const f32x4*)(beta + c);
        *(f32x4*)(y + row * C + c) = v[i] * rstd * g + bb;
    }
}

// ---- positional conv operand: x (B*L, 768) -> xg[b][g][L + 128][48], 64 zero rows before and after ---------------
// (cnt: ragged batch, frames >= L_b are selected as 0 too: the zero edge a row encoded alone sees)
__global__ void __launch_bounds__(256) pos_pack_kernel(const float* __restrict__ x, int L, int64_t n4, float* __restrict__ xg,
                                                       const int32_t* __restrict__ cnt) {
    const int64_t rows = L + POS_K;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t e = i * 4;
        const int c = (int)(e % POS_C);
        const int64_t r = (e / POS_C) % rows, bg = e / (POS_C * rows);
        const int64_t b = bg / POS_G, g = bg % POS_G;
        const int64_t src = r - POS_K / 2;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int64_t Lb = cnt ? (int64_t)cnt[b * HCNT + 7] : (int64_t)L;
        if (src >= 0 && src < Lb) v = *(const f32x4*)(x + (b * L + src) * HD + g * POS_C + c);
        *(f32x4*)(xg + e) = v;
    }
}

// ---- weight preparation ------------------------------------------------------------------------------------
// (Cout, Cin, taps) -> (Cout, tap * Cin + ci)
__global__ void __launch_bounds__(256) conv_repack_kernel(const float* __restrict__ w, int taps, int64_t n, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t co = i / (HC * taps);
        const int rem = (int)(i % (HC * taps));
        const int t = rem / HC, ci = rem % HC;
        out[i] = w[(co * HC + ci) * taps + t];
    }
}

// weight_norm(dim=2): scale[k] = g[k] / ||v[:, :, k]||  (fp64 sum of squares), one block per tap
__global__ void __launch_bounds__(256) pos_norm_kernel(const float* __restrict__ v, const float* __restrict__ g, float* __restrict__ scale) {
    __shared__ double red[4];
    const int k = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < HD * POS_C; i += 256) {
        const double a = v[(int64_t)i * POS_K + k];
        s += a * a;
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) scale[k] = (float)((double)g[k] / sqrt((red[0] + red[1]) + (red[2] + red[3])));
}

// w[g][n][tap * 48 + ci] = v[g*48 + n][ci][tap] * scale[tap]
__global__ void __launch_bounds__(256) pos_weight_kernel(const float* __restrict__ v, const float* __restrict__ scale, float* __restrict__ out) {
    const int64_t n = (int64_t)HD * POS_KK;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t co = i / POS_KK;                 // = g * 48 + n
        const int kk = (int)(i % POS_KK), t = kk / POS_C, ci = kk % POS_C;
        out[i] = v[(co * POS_C + ci) * POS_K + t] * scale[t];
    }
}

// fairseq keeps the attention's input projections apart: q_proj, k_proj, v_proj (768, 768) with a bias each.  The QKV GEMM reads
// one (2304, 768) operand and one (2304) bias per layer: rows q, then k, then v, as nn.MultiheadAttention's in_proj.
// p[layer] = {q_w, k_w, v_w, q_b, k_b, v_b}.  grid (blocks, 12), a copy.
struct HubQkv {
    const float* p[12][6];
};
__global__ void __launch_bounds__(256) qkv_pack_kernel(HubQkv s, float* __restrict__ wout, float* __restrict__ bout) {
    const int ly = blockIdx.y;
    constexpr int NW = HD * HD;
    float* w = wout + (int64_t)ly * 3 * NW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 3 * NW; i += gridDim.x * 256) {
        const int part = i / NW;
        w[i] = s.p[ly][part][i - part * NW];
    }
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < 3 * HD; i += 256) bout[ly * 3 * HD + i] = s.p[ly][3 + i / HD][i % HD];
}

// ---- softmax attention (flash form: online softmax, no L x L matrix) ---------------------------------------------
// q, k, v: rows (b * L + i) at stride ld, head h at column h * 64; out likewise at stride ldo.  One workgroup per (QT queries,
// utterance, head); thread t owns query t % QT and the keys j = s, s + S, ... (s = t / QT, S = 256 / QT) of every 64-key tile
// staged in LDS; the S partial (max, sum, accumulator) triples of a query are merged through LDS at the end.  fp32 products.
constexpr int ATT_KT = 64, ATT_LD = HDH + 4;   // keys per LDS tile; padded row (4 rows read at once by a wave when QT = 16)

// RAGGED: keys[b * kstride] is the key count L_b of utterance b (held inside 0..L); rows are still L apart.  Tile loop, nk
// and staging test against L_b, so the online softmax of a row walks the tiles it walks alone; a query tile wholly past L_b
// returns before it stages anything and query rows >= L_b are not written.
template <int QT, bool RAGGED>
__global__ void __launch_bounds__(256) attention_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                        const float* __restrict__ v, int64_t ld, float* __restrict__ out,
                                                        int64_t ldo, int Lpad, int heads, float scale,
                                                        const int32_t* __restrict__ keys, int kstride) {
    constexpr int S = 256 / QT, KPT = ATT_KT / S;    // key splits, keys per thread and tile
    constexpr int MERGE = S * QT * HDH;              // floats of the merge buffer
    __shared__ __attribute__((aligned(16))) float smem[MERGE + 2 * 256];
    float* const ks = smem;
    float* const vs = smem + ATT_KT * ATT_LD;
    const int tid = threadIdx.x, qi = tid % QT, s = tid / QT;
    const int b = blockIdx.y / heads, h = blockIdx.y % heads;
    int L = Lpad;
    if (RAGGED) {
        L = keys[(int64_t)b * kstride];
        L = L < 0 ? 0 : (L > Lpad ? Lpad : L);
        if ((int)blockIdx.x * QT >= L) return;   // (uniform over the workgroup)
    }
    const int qrow = blockIdx.x * QT + qi;
    const int64_t base = (int64_t)b * Lpad;
    float qr[HDH], acc[HDH];
    {
        const float* qp = q + (base + (qrow < L ? qrow : L - 1)) * ld + h * HDH;
#pragma unroll
        for (int d = 0; d < HDH; d += 4) {
            const f32x4 t = *(const f32x4*)(qp + d);
            qr[d] = t[0] * scale; qr[d + 1] = t[1] * scale; qr[d + 2] = t[2] * scale; qr[d + 3] = t[3] * scale;
        }
    }
#pragma unroll
    for (int d = 0; d < HDH; ++d) acc[d] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int kt0 = 0; kt0 < L; kt0 += ATT_KT) {
        __syncthreads();   // the previous tile's readers are done
#pragma unroll
        for (int i = 0; i < ATT_KT * HDH / 4 / 256; ++i) {
            const int idx = tid + i * 256, row = idx >> 4, c4 = (idx & 15) * 4;
            const int key = kt0 + row;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (key < L) {
                kv = *(const f32x4*)(k + (base + key) * ld + h * HDH + c4);
                vv = *(const f32x4*)(v + (base + key) * ld + h * HDH + c4);
            }
            *(f32x4*)(ks + row * ATT_LD + c4) = kv;
            *(f32x4*)(vs + row * ATT_LD + c4) = vv;
        }
        __syncthreads();
        const int nk = L - kt0 < ATT_KT ? L - kt0 : ATT_KT;
        float sc[KPT];
        float tmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < KPT; ++u) {
            const int j = s + u * S;
            float a = -INFINITY;
            if (j < nk) {
                a = 0.f;
                const float* kr = ks + j * ATT_LD;
#pragma unroll
                for (int d = 0; d < HDH; d += 4) {
                    const f32x4 t = *(const f32x4*)(kr + d);
                    a = fmaf(qr[d], t[0], a);
                    a = fmaf(qr[d + 1], t[1], a);
                    a = fmaf(qr[d + 2], t[2], a);
                    a = fmaf(qr[d + 3], t[3], a);
                }
            }
            sc[u] = a;
            tmax = fmaxf(tmax, a);
        }
        if (tmax == -INFINITY) continue;   // no key of this tile for this thread (uniform across the barrier-free rest)
        const float mn = fmaxf(m, tmax);
        const float corr = expf(m - mn);   // m = -inf on the first tile: 0
        l *= corr;
#pragma unroll
        for (int d = 0; d < HDH; ++d) acc[d] *= corr;
#pragma unroll
        for (int u = 0; u < KPT; ++u) {
            const int j = s + u * S;
            if (j < nk) {
                const float p = expf(sc[u] - mn);
                l += p;
                const float* vr = vs + j * ATT_LD;
#pragma unroll
                for (int d = 0; d < HDH; d += 4) {
                    const f32x4 t = *(const f32x4*)(vr + d);
                    acc[d] = fmaf(p, t[0], acc[d]);
                    acc[d + 1] = fmaf(p, t[1], acc[d + 1]);
                    acc[d + 2] = fmaf(p, t[2], acc[d + 2]);
                    acc[d + 3] = fmaf(p, t[3], acc[d + 3]);
                }
            }
        }
        m = mn;
    }
    // merge the S partial results of every query (layout [s][d][qi]: consecutive threads, consecutive words)
    __syncthreads();
    float* const red = smem;
    float* const mred = smem + MERGE;
    float* const lred = mred + 256;
#pragma unroll
    for (int d = 0; d < HDH; ++d) red[(s * HDH + d) * QT + qi] = acc[d];
    mred[s * QT + qi] = m;
    lred[s * QT + qi] = l;
    __syncthreads();
    constexpr int DPT = HDH / S;   // output dims per thread
    const int q2 = tid % QT, dg = tid / QT;
    const int orow = blockIdx.x * QT + q2;
    if (orow >= L) return;
    float M = -INFINITY;
#pragma unroll
    for (int t = 0; t < S; ++t) M = fmaxf(M, mred[t * QT + q2]);
    float wsum = 0.f, wt[S];
#pragma unroll
    for (int t = 0; t < S; ++t) {
        wt[t] = expf(mred[t * QT + q2] - M);   // a split without keys: exp(-inf) = 0
        wsum = fmaf(lred[t * QT + q2], wt[t], wsum);
    }
    const float inv = 1.f / wsum;
    float* op = out + (base + orow) * ldo + h * HDH + dg * DPT;
#pragma unroll
    for (int e = 0; e < DPT; ++e) {
        const int d = dg * DPT + e;
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < S; ++t) a = fmaf(red[(t * HDH + d) * QT + q2], wt[t], a);
        op[e] = a * inv;
    }
}

template <bool RAGGED>
int attention_launch(hipStream_t st, const float* q, const float* k, const float* v, int64_t ld, float* out, int64_t ldo,
                     int64_t B, int L, int heads, const int32_t* keys = nullptr, int kstride = 0) {
    // the largest query tile whose grid still covers the 256 CUs (small L: more, shorter workgroups); a ragged batch chooses
    // by its padded L
    const int64_t bh = B * heads;
    const float scale = 0.125f;   // 1 / sqrt(64)
    if (bh * ceil_div64(L, 64) >= 256) {
        hipLaunchKernelGGL((attention_kernel<64, RAGGED>), dim3((unsigned)ceil_div64(L, 64), (unsigned)bh), dim3(256), 0, st, q, k, v, ld, out, ldo, L, heads, scale, keys, kstride);
    } else if (bh * ceil_div64(L, 32) >= 256) {
        hipLaunchKernelGGL((attention_kernel<32, RAGGED>), dim3((unsigned)ceil_div64(L, 32), (unsigned)bh), dim3(256), 0, st, q, k, v, ld, out, ldo, L, heads, scale, keys, kstride);
    } else {
        hipLaunchKernelGGL((attention_kernel<16, RAGGED>), dim3((unsigned)ceil_div64(L, 16), (unsigned)bh), dim3(256), 0, st, q, k, v, ld, out, ldo, L, heads, scale, keys, kstride);
    }
    return 0;
}

// ---- last step of a ragged batch: dst[b][i][:] = i < L_b ? src[b][i][:] : 0 over (B, L, C); src == dst is allowed -----
// A selection, never a product: the rows >= L_b of src may hold NaN (hubert_run, RAGGED INVARIANT).  16-byte aligned dst.
__global__ void __launch_bounds__(256) hub_crop_kernel(const float* src, float* dst, int64_t L, int C4, int64_t n4,
                                                       const int32_t* __restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C4, b = row / L, fr = row - b * L;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (fr < (int64_t)cnt[b * HCNT + 7]) v = *(const f32x4*)(src + i * 4);
        *(f32x4*)(dst + i * 4) = v;
    }
}

// ---- GEMM helper --------------------------------------------------------------------------------------------
template <class Epi>
void hub_gemm(hipStream_t st, int math, const float* A, int64_t lda, int64_t sA, const float* W, int64_t ldw, int64_t sW_lo,
              int M, int N, int K, int batch, int zdiv, const Epi& e) {
    gemm::Args g = gemm::make(A, lda, W, ldw, M, N, K);
    g.zdiv = zdiv;
    if (zdiv > 1) {   // z = (outer, inner): A moves by sA per outer, by (L + 128) * 48 per inner; W by sW_lo per inner
        g.sA_hi = sA * zdiv;
        g.sA_lo = sA;
        g.sB_lo = sW_lo;
    } else {
        g.sA_hi = sA;
    }
    g.math = math == DDSP_MATH_FP32 ? 0 : 3;
    gemm::launch<true, true, gemm::A_PLAIN>(st, g, batch, e);
}

int64_t frames_of(int64_t T, int64_t (&t)[7], int pad) {
    if (T < 0) return -1;
    int64_t n = T + 2 * pad;
    if (n < 10) return 0;
    n = (n - 10) / 5 + 1;
    t[0] = n;
    for (int i = 0; i < 6; ++i) {
        const int kt = CONV_TAPS[i];
        if (n < kt) return 0;
        n = (n - kt) / 2 + 1;
        t[i + 1] = n;
    }
    return n;
}

struct HubPlan {
    size_t off[16];
    size_t total;
};
enum { S_Y0, S_Y1, S_PART, S_AFF, S_Z, S_X, S_Y, S_QKV, S_CTX, S_H, S_XG, S_WCONV, S_WPOS, S_PSCALE, S_CNT, S_WQKV, S_BQKV, S_N };

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// bytes of the prepared weights: the six repacked conv matrices, the folded positional weights, the tap scales and, for the
// base form, the packed QKV operands and biases of the 12 layers behind them
size_t wconv_floats() { return (size_t)HC * HC * (3 * 4 + 2 * 2); }
size_t wpos_floats() { return (size_t)HD * POS_KK; }
size_t wqkv_floats() { return (size_t)12 * 3 * HD * HD; }
size_t bqkv_floats() { return (size_t)12 * 3 * HD; }
size_t prep_bytes(bool base) {
    return align256(wconv_floats() * 4) + align256(wpos_floats() * 4) + align256(POS_K * 4) +
           (base ? align256(wqkv_floats() * 4) + align256(bqkv_floats() * 4) : 0);
}

HubPlan plan(int64_t B, const int64_t (&t)[7], bool base) {
    const int64_t L = t[6];
    size_t sz[S_N];
    sz[S_Y0] = (size_t)B * t[0] * HC * 4;
    sz[S_Y1] = (size_t)B * t[1] * HC * 4;
    sz[S_PART] = (size_t)B * GN_PARTS * 2 * HC * 8;
    sz[S_AFF] = (size_t)B * HC * 2 * 4;
    sz[S_Z] = (size_t)B * L * HC * 4;
    sz[S_X] = (size_t)B * L * HD * 4;
    sz[S_Y] = (size_t)B * L * HD * 4;
    sz[S_QKV] = (size_t)B * L * 3 * HD * 4;
    sz[S_CTX] = (size_t)B * L * HD * 4;
    sz[S_H] = (size_t)B * L * HFF * 4;
    sz[S_XG] = (size_t)B * POS_G * (L + POS_K) * POS_C * 4;
    sz[S_WCONV] = wconv_floats() * 4;
    sz[S_WPOS] = wpos_floats() * 4;
    sz[S_PSCALE] = POS_K * 4;
    sz[S_CNT] = (size_t)B * HCNT * 4;
    sz[S_WQKV] = base ? wqkv_floats() * 4 : 0;
    sz[S_BQKV] = base ? bqkv_floats() * 4 : 0;
    HubPlan p;
    size_t o = 0;
    for (int i = 0; i < S_N; ++i) {
        p.off[i] = o;
        o += align256(sz[i]);
    }
    p.total = o;
    return p;
}

int prepare_weights(ddsp_ctx* ctx, hipStream_t st, const ddsp_hubert_weights& w, float* wconv, float* wpos, float* pscale,
                    const HubQkv* qkv, float* wqkv, float* bqkv) {
    size_t o = 0;
    for (int i = 0; i < 6; ++i) {
        const int64_t n = (int64_t)HC * HC * CONV_TAPS[i];
        hipLaunchKernelGGL(conv_repack_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(n, 256), 4096)), dim3(256), 0, st,
                           w.conv_w[i], CONV_TAPS[i], n, wconv + o);
        o += n;
    }
    hipLaunchKernelGGL(pos_norm_kernel, dim3(POS_K), dim3(256), 0, st, w.pos_v, w.pos_g, pscale);
    hipLaunchKernelGGL(pos_weight_kernel, dim3(4096), dim3(256), 0, st, w.pos_v, pscale, wpos);
    if (qkv) hipLaunchKernelGGL(qkv_pack_kernel, dim3(512, 12), dim3(256), 0, st, *qkv, wqkv, bqkv);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// every pointer in front of `version` is set (both weight structs are pointers up to there)
template <class W>
bool weights_complete(const W& w) {
    const float* const* p = (const float* const*)&w;
    const size_t n = offsetof(W, version) / sizeof(const float*);
    for (size_t i = 0; i < n; ++i)
        if (!p[i]) return false;
    return true;
}

// What differs between the two forms of the network.  `key`: the caller's struct, whose bytes in front of its version name
// the prepared weights in the context's slot.  `qkv`: nullptr (HuBERT-Soft: `w` holds in_proj) or the base form's separate
// projections, which prepare_weights packs; hubert_run then points in_proj of its copy of `w` at the packed operands.
struct HubForm {
    int pad;
    const void* key;
    size_t key_bytes;
    const HubQkv* qkv;
};

// nl transformer layers (0..12), then `tail`.  n_samples: nullptr, or the DEVICE array of a ragged batch's B sample counts
// (never read back: the per-row frame counts are derived on the device); the launches are the rectangular call's plus the
// counts kernel and the final crop, over the padded shapes.
enum { TAIL_CONV, TAIL_HIDDEN, TAIL_UNITS };   // conv stack output (B, Fr, 512) | hidden state (B, Fr, 768) | its projection (B, Fr, 256)
int hubert_run(ddsp_ctx* ctx, hipStream_t st, const ddsp_hubert_weights& w0, const HubForm& form, const float* wav, int64_t B,
               int64_t T, int nl, int tail, float* out, const int32_t* n_samples) {
    // ("ddsp_hubert" / "ddsp_hubert_ragged" / "ddsp_hubert_base": the family of entry points that was called)
    const bool is_base = form.qkv != nullptr;
#define HUB_MSG(text) (is_base ? "ddsp_hubert_base: " text : n_samples ? "ddsp_hubert_ragged: " text : "ddsp_hubert: " text)
    DDSP_REQUIRE(ctx, wav && out, HUB_MSG("null argument"));
    DDSP_REQUIRE(ctx, B >= 1 && T >= 0 && nl >= 0 && nl <= 12, HUB_MSG("bad shape or layer"));
    // the final crop of a ragged batch moves 16 bytes at a time
    DDSP_REQUIRE(ctx, !n_samples || ((uintptr_t)out % 16) == 0, HUB_MSG("the output of a ragged batch must be 16-byte aligned"));
    int64_t t[7];
    const int64_t Fr = frames_of(T, t, form.pad);
    DDSP_REQUIRE(ctx, Fr >= 1, HUB_MSG("audio too short for the conv stack (its frame rule gives 0)"));
    DDSP_REQUIRE(ctx, B * t[0] < ((int64_t)1 << 31) && B * Fr * HFF < ((int64_t)1 << 31), HUB_MSG("input too long"));
#undef HUB_MSG
    ddsp_hubert_weights w = w0;
    DDSP_ENTER_DEVICE(ctx);
    const int L = (int)Fr;
    const int64_t rows = B * Fr;
    const int math = ctx->math;
    const int pad = form.pad;

    // prepared weights: the context's slot (state bit 0: prepared), else scratch
    const float *wconv = nullptr, *wpos = nullptr;
    float *wqkv = nullptr, *bqkv = nullptr;
    ddsp_weight_slot* slot;
    int rc = ddsp_weight_slot_take(ctx, st, ctx->hubert_slot, form.key, form.key_bytes, w.version, prep_bytes(is_base), &slot, true);
    if (rc) return rc;
    const bool cached = slot != nullptr;
    if (cached) {
        char* base = slot->dev;
        wconv = (const float*)base;
        wpos = (const float*)(base + align256(wconv_floats() * 4));
        float* pscale = (float*)(base + align256(wconv_floats() * 4) + align256(wpos_floats() * 4));
        if (is_base) {
            wqkv = pscale + align256(POS_K * 4) / 4;
            bqkv = wqkv + align256(wqkv_floats() * 4) / 4;
        }
        if (!(slot->state & 1)) {
            if ((rc = prepare_weights(ctx, st, w, (float*)wconv, (float*)wpos, pscale, form.qkv, wqkv, bqkv))) return rc;
            slot->state = 1;
        }
    }
    // (the arena always has room for the prepared weights: a capture after cached warm-up calls must not have to grow it)
    const HubPlan p = plan(B, t, is_base);
    rc = ddsp_scratch_reserve_bytes(ctx, p.total + 4096);
    if (rc) return rc;
    ddsp_scratch_reset(ctx);
    void* arena = nullptr;
    if ((rc = ddsp_scratch_get(ctx, p.total, &arena))) return rc;
    char* a = (char*)arena;
    auto buf = [&](int i) { return (float*)(a + p.off[i]); };
    if (!cached) {
        wconv = buf(S_WCONV);
        wpos = buf(S_WPOS);
        wqkv = buf(S_WQKV);
        bqkv = buf(S_BQKV);
        if ((rc = prepare_weights(ctx, st, w, buf(S_WCONV), buf(S_WPOS), buf(S_PSCALE), form.qkv, wqkv, bqkv))) return rc;
    }
    if (is_base)
        for (int li = 0; li < 12; ++li) {
            w.layer[li].in_proj_w = wqkv + (size_t)li * 3 * HD * HD;
            w.layer[li].in_proj_b = bqkv + (size_t)li * 3 * HD;
        }

    // ---- feature extractor ----
    float* y0 = buf(S_Y0);
    float* y1 = buf(S_Y1);
    const bool ragged = n_samples != nullptr;
    int32_t* cnt = ragged ? (int32_t*)buf(S_CNT) : nullptr;
    if (ragged) {
        hipLaunchKernelGGL(hub_counts_kernel, dim3((unsigned)ceil_div64(B, 256)), dim3(256), 0, st, n_samples, B, T, pad, cnt);
        hipLaunchKernelGGL(conv0_kernel<true>, dim3(GN_PARTS, (unsigned)B), dim3(512), 0, st, wav, T, w.conv0_w, y0, t[0],
                           (double*)buf(S_PART), (const int32_t*)cnt, pad);
    } else {
        hipLaunchKernelGGL(conv0_kernel<false>, dim3(GN_PARTS, (unsigned)B), dim3(512), 0, st, wav, T, w.conv0_w, y0, t[0],
                           (double*)buf(S_PART), (const int32_t*)nullptr, pad);
    }
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(HC / 64, (unsigned)B), dim3(1024), 0, st, (const double*)buf(S_PART), t[0], w.norm0_w, w.norm0_b,
                       buf(S_AFF), (const int32_t*)cnt);
    {
        const int64_t n4 = B * t[0] * HC / 4;
        hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(n4, 256), 8192)), dim3(256), 0, st, y0, t[0], n4,
                           (const float*)buf(S_AFF));
    }
    float* cur = y0;
    float* nxt = y1;
    size_t wo = 0;
    // A ragged batch needs nothing here: frame j < t_{i+1}(b) of a row reads frames 2j .. 2j + taps - 1 <= t_i(b) - 1, its
    // own.  The frames past a row's count are computed too, from conv0's selected zeros and the row's own GroupNorm
    // affine: up to the transformer they are finite, and nothing of the row reads them.
    for (int i = 0; i < 6; ++i) {
        const int kt = CONV_TAPS[i];
        EpiGelu e{nxt, HC, nullptr, t[i + 1] * HC};
        hub_gemm(st, math, cur, 2 * HC, t[i] * HC, wconv + wo, (int64_t)kt * HC, 0, (int)t[i + 1], HC, kt * HC, (int)B, 1, e);
        wo += (size_t)HC * HC * kt;
        float* s = cur;
        cur = nxt;
        nxt = s;
    }
    // ragged: rows >= L_b of whatever is returned are written as exact zeros, by selection
    auto crop = [&](const float* src, int C) {
        const int64_t n4 = rows * C / 4;
        hipLaunchKernelGGL(hub_crop_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(n4, 256), 8192)), dim3(256), 0, st, src, out,
                           Fr, C / 4, n4, (const int32_t*)cnt);
    };
    if (tail == TAIL_CONV) {
        if (ragged)
            crop(cur, HC);
        else
            DDSP_HIP(ctx, hipMemcpyAsync(out, cur, (size_t)rows * HC * 4, hipMemcpyDeviceToDevice, st));
        DDSP_LAUNCH_CHECK(ctx);
        return DDSP_OK;
    }
    // ---- feature projection, positional embedding, norm ----
    const unsigned ln_grid = (unsigned)ceil_div64(rows, 4);
    float* z = buf(S_Z);
    float* X = buf(S_X);
    float* Y = buf(S_Y);
    hipLaunchKernelGGL(layernorm_kernel<HC>, dim3(ln_grid), dim3(256), 0, st, cur, nullptr, w.fp_norm_w, w.fp_norm_b, z, rows);
    hub_gemm(st, math, z, HC, 0, w.fp_proj_w, HC, 0, (int)rows, HD, HC, 1, 1, gemm::EpiStore{X, HD, w.fp_proj_b, 1, 0, 0});
    {
        const int64_t n4 = B * POS_G * (L + POS_K) * POS_C / 4;
        hipLaunchKernelGGL(pos_pack_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(n4, 256), 8192)), dim3(256), 0, st, X, L, n4,
                           buf(S_XG), (const int32_t*)cnt);
        hub_gemm(st, math, buf(S_XG), POS_C, (int64_t)(L + POS_K) * POS_C, wpos, POS_KK, (int64_t)POS_C * POS_KK, L, POS_C, POS_KK,
                 (int)(B * POS_G), POS_G, EpiPos{Y, X, w.pos_b, L});
    }
    hipLaunchKernelGGL(layernorm_kernel<HD>, dim3(ln_grid), dim3(256), 0, st, Y, nullptr, w.norm_w, w.norm_b, X, rows);
    // ---- transformer (post-norm) ----
    float* qkv = buf(S_QKV);
    float* cx = buf(S_CTX);
    float* hh = buf(S_H);
    for (int li = 0; li < nl; ++li) {
        const ddsp_hubert_layer& ly = w.layer[li];
        hub_gemm(st, math, X, HD, 0, ly.in_proj_w, HD, 0, (int)rows, 3 * HD, HD, 1, 1, gemm::EpiStore{qkv, 3 * HD, ly.in_proj_b, 1, 0, 0});
        // RAGGED INVARIANT: the query rows >= L_b of cx keep what the arena held - possibly NaN or inf - and from here on so
        // may those rows of Y, X and hh.  That is sound only because (1) every step below is row-wise (GEMM rows, LayerNorm),
        // (2) the key loop stops at L_b, and (3) the returned rows >= L_b are written by SELECTION in hub_crop_kernel.  A crop
        // that multiplies by a mask, or any new step that mixes rows, must first zero those rows of cx.
        if (ragged)
            attention_launch<true>(st, qkv, qkv + HD, qkv + 2 * HD, 3 * HD, cx, HD, B, L, HHEADS, cnt + 7, HCNT);
        else
            attention_launch<false>(st, qkv, qkv + HD, qkv + 2 * HD, 3 * HD, cx, HD, B, L, HHEADS);
        hub_gemm(st, math, cx, HD, 0, ly.out_proj_w, HD, 0, (int)rows, HD, HD, 1, 1, gemm::EpiResidual{Y, X, HD, ly.out_proj_b});
        hipLaunchKernelGGL(layernorm_kernel<HD>, dim3(ln_grid), dim3(256), 0, st, Y, nullptr, ly.norm1_w, ly.norm1_b, X, rows);
        hub_gemm(st, math, X, HD, 0, ly.linear1_w, HD, 0, (int)rows, HFF, HD, 1, 1, EpiGelu{hh, HFF, ly.linear1_b, 0});
        hub_gemm(st, math, hh, HFF, 0, ly.linear2_w, HFF, 0, (int)rows, HD, HFF, 1, 1, gemm::EpiResidual{Y, X, HD, ly.linear2_b});
        hipLaunchKernelGGL(layernorm_kernel<HD>, dim3(ln_grid), dim3(256), 0, st, Y, nullptr, ly.norm2_w, ly.norm2_b, X, rows);
    }
    if (tail == TAIL_HIDDEN) {
        if (ragged)
            crop(X, HD);
        else
            DDSP_HIP(ctx, hipMemcpyAsync(out, X, (size_t)rows * HD * 4, hipMemcpyDeviceToDevice, st));
    } else {
        hub_gemm(st, math, X, HD, 0, w.proj_w, HD, 0, (int)rows, HU, HD, 1, 1, gemm::EpiStore{out, HU, w.proj_b, 1, 0, 0});
        if (ragged) crop(out, HU);
    }
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

}  // namespace

extern "C" int64_t ddsp_hubert_frames(int64_t T) {
    int64_t t[7];
    return frames_of(T, t, HPAD);
}

extern "C" int64_t ddsp_hubert_base_frames(int64_t T) {
    int64_t t[7];
    return frames_of(T, t, 0);
}

namespace {
int hubert_soft_run(ddsp_ctx* ctx, hipStream_t st, const ddsp_hubert_weights* w, const float* wav, int64_t B, int64_t T, int nl,
                    int tail, float* out, const int32_t* n_samples) {
    DDSP_REQUIRE(ctx, ctx && w, n_samples ? "ddsp_hubert_ragged: null argument" : "ddsp_hubert: null argument");
    DDSP_REQUIRE(ctx, weights_complete(*w), n_samples ? "ddsp_hubert_ragged: a weight pointer is null" : "ddsp_hubert: a weight pointer is null");
    const HubForm form{HPAD, w, offsetof(ddsp_hubert_weights, version), nullptr};
    return hubert_run(ctx, st, *w, form, wav, B, T, nl, tail, out, n_samples);
}
}  // namespace

// n_samples == nullptr is the rectangular batch
extern "C" int ddsp_hubert_soft_units(ddsp_ctx* ctx, void* stream, const ddsp_hubert_weights* w, const float* wav, int64_t B,
                                      int64_t T, const int32_t* n_samples, float* units) {
    return hubert_soft_run(ctx, (hipStream_t)stream, w, wav, B, T, 12, TAIL_UNITS, units, n_samples);
}

extern "C" int ddsp_hubert_encode(ddsp_ctx* ctx, void* stream, const ddsp_hubert_weights* w, const float* wav, int64_t B, int64_t T,
                                  const int32_t* n_samples, int layer, float* out) {
    DDSP_REQUIRE(ctx, layer >= -1 && layer <= 12, "ddsp_hubert_encode: layer must be -1 (conv stack) or 0..12");
    return hubert_soft_run(ctx, (hipStream_t)stream, w, wav, B, T, layer < 0 ? 0 : layer, layer < 0 ? TAIL_CONV : TAIL_HIDDEN, out,
                           n_samples);
}

// the base form: the struct's fields that both forms share go into a ddsp_hubert_weights whose in_proj hubert_run fills in
extern "C" int ddsp_hubert_base_units(ddsp_ctx* ctx, void* stream, const ddsp_hubert_base_weights* bw, const float* wav, int64_t B,
                                      int64_t T, const int32_t* n_samples, int n_layers, int project, float* out) {
    DDSP_REQUIRE(ctx, ctx && bw, "ddsp_hubert_base: null argument");
    DDSP_REQUIRE(ctx, weights_complete(*bw), "ddsp_hubert_base: a weight pointer is null");
    DDSP_REQUIRE(ctx, n_layers >= 1 && n_layers <= 12 && (project == 0 || project == 1),
                 "ddsp_hubert_base: n_layers must be 1..12 and project 0 or 1");
    ddsp_hubert_weights w{};
    w.conv0_w = bw->conv0_w; w.norm0_w = bw->norm0_w; w.norm0_b = bw->norm0_b;
    for (int i = 0; i < 6; ++i) w.conv_w[i] = bw->conv_w[i];
    w.fp_norm_w = bw->fp_norm_w; w.fp_norm_b = bw->fp_norm_b; w.fp_proj_w = bw->fp_proj_w; w.fp_proj_b = bw->fp_proj_b;
    w.pos_b = bw->pos_b; w.pos_g = bw->pos_g; w.pos_v = bw->pos_v;
    w.norm_w = bw->norm_w; w.norm_b = bw->norm_b;
    HubQkv qkv;
    for (int i = 0; i < 12; ++i) {
        const ddsp_hubert_base_layer& s = bw->layer[i];
        ddsp_hubert_layer& d = w.layer[i];
        const float* six[6] = {s.q_w, s.k_w, s.v_w, s.q_b, s.k_b, s.v_b};
        for (int j = 0; j < 6; ++j) qkv.p[i][j] = six[j];
        d.out_proj_w = s.out_w; d.out_proj_b = s.out_b;
        d.norm1_w = s.ln1_w; d.norm1_b = s.ln1_b;
        d.linear1_w = s.fc1_w; d.linear1_b = s.fc1_b; d.linear2_w = s.fc2_w; d.linear2_b = s.fc2_b;
        d.norm2_w = s.ln2_w; d.norm2_b = s.ln2_b;
    }
    w.proj_w = bw->proj_w; w.proj_b = bw->proj_b;
    w.version = bw->version;
    const HubForm form{0, bw, offsetof(ddsp_hubert_base_weights, version), &qkv};
    return hubert_run(ctx, (hipStream_t)stream, w, form, wav, B, T, n_layers, project ? TAIL_UNITS : TAIL_HIDDEN, out, n_samples);
}

// n_keys == nullptr attends over all L rows
extern "C" int ddsp_softmax_attention(ddsp_ctx* ctx, void* stream, const float* q, const float* k, const float* v, int64_t B,
                                      int64_t L, int heads, float* out, int math, const int32_t* n_keys) {
    DDSP_REQUIRE(ctx, ctx && q && k && v && out, "ddsp_softmax_attention: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && L >= 0 && L < (1 << 30) && heads >= 1 && heads <= 4096, "ddsp_softmax_attention: bad shape");
    DDSP_REQUIRE(ctx, math == DDSP_MATH_FP32 || math == DDSP_MATH_SPLIT_BF16, "ddsp_softmax_attention: unknown math");
    DDSP_REQUIRE(ctx, (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16) == 0, "ddsp_softmax_attention: 16-byte aligned operands");
    if (B == 0 || L == 0) return DDSP_OK;
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    if (n_keys)
        attention_launch<true>(st, q, k, v, (int64_t)heads * HDH, out, (int64_t)heads * HDH, B, (int)L, heads, n_keys, 1);
    else
        attention_launch<false>(st, q, k, v, (int64_t)heads * HDH, out, (int64_t)heads * HDH, B, (int)L, heads);
    ddsp_prof_end(ctx, st, 4.0 * B * heads * (double)L * L * HDH, 16.0 * B * L * heads * HDH);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
