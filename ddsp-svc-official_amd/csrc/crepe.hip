// CREPE pitch tracker (the 'crepe' branch of the reference's F0_Extractor, ddsp/vocoder.py:39-113: torchcrepe.predict with
// pad=True, hop 80, the Viterbi decoder, then the reference's median / threshold / masked-average post-filter) on gfx950.
//
// Network (torchcrepe's 'full' or 'tiny'; frame-major fp32 activations, one row per (CREPE frame, position)):
//   * framing: each 1024-sample frame normalised (fp64 mean and unbiased std) and written with the conv1 padding (254 zeros
//     on each side: 1532 floats per frame);
//   * conv1 (1 -> W0, 512 taps, stride 4): a GEMM over OVERLAPPING rows, batched over the frames: A(m, k) = frame[4m + k],
//     lda = 4 < K = 512, frames 1532 floats apart (gemm_f32.h, A_FRAMES note); the weights are already (Cout, K);
//   * conv2..conv6 (64 taps, padding (31, 32)): the A_CONVK implicit-im2col loader with Fr = positions per CREPE frame - its
//     centring (ktaps - 1) / 2 = 31 is exactly the (31, 32) padding, and m % Fr keeps every frame's zeros inside the frame;
//     weights repacked once to (Cout, tap * Cin + ci);
//   * each conv's epilogue (EpiPool) is bias -> ReLU -> batch norm folded to a scale and shift -> max over row pairs (the
//     2x1 pool), storing half the rows;
//   * classifier (4 * W5 -> 360), then the sigmoid.
// The network runs over at most NET_CHUNK frames at a time (torchcrepe's batch_size of the reference's call).
// Decode: one row kernel (mask, softmax, log) and one workgroup per (utterance, segment) for the Viterbi recursion.
#include "gemm_f32.h"

#include <algorithm>
#include <math.h>
#include <stddef.h>

namespace {

constexpr int WIN = 1024;                  // samples per CREPE frame
constexpr int C1_TAPS = 512, C1_STRIDE = 4, C1_PAD = 254;
constexpr int FRAME_LD = WIN + 2 * C1_PAD;  // 1532 floats per padded frame
constexpr int C1_POS = 256;                // conv1 output positions per frame
constexpr int TAPS = 64;                   // conv2..conv6
constexpr int BINS = 360;
constexpr int NET_CHUNK = 512;             // frames per network pass
constexpr float BN_EPS = 0.0010000000474974513f;
constexpr float CENTS0 = 1997.3794084376191f;
// librosa.sequence.viterbi in fp64: log(1/360 + tiny) (uniform start) and log(0 + tiny) (an out-of-band transition), tiny =
// fp32's smallest normal (util.tiny of the fp32 emissions)
constexpr double LOG_INIT = -0x1.78b5edaefba8cp+2;   // -5.886104031450156
constexpr double LOG_EPS = -0x1.5d589f2fe5107p+6;    // -87.3365447505531
constexpr float TINY_F = 1.17549435e-38f;
constexpr int BAND = 23;                   // in-band transitions |i - j| <= 11

// ---- GEMM epilogues --------------------------------------------------------------------------------------
// out[z * sO + (m / 2) * ldo + n] = max(y(m), y(m + 1)),  y = relu(acc + bias[n]) * scale[n] + shift[n]
struct EpiPool {
    float* out;
    int64_t ldo, sO;
    const float* bias;
    const float* scale;
    const float* shift;
    static constexpr bool kRowPair = true;
    __device__ __forceinline__ float col(int n) const { return bias[n]; }
    __device__ __forceinline__ void pair(int z, int m, int n, float a, float b, float cb) const {
        const float s = scale[n], t = shift[n];
        const float ya = fmaxf(a + cb, 0.f) * s + t;
        const float yb = fmaxf(b + cb, 0.f) * s + t;
        out[(int64_t)z * sO + (int64_t)(m >> 1) * ldo + n] = fmaxf(ya, yb);
    }
};

// Ragged batch: packed frame z of the real frames of all rows -> its row b (prefix[b] <= z < prefix[b + 1]; prefix: the (B + 1,)
// exclusive prefix sums of the rows' frame counts), held inside 0..B-1 whatever the table holds.
__device__ __forceinline__ int packed_row(const int32_t* __restrict__ prefix, int B, int64_t z) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)prefix[mid] <= z) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// x = sigmoid(x) (the classifier's activation; a separate pass keeps expf out of the GEMM epilogue's registers): in place, or
// (prefix != nullptr, ragged batch) from the pass's packed rows z0 + i / 360 to out (B, Fr, 360) at the frame's (row, frame)
__global__ void __launch_bounds__(256) sigmoid_kernel(float* __restrict__ x, int64_t n, const int32_t* __restrict__ prefix, int B,
                                                      int64_t z0, int64_t Fr, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float y = 1.0f / (1.0f + expf(-x[i]));
        if (!prefix) {
            x[i] = y;
            continue;
        }
        const int64_t z = z0 + i / BINS;
        const int b = packed_row(prefix, B, z);
        const int64_t f = z - (int64_t)prefix[b];
        if (f >= 0 && f < Fr) out[((int64_t)b * Fr + f) * BINS + i % BINS] = y;
    }
}

// ragged batch: one wave per (row, frame) of out (B, Fr, 360); the frames a row does not have are set to 0
__global__ void __launch_bounds__(256) tail_zero_kernel(float* __restrict__ out, int64_t Fr, int64_t rows,
                                                        const int32_t* __restrict__ prefix) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t b = row / Fr, f = row - b * Fr;
    if (f < (int64_t)prefix[b + 1] - (int64_t)prefix[b]) return;
    for (int j = lane; j < BINS; j += 64) out[row * BINS + j] = 0.f;
}

// ---- framing -----------------------------------------------------------------------------------------------
// block per frame z (of the chunk starting at frame z0 of the B * Fr flattened frames): 1532 floats, 254 zeros, the 1024
// normalised samples, 254 zeros.  Sample s of frame f reads audio[f * hop + s - 512] (zero outside the utterance).
// Ragged batch (prefix != nullptr): z counts the packed real frames, its (row, frame) comes from the prefix table, and the
// utterance ends at the row's own n16[b] samples: what follows them is never loaded.
__global__ void __launch_bounds__(256) frame_kernel(const float* __restrict__ audio, int64_t T, int64_t Fr, int hop, int64_t z0,
                                                    float* __restrict__ frames, const int32_t* __restrict__ n16,
                                                    const int32_t* __restrict__ prefix, int B) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t z = z0 + blockIdx.x;
    int64_t b = z / Fr, f = z % Fr;
    const int64_t ld = T;
    if (prefix) {
        b = packed_row(prefix, B, z);
        f = z - (int64_t)prefix[b];
        f = f < 0 ? 0 : f;
        const int64_t nb = n16[b];
        T = nb < 0 ? 0 : (nb < T ? nb : T);
    }
    const float* x = audio + b * ld;
    float v[4];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t idx = f * hop + tid + 256 * i - WIN / 2;
        v[i] = (idx >= 0 && idx < T) ? x[idx] : 0.f;
        s += (double)v[i];
    }
    s = wave_sum_d(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    const double mean = ((red[0] + red[1]) + (red[2] + red[3])) / WIN;
    __syncthreads();
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double d = (double)v[i] - mean;
        q += d * d;
    }
    q = wave_sum_d(q);
    if ((tid & 63) == 0) red[tid >> 6] = q;
    __syncthreads();
    const double sd = sqrt(((red[0] + red[1]) + (red[2] + red[3])) / (WIN - 1));
    const double den = sd > 1e-10 ? sd : 1e-10;
    float* out = frames + (int64_t)blockIdx.x * FRAME_LD;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[C1_PAD + tid + 256 * i] = (float)(((double)v[i] - mean) / den);
    if (tid < C1_PAD) {
        out[tid] = 0.f;
        out[C1_PAD + WIN + tid] = 0.f;
    }
}

// ---- weight preparation (one launch) ------------------------------------------------------------------------
struct PrepArgs {
    const float* w[6];
    const float* bn_w[6];
    const float* bn_b[6];
    const float* bn_mean[6];
    const float* bn_var[6];
    float* wpk[6];      // repacked conv2..conv6 (index 0 unused)
    float* scale[6];
    float* shift[6];
    int cin[6], cout[6];
    int64_t end[12];    // prefix ends of the work items: repack of layers 1..5, then the fold of layers 0..5
};

__global__ void __launch_bounds__(256) prep_kernel(PrepArgs a) {
    const int64_t total = a.end[10];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int s = 0;
        while (i >= a.end[s]) ++s;
        const int64_t r = i - (s ? a.end[s - 1] : 0);
        if (s < 5) {
            // (Cout, Cin, 64, 1) -> (Cout, tap * Cin + ci)
            const int l = s + 1, cin = a.cin[l];
            const int64_t co = r / ((int64_t)TAPS * cin);
            const int kk = (int)(r % ((int64_t)TAPS * cin)), t = kk / cin, ci = kk % cin;
            a.wpk[l][r] = a.w[l][(co * cin + ci) * TAPS + t];
        } else {
            const int l = s - 5, c = (int)r;
            const double sc = (double)a.bn_w[l][c] / sqrt((double)a.bn_var[l][c] + (double)BN_EPS);
            a.scale[l][c] = (float)sc;
            a.shift[l][c] = (float)((double)a.bn_b[l][c] - (double)a.bn_mean[l][c] * sc);
        }
    }
}

// ---- decode -------------------------------------------------------------------------------------------------
// one wave per frame: emissions log(softmax(masked probs) + tiny) (fp32), the mask [0, lo) and [hi, 360).  Ragged batch
// (n_frames != nullptr): a frame its row does not have is skipped - its activations are not read - and its entries of the
// decode's outputs (B, Fr) are set to 0 here, so the Viterbi workgroups write a row's own frames only.
__global__ void __launch_bounds__(256) emission_kernel(const float* __restrict__ probs, int64_t rows, int lo, int hi,
                                                       float* __restrict__ logp, const int32_t* __restrict__ n_frames, int64_t Fr,
                                                       float* __restrict__ f0, float* __restrict__ pd,
                                                       int32_t* __restrict__ bins_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    if (n_frames) {
        const int64_t b = row / Fr;
        if (row - b * Fr >= (int64_t)n_frames[b]) {
            if (lane == 0) {
                f0[row] = 0.f;
                pd[row] = 0.f;
                if (bins_out) bins_out[row] = 0;
            }
            return;
        }
    }
    const float* p = probs + row * BINS;
    float x[6];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int j = lane + 64 * i;
        x[i] = (j < BINS && j >= lo && j < hi) ? p[j] : -INFINITY;
        mx = fmaxf(mx, x[i]);
    }
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        x[i] = expf(x[i] - mx);   // masked: exp(-inf) = 0
        s += x[i];
    }
    s = wave_sum(s);
    float* o = logp + row * BINS;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int j = lane + 64 * i;
        if (j < BINS) o[j] = logf(x[i] / s + TINY_F);
    }
}

constexpr int VT = 384;        // threads of the Viterbi workgroup (6 waves; states j < 360)
constexpr int BT_ROWS = 64;    // back-pointer rows staged in LDS per backtracking block
constexpr int PF = 8;          // emission frames per prefetch block of the Viterbi recursion

__device__ __forceinline__ void argmax_merge(double& v, int& i, double v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}

// The dither seed of ddsp_crepe_decode (seed_dev) moves to its successor (one 64-bit LCG step, Knuth's MMIX constants: full
// period, both 32-bit halves change from call to call).  One thread, enqueued behind the decode that read the word.
__global__ void seed_advance_kernel(uint64_t* __restrict__ seed) {
    *seed = *seed * 6364136223846793005ull + 1442695040888963407ull;
}

// grid (segments, B).  Frames [t0, t1) of utterance b (of its own n_frames[b] <= Fr frames in a ragged batch: a piece that
// starts at or after them returns at once, the last piece ends - and its backtrack starts - at the row's own last frame, and
// the dither is drawn for the row-local frame, as a call on the row alone draws it), decoded on their own from a uniform start:
//   value[t][j] = logp[t][j] + max_i(value[t-1][i] + logT[i][j])  (fp64, first i on ties)
// computed exactly from the 23 in-band candidates and the out-of-band term value[t-1][g] + log(tiny), g = the first global
// argmax of value[t-1]: every in-band logT exceeds log(tiny), so an out-of-band i beats the band only if it is g.
__global__ void __launch_bounds__(VT) viterbi_kernel(const float* __restrict__ logp, const float* __restrict__ probs, int64_t Fr,
                                                     int64_t seg, int lo, int hi, uint16_t* __restrict__ ptr, uint64_t seed_arg,
                                                     const uint64_t* __restrict__ seed_dev, int dither,
                                                     float* __restrict__ f0, float* __restrict__ pd,
                                                     int32_t* __restrict__ bins_out, const int32_t* __restrict__ n_frames) {
    const int64_t t0 = (int64_t)blockIdx.x * seg;
    int64_t Frb = Fr;
    if (n_frames) {
        const int64_t nb = n_frames[blockIdx.y];
        Frb = nb < Fr ? nb : Fr;
        if (t0 >= Frb) return;
    }
    // the dither seed: the argument, or (seed_dev) the device word a captured graph re-reads on every replay
    const uint64_t seed = seed_dev ? *seed_dev : seed_arg;
    __shared__ double band[BINS * BAND];        // logT[j + d - 11][j] at [j * 23 + d]; reused for back-pointer rows
    __shared__ double val[2][BINS];
    __shared__ double rv[2][8];
    __shared__ int ri[2][8];
    __shared__ int16_t state[1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int n = (int)std::min<int64_t>(seg, Frb - t0);
    const float* lp = logp + ((int64_t)b * Fr + t0) * BINS;
    uint16_t* pt = ptr + ((int64_t)b * Fr + t0) * BINS;
    // transition table: row i of T is max(12 - |i - j|, 0) / sum_j(...), the sum exact in integers
    for (int e = tid; e < BINS * BAND; e += VT) {
        const int j = e / BAND, d = e % BAND, i = j + d - 11;
        double v = -INFINITY;
        if (i >= 0 && i < BINS) {
            int rowsum = 0;
            for (int u = -11; u <= 11; ++u)
                if (i + u >= 0 && i + u < BINS) rowsum += 12 - (u < 0 ? -u : u);
            const int dd = d - 11 < 0 ? 11 - d : d - 11;
            v = log((double)(12 - dd) / (double)rowsum);   // (+ tiny: below half an ulp of any in-band entry)
        }
        band[e] = v;
    }
    // value[0] and its argmax
    double v = -INFINITY;
    if (tid < BINS) {
        v = (double)lp[tid] + LOG_INIT;
        val[0][tid] = v;
    }
    double wv = v;
    int wi = tid < BINS ? tid : 1 << 20;
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_xor(wv, o, 64);
        const int i2 = __shfl_xor(wi, o, 64);
        argmax_merge(wv, wi, v2, i2);
    }
    if (lane == 0) {
        rv[0][wave] = wv;
        ri[0][wave] = wi;
    }
    __syncthreads();
    // one step of the recursion (emission e of frame s); the barrier orders the LDS only - a __syncthreads() would also wait for
    // every outstanding global access of the thread (its back-pointer stores, the emission prefetch) on every step
    auto step = [&](int s, float e) {
        const int pb = (s - 1) & 1, cbuf = s & 1;
        double gv = rv[pb][0];
        int g = ri[pb][0];
        for (int w = 1; w < VT / 64; ++w) argmax_merge(gv, g, rv[pb][w], ri[pb][w]);
        double nv = -INFINITY;
        int ni = 1 << 20;
        if (tid < BINS) {
            const int j = tid;
            double best = -INFINITY;
            int bi = -1;
#pragma unroll
            for (int d = 0; d < BAND; ++d) {
                const int i = j + d - 11;
                if (i >= 0 && i < BINS) {
                    const double c = val[pb][i] + band[j * BAND + d];
                    if (c > best) {
                        best = c;
                        bi = i;
                    }
                }
            }
            if (g < j - 11 || g > j + 11) {
                const double c = gv + LOG_EPS;
                if (c > best || (c == best && g < bi)) {
                    best = c;
                    bi = g;
                }
            }
            nv = (double)e + best;
            ni = j;
            val[cbuf][j] = nv;
            pt[(int64_t)s * BINS + j] = (uint16_t)bi;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double v2 = __shfl_xor(nv, o, 64);
            const int i2 = __shfl_xor(ni, o, 64);
            argmax_merge(nv, ni, v2, i2);
        }
        if (lane == 0) {
            rv[cbuf][wave] = nv;
            ri[cbuf][wave] = ni;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // emissions PF frames ahead: the block after the current one is in flight while the current one is consumed
    float cur[PF], nxt[PF];
    auto load_block = [&](int base, float (&dst)[PF]) {
#pragma unroll
        for (int u = 0; u < PF; ++u) dst[u] = (tid < BINS && base + u < n) ? lp[(int64_t)(base + u) * BINS + tid] : 0.f;
    };
    load_block(1, cur);
    for (int base = 1; base < n; base += PF) {
        load_block(base + PF, nxt);
#pragma unroll
        for (int u = 0; u < PF; ++u)
            if (base + u < n) step(base + u, cur[u]);
#pragma unroll
        for (int u = 0; u < PF; ++u) cur[u] = nxt[u];
    }
    // backtrack from the first argmax of the last values; back-pointer rows staged through LDS, BT_ROWS at a time
    {
        const int pb = (n - 1) & 1;
        double gv = rv[pb][0];
        int g = ri[pb][0];
        for (int w = 1; w < VT / 64; ++w) argmax_merge(gv, g, rv[pb][w], ri[pb][w]);
        if (tid == 0) state[n - 1] = (int16_t)g;
    }
    uint16_t* rows = (uint16_t*)band;
    for (int hiRow = n - 1; hiRow >= 1; hiRow -= BT_ROWS) {
        const int loRow = hiRow - BT_ROWS + 1 > 1 ? hiRow - BT_ROWS + 1 : 1;
        __syncthreads();   // (the previous block's chase is done with the staging rows; state[] of hiRow + 1 is written)
        const int cnt = (hiRow - loRow + 1) * BINS;
        for (int e = tid; e < cnt; e += VT) rows[e] = pt[(int64_t)loRow * BINS + e];
        __syncthreads();
        if (tid == 0) {
            int st = state[hiRow];
            for (int r = hiRow; r >= loRow; --r) {
                st = rows[(r - loRow) * BINS + st];
                state[r - 1] = (int16_t)st;
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < n; t += VT) {
        const int bin = state[t];
        const int64_t o = (int64_t)b * Fr + t0 + t;
        float cents = (float)(20 * bin) + CENTS0;
        if (dither) {
            const uint64_t h = (uint64_t)(n_frames ? t0 + t : o);
            const float u1 = (float)(ddsp_hash32(seed, 2 * h) >> 8) * (1.0f / 16777216.0f);
            const float u2 = (float)(ddsp_hash32(seed, 2 * h + 1) >> 8) * (1.0f / 16777216.0f);
            cents = cents + 20.0f * ((u1 + u2) - 1.0f);   // triangular on (-20, 20), mode 0 (scipy triang(c=0.5))
        }
        f0[o] = 10.0f * exp2f(cents / 1200.0f);
        pd[o] = (bin >= lo && bin < hi) ? probs[o * BINS + bin] : -INFINITY;
        if (bins_out) bins_out[o] = bin;
    }
}

// ---- post-filter (one workgroup per utterance) -------------------------------------------------------------------
__device__ __forceinline__ int64_t reflect_idx(int64_t i, int64_t n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

__global__ void __launch_bounds__(256) postfilter_kernel(const float* __restrict__ f0, const float* __restrict__ pd, int64_t Fr,
                                                         int sr, double hop, int64_t n_frames, int64_t start_frame, float thr,
                                                         int uv_interp, float f0_min, float* __restrict__ pooled,
                                                         float* __restrict__ out, const int32_t* __restrict__ n_crepe,
                                                         const int32_t* __restrict__ n_out) {
    __shared__ int64_t first_v[256], last_v[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* f = f0 + (int64_t)b * Fr;
    const float* p = pd + (int64_t)b * Fr;
    float* pl = pooled + (int64_t)b * Fr;
    float* o = out + (int64_t)b * n_frames;
    if (n_crepe) {
        // ragged batch: the row's own frame counts stand for Fr and n_frames from here on (held inside 3..Fr and 0..n_frames),
        // and the frames of `out` after them are 0 - written once, and looked at by nothing below
        const int64_t cb = n_crepe[b], ob = n_out[b];
        for (int64_t n = (ob < 0 ? 0 : ob) + tid; n < n_frames; n += 256) o[n] = 0.f;
        Fr = cb < 3 ? 3 : (cb < Fr ? cb : Fr);
        n_frames = ob < 0 ? 0 : (ob < n_frames ? ob : n_frames);
    }
    // MedianPool1d(pd, 4) -> At(thr) -> MaskedAvgPool1d(f0, 4); window i = reflect(i - 1 .. i + 2)
    for (int64_t i = tid; i < Fr; i += 256) {
        float sum = 0.f, cnt = 0.f;
        float q[4], fv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t c = reflect_idx(i - 1 + k, Fr);
            // the median window of this position c of the threshold step: pd at reflect(c - 1 .. c + 2)
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = p[reflect_idx(c - 1 + u, Fr)];
            // lower median of 4: the second smallest (sorting network)
            float a0 = fminf(w[0], w[1]), a1 = fmaxf(w[0], w[1]), a2 = fminf(w[2], w[3]), a3 = fmaxf(w[2], w[3]);
            const float lo2 = fmaxf(a0, a2), hi2 = fminf(a1, a3);
            q[k] = fminf(lo2, hi2);
            fv[k] = q[k] < thr ? NAN : f[c];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = !isnan(fv[k]);
            sum = sum + (ok ? fv[k] : 0.f);
            cnt = cnt + (ok ? 1.f : 0.f);
        }
        pl[i] = sum / (cnt > 1.f ? cnt : 1.f);
    }
    __syncthreads();
    for (int64_t n = tid; n < n_frames; n += 256) {
        float v = 0.f;
        if (n >= start_frame) {
            const double x = (double)(n - start_frame) * hop / (double)sr / 0.005;
            int64_t idx = (int64_t)rint(x);
            idx = idx < Fr - 1 ? idx : Fr - 1;
            v = pl[idx];
        }
        o[n] = v;
    }
    if (!uv_interp) return;
    __syncthreads();
    const int64_t chunk = (n_frames + 255) / 256, c0 = tid * chunk, c1 = std::min<int64_t>(n_frames, c0 + chunk);
    int64_t fv = n_frames, lv = -1;
    for (int64_t i = c0; i < c1; ++i)
        if (o[i] != 0.f) {
            if (fv == n_frames) fv = i;
            lv = i;
        }
    first_v[tid] = fv;
    last_v[tid] = lv;
    __syncthreads();
    int64_t prev = -1, next = n_frames, any = n_frames;
    for (int u = 0; u < 256; ++u) {
        if (u < tid) prev = last_v[u] > prev ? last_v[u] : prev;
        if (u > tid) next = first_v[u] < next ? first_v[u] : next;
        any = first_v[u] < any ? first_v[u] : any;
    }
    if (any < n_frames) {
        // numpy.interp over the zero frames: runs [i, k) of zeros between voiced neighbours xl < i and xr >= k
        int64_t i = c0;
        while (i < c1) {
            if (o[i] != 0.f) {
                prev = i;
                ++i;
                continue;
            }
            int64_t k = i;
            while (k < c1 && o[k] == 0.f) ++k;
            const int64_t xr = k < c1 ? k : next, xl = prev;
            for (int64_t x = i; x < k; ++x) {
                double r;
                if (xl < 0) {
                    r = (double)o[xr];
                } else if (xr >= n_frames) {
                    r = (double)o[xl];
                } else {
                    const double yl = (double)o[xl], yr = (double)o[xr];
                    const double slope = (yr - yl) / ((double)xr - (double)xl);
                    r = slope * ((double)x - (double)xl) + yl;
                }
                o[x] = (float)r;
            }
            i = k;
        }
    }
    __syncthreads();
    for (int64_t x = c0; x < c1; ++x)
        if (o[x] < f0_min) o[x] = f0_min;
}

// ---- network -------------------------------------------------------------------------------------------------
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Dims {
    int cin[6], cout[6], pos[6];   // input channels, output channels, output positions per frame (before the pool)
    int feat;                      // classifier inputs
};

Dims dims_of(const ddsp_crepe_weights& w) {
    Dims d;
    for (int l = 0; l < 6; ++l) {
        d.cout[l] = w.width[l];
        d.cin[l] = l ? w.width[l - 1] : 1;
        d.pos[l] = C1_POS >> l;
    }
    d.feat = 4 * w.width[5];
    return d;
}

size_t prep_floats(const Dims& d, size_t (&off)[13]) {
    // wpk[1..5], scale[0..5], shift[0..5]
    size_t o = 0;
    for (int l = 1; l < 6; ++l) {
        off[l - 1] = o;
        o += align256((size_t)d.cout[l] * d.cin[l] * TAPS * 4) / 4;
    }
    for (int l = 0; l < 6; ++l) {
        off[5 + l] = o;
        o += 2 * (align256((size_t)d.cout[l] * 4) / 4);
    }
    off[11] = o;
    return o;
}

int prepare(ddsp_ctx* ctx, hipStream_t st, const ddsp_crepe_weights& w, const Dims& d, float* base) {
    size_t off[13];
    prep_floats(d, off);
    PrepArgs a;
    int64_t e = 0;
    for (int l = 0; l < 6; ++l) {
        a.w[l] = w.conv_w[l];
        a.bn_w[l] = w.bn_w[l];
        a.bn_b[l] = w.bn_b[l];
        a.bn_mean[l] = w.bn_mean[l];
        a.bn_var[l] = w.bn_var[l];
        a.cin[l] = d.cin[l];
        a.cout[l] = d.cout[l];
        a.wpk[l] = l ? base + off[l - 1] : nullptr;
        a.scale[l] = base + off[5 + l];
        a.shift[l] = base + off[5 + l] + align256((size_t)d.cout[l] * 4) / 4;
    }
    for (int l = 1; l < 6; ++l) a.end[l - 1] = (e += (int64_t)d.cout[l] * d.cin[l] * TAPS);
    for (int l = 0; l < 6; ++l) a.end[5 + l] = (e += d.cout[l]);
    a.end[11] = e;
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(e, 256), 8192)), dim3(256), 0, st, a);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

bool weights_complete(const ddsp_crepe_weights& w) {
    const float* const* p = (const float* const*)&w;
    const size_t n = offsetof(ddsp_crepe_weights, width) / sizeof(const float*);
    for (size_t i = 0; i < n; ++i)
        if (!p[i] || ((uintptr_t)p[i] % 16) != 0) return false;
    for (int l = 0; l < 6; ++l)
        if (w.width[l] < 16 || w.width[l] % 16 || w.width[l] > 4096) return false;
    return true;
}

// implicit-im2col conv of one layer (l >= 1) with the pooling epilogue: tile by the launch size; Cin % 32 == 0 -> LDS-DMA
template <class Epi>
void conv_gemm(hipStream_t st, gemm::Args g, const Epi& e) {
    auto blocks = [&](int bm, int bn) { return (int64_t)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn); };
    if (g.Cin % 32 == 0 && g.zeros) {
        if (g.N % 128 == 0 && blocks(128, 128) >= 256)
            gemm::dma_go<128, 128, Epi, 2, 8, gemm::A_CONVK>(st, g, 1, e);
        else if (blocks(128, 64) >= 256)
            gemm::dma_go<128, 64, Epi, 3, 8, gemm::A_CONVK>(st, g, 1, e);
        else
            gemm::dma_go<64, 64, Epi, 3, 4, gemm::A_CONVK>(st, g, 1, e);
    } else if (blocks(128, 64) >= 512) {
        gemm::launch_tile<128, 64, true, true, gemm::A_CONVK, Epi, 8>(st, g, 1, e);
    } else {
        gemm::launch_tile<64, 64, true, true, gemm::A_CONVK, Epi, 4>(st, g, 1, e);
    }
}

// n16 / prefix / n_packed: a ragged batch - the network runs over the n_packed real frames of all rows, in passes that may
// hold frames of several rows; nullptr: the B * Fr frames of a rectangular batch.
int crepe_run(ddsp_ctx* ctx, hipStream_t st, const ddsp_crepe_weights* wp, const float* audio, int64_t B, int64_t T, int hop,
              float* probs, const int32_t* n16, const int32_t* prefix, int64_t n_packed) {
    DDSP_REQUIRE(ctx, ctx && wp && audio && probs, "ddsp_crepe_activations: null argument");
    DDSP_REQUIRE(ctx, weights_complete(*wp), "ddsp_crepe_activations: a weight pointer is null or not 16-byte aligned, or a width is not a multiple of 16");
    DDSP_REQUIRE(ctx, B >= 1 && T >= 0 && hop >= 1, "ddsp_crepe_activations: bad shape");
    const int64_t Fr = 1 + T / hop;
    DDSP_REQUIRE(ctx, B * Fr < ((int64_t)1 << 31) / BINS && (Fr - 1) * (int64_t)hop < ((int64_t)1 << 40), "ddsp_crepe_activations: input too long");
    const int64_t n_run = prefix ? n_packed : B * Fr;   // frames the network runs over
    const ddsp_crepe_weights w = *wp;
    const Dims d = dims_of(w);
    DDSP_ENTER_DEVICE(ctx);
    const int math = ctx->math == DDSP_MATH_FP32 ? 0 : 3;
    const float* zeros = nullptr;
    int rc = ddsp_zero_page(ctx, &zeros);
    if (rc) return rc;

    size_t off[13];
    const size_t pfl = prep_floats(d, off);
    ddsp_weight_slot* slot;
    rc = ddsp_weight_slot_take(ctx, st, ctx->crepe_slot, &w, offsetof(ddsp_crepe_weights, version), w.version, pfl * 4, &slot, true);
    if (rc) return rc;
    float* prep = nullptr;
    if (slot) {
        prep = (float*)slot->dev;
        if (!(slot->state & 1)) {
            if ((rc = prepare(ctx, st, w, d, prep))) return rc;
            slot->state = 1;
        }
    }
    // arena: [prepared weights (when not cached)] [ping: frames / conv2 / conv4 / conv6 outputs] [pong: conv1 / conv3 / conv5]
    const int64_t zc_max = std::min<int64_t>(n_run, NET_CHUNK);
    size_t ping = (size_t)zc_max * FRAME_LD, pong = 0;
    for (int l = 0; l < 6; ++l) {
        const size_t sz = (size_t)zc_max * (d.pos[l] / 2) * d.cout[l];
        if (l & 1) ping = std::max(ping, sz); else pong = std::max(pong, sz);
    }
    // (ragged: the classifier's rows of a pass, before the sigmoid carries them to their (row, frame) of probs)
    const size_t cls = prefix ? (size_t)zc_max * BINS : 0;
    const size_t total = align256(pfl * 4) + align256(ping * 4) + align256(pong * 4) + align256(cls * 4);
    // (the arena always has room for the prepared weights: a capture after cached warm-up calls must not have to grow it)
    if ((rc = ddsp_scratch_reserve_bytes(ctx, total + 4096))) return rc;
    ddsp_scratch_reset(ctx);
    void* arena = nullptr;
    if ((rc = ddsp_scratch_get(ctx, total, &arena))) return rc;
    char* a = (char*)arena;
    if (!prep) {
        prep = (float*)a;
        if ((rc = prepare(ctx, st, w, d, prep))) return rc;
    }
    float* P = (float*)(a + align256(pfl * 4));
    float* Q = (float*)(a + align256(pfl * 4) + align256(ping * 4));
    float* L = (float*)(a + align256(pfl * 4) + align256(ping * 4) + align256(pong * 4));
    auto scale_of = [&](int l) { return prep + off[5 + l]; };
    auto shift_of = [&](int l) { return prep + off[5 + l] + align256((size_t)d.cout[l] * 4) / 4; };

    if (prefix)
        hipLaunchKernelGGL(tail_zero_kernel, dim3((unsigned)ceil_div64(B * Fr, 4)), dim3(256), 0, st, probs, Fr, B * Fr, prefix);
    for (int64_t z0 = 0; z0 < n_run; z0 += NET_CHUNK) {
        const int zc = (int)std::min<int64_t>(n_run - z0, NET_CHUNK);
        hipLaunchKernelGGL(frame_kernel, dim3((unsigned)zc), dim3(256), 0, st, audio, T, Fr, hop, z0, P, n16, prefix, (int)B);
        {   // conv1: batched over the frames, rows 4 floats apart
            gemm::Args g = gemm::make(P, C1_STRIDE, w.conv_w[0], C1_TAPS, C1_POS, d.cout[0], C1_TAPS);
            g.sA_hi = FRAME_LD;
            g.math = math;
            EpiPool e{Q, d.cout[0], (int64_t)(C1_POS / 2) * d.cout[0], w.conv_b[0], scale_of(0), shift_of(0)};
            if (d.cout[0] % 128 == 0)
                gemm::dma_go<128, 128, EpiPool, 2>(st, g, zc, e);
            else
                gemm::dma_go<64, 64, EpiPool, 3, 4>(st, g, zc, e);
        }
        float* x = Q;
        float* y = P;
        for (int l = 1; l < 6; ++l) {
            const int Fin = d.pos[l - 1] / 2;   // positions per frame of this layer's input (= its output before the pool)
            gemm::Args g = gemm::make(x, d.cin[l], prep + off[l - 1], (int64_t)TAPS * d.cin[l], zc * Fin, d.cout[l], TAPS * d.cin[l]);
            g.Fr = Fin;
            g.Cin = d.cin[l];
            g.ktaps = TAPS;
            g.dil = 1;
            g.zeros = zeros;
            g.math = math;
            EpiPool e{y, d.cout[l], 0, w.conv_b[l], scale_of(l), shift_of(l)};
            conv_gemm(st, g, e);
            std::swap(x, y);
        }
        // classifier over (position, channel) features: rows of 4 * W5 floats
        {
            gemm::Args g = gemm::make(x, d.feat, w.cls_w, d.feat, zc, BINS, d.feat);
            g.math = math;
            float* logits = prefix ? L : probs + z0 * BINS;
            gemm::launch<true, true, gemm::A_PLAIN>(st, g, 1, gemm::EpiStore{logits, BINS, w.cls_b, 1, 0, 0});
            const int64_t n = (int64_t)zc * BINS;
            hipLaunchKernelGGL(sigmoid_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, logits, n, prefix, (int)B, z0, Fr,
                               probs);
        }
    }
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// torchcrepe.convert.frequency_to_bins in fp32, then Python's slice rules for [:minidx] / [maxidx:] over 360 bins
int bin_of(float f, bool ceil_) {
    const float c = 1200.f * log2f(f / 10.f);
    const float x = (c - CENTS0) / 20.f;
    return (int)(ceil_ ? ceilf(x) : floorf(x));
}
int slice_pos(int k) { return k < 0 ? std::max(BINS + k, 0) : std::min(k, BINS); }

}  // namespace

extern "C" int64_t ddsp_crepe_frames(int64_t T16, int hop) {
    if (T16 < 0 || hop < 1) return -1;
    return 1 + T16 / hop;
}

// n_samples, frame_prefix and n_packed: all three (a ragged batch) or none (n_packed is then not read)
extern "C" int ddsp_crepe_activations(ddsp_ctx* ctx, void* stream, const ddsp_crepe_weights* w, const float* audio16, int64_t B,
                                      int64_t T, const int32_t* n_samples, const int32_t* frame_prefix, int64_t n_packed, int hop,
                                      float* probs) {
    DDSP_REQUIRE(ctx, ctx && !n_samples == !frame_prefix,
                 "ddsp_crepe_activations: n_samples and frame_prefix are given together or not at all");
    DDSP_REQUIRE(ctx, !n_samples || (B >= 1 && B < ((int64_t)1 << 31) && hop >= 1 && T >= 0 && n_packed >= B &&
                                     n_packed <= B * (1 + T / hop)),
                 "ddsp_crepe_activations: n_packed must lie in B..B * frames(T)");
    return crepe_run(ctx, (hipStream_t)stream, w, audio16, B, T, hop, probs, n_samples, frame_prefix, n_packed);
}

// n_frames: the rows' own frame counts, or null; seed_dev: the dither seed in device memory, or null (dither_seed by value)
extern "C" int ddsp_crepe_decode(ddsp_ctx* ctx, void* stream, const float* probs, int64_t B, int64_t Fr, const int32_t* n_frames,
                                 float fmin, float fmax, int64_t segment, uint64_t dither_seed, uint64_t* seed_dev, int use_dither,
                                 float* f0, float* periodicity, int32_t* bins) {
    DDSP_REQUIRE(ctx, ctx && ((uintptr_t)seed_dev & 7) == 0, "ddsp_crepe_decode: seed_dev not 8-byte aligned");
    DDSP_REQUIRE(ctx, !(seed_dev && n_frames), "ddsp_crepe_decode: seed_dev is not available with n_frames (a ragged batch)");
    if (seed_dev) dither_seed = 0;   // (not read by the kernels then)
    DDSP_REQUIRE(ctx, ctx && probs && f0 && periodicity, "ddsp_crepe_decode: null argument");
    DDSP_REQUIRE(ctx, B >= 1 && Fr >= 1 && B * Fr < ((int64_t)1 << 31) / BINS, "ddsp_crepe_decode: bad shape");
    DDSP_REQUIRE(ctx, fmin > 0.f && fmax > 0.f && isfinite(fmin) && isfinite(fmax), "ddsp_crepe_decode: fmin, fmax > 0");
    DDSP_REQUIRE(ctx, segment >= 0, "ddsp_crepe_decode: segment >= 0");
    const int64_t seg = segment == 0 ? Fr : std::min<int64_t>(segment, Fr);
    DDSP_REQUIRE(ctx, seg <= 1024, "ddsp_crepe_decode: segments of at most 1024 frames");
    const int lo = slice_pos(bin_of(fmin, false)), hi = slice_pos(bin_of(fmax, true));
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    const size_t rows = (size_t)B * Fr;
    const size_t total = align256(rows * BINS * 4) + align256(rows * BINS * 2);
    int rc = ddsp_scratch_reserve_bytes(ctx, total + 4096);
    if (rc) return rc;
    ddsp_scratch_reset(ctx);
    void* arena = nullptr;
    if ((rc = ddsp_scratch_get(ctx, total, &arena))) return rc;
    float* logp = (float*)arena;
    uint16_t* ptr = (uint16_t*)((char*)arena + align256(rows * BINS * 4));
    hipLaunchKernelGGL(emission_kernel, dim3((unsigned)ceil_div64((int64_t)rows, 4)), dim3(256), 0, st, probs, (int64_t)rows, lo, hi, logp,
                       n_frames, Fr, f0, periodicity, bins);
    hipLaunchKernelGGL(viterbi_kernel, dim3((unsigned)ceil_div64(Fr, seg), (unsigned)B), dim3(VT), 0, st, logp, probs, Fr, seg, lo, hi,
                       ptr, dither_seed, (const uint64_t*)seed_dev, use_dither ? 1 : 0, f0, periodicity, bins, n_frames);
    // every workgroup of the decode has read the word when this one-thread kernel, next on the stream, advances it
    if (seed_dev) hipLaunchKernelGGL(seed_advance_kernel, dim3(1), dim3(1), 0, st, seed_dev);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// n_crepe and n_out: both (a ragged batch, start_frame = 0) or neither
extern "C" int ddsp_f0_postfilter(ddsp_ctx* ctx, void* stream, const float* f0, const float* pd, int64_t B, int64_t Fr,
                                  const int32_t* n_crepe, int sr, double hop, int64_t n_frames, int64_t start_frame,
                                  const int32_t* n_out, float threshold, int uv_interp, float f0_min, float* out) {
    DDSP_REQUIRE(ctx, ctx && !n_crepe == !n_out, "ddsp_f0_postfilter: n_crepe and n_out are given together or not at all");
    DDSP_REQUIRE(ctx, !n_crepe || start_frame == 0, "ddsp_f0_postfilter: start_frame must be 0 with n_crepe / n_out (a ragged batch)");
    DDSP_REQUIRE(ctx, ctx && f0 && pd && out, "ddsp_f0_postfilter: null argument");
    DDSP_REQUIRE(ctx, B >= 1 && B < 65536 && Fr >= 3, "ddsp_f0_postfilter: B >= 1 and at least 3 frames (the reflect padding)");
    DDSP_REQUIRE(ctx, sr > 0 && hop > 0.0 && isfinite(hop), "ddsp_f0_postfilter: sr, hop > 0");
    DDSP_REQUIRE(ctx, n_frames >= 1 && start_frame >= 0 && start_frame <= n_frames, "ddsp_f0_postfilter: bad frame counts");
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    const size_t total = align256((size_t)B * Fr * 4);
    int rc = ddsp_scratch_reserve_bytes(ctx, total + 4096);
    if (rc) return rc;
    ddsp_scratch_reset(ctx);
    void* arena = nullptr;
    if ((rc = ddsp_scratch_get(ctx, total, &arena))) return rc;
    hipLaunchKernelGGL(postfilter_kernel, dim3((unsigned)B), dim3(256), 0, st, f0, pd, Fr, sr, hop, n_frames, start_frame, threshold,
                       uv_interp ? 1 : 0, f0_min, (float*)arena, out, n_crepe, n_out);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
