// a4: the unit -> control network (conv prenet + side embeddings + 3 x [Performer attention, Conformer conv
// module] + LayerNorm + weight-normed head), non-causal or causal (`c: true`): weight preparation and the forward pass.
// The backward pass is in unit2ctrl_bwd.hip, what both share in u2c.h.
//
// Replaces ddsp/unit2control.py:23-101 and ddsp/pcmer.py:11-63,69-77,123-159,191-251.
// Activations live frame-major (rows = B*Fr frames, 256/512/1024 channels contiguous), so every Linear /
// 1x1 conv is a plain row-major GEMM and the k=3 convolutions are GEMMs with an implicit im2col loader
// (gemm_f32.h, A_CONV3).  The products run in the context's arithmetic (ddsp_ctx_set_math): by default split-bf16, every
// fp32 product formed from three bf16 matrix products (hi*hi + hi*lo + lo*hi); DDSP_MATH_FP32 runs them on the fp32
// matrix pipe.  The training forward (activations kept for the backward pass) stays on fp32 MFMA.
// Linear attention is evaluated per (utterance, head) with batched GEMMs: k'^T v (266x64 context) and
// q' ctx; the softmax-kernel feature maps are a GEMM against the fixed 266x64 projection followed by a
// row-wise exp pass.  Everything else (GroupNorm, LayerNorm, GLU, depthwise k=31 conv + SiLU, embeddings,
// weight-norm) is small fused elementwise / row-reduction kernels.
#include "gemm_f32.h"
#include "gemm_ws.h"
#include "gemm_ln.h"
#include "performer_attn.h"
#include "u2c.h"

using namespace u2c;

namespace {

// ---- weight preparation --------------------------------------------------------------------------
// Every GEMM weight of a forward is re-packed by ONE launch (u2c_prepare_kernel).  Each job produces groups of 8
// consecutive k-values of one packed row and stores them either as 8 floats or, for the split-bf16 GEMMs that read B
// already split (gemm::Args::B_split), as 8 bf16 hi parts | 8 bf16 lo parts - the same 32 bytes.
__device__ __forceinline__ void store_group8(float* __restrict__ dst, const float (&x)[8], bool split) {
    if (split) {
        ddsp_u32x4 hi, lo;
        ddsp_split8(x, hi, lo);
        *(ddsp_u32x4*)dst = hi;
        *(ddsp_u32x4*)(dst + 4) = lo;
    } else {
        *(f32x4*)dst = f32x4{x[0], x[1], x[2], x[3]};
        *(f32x4*)(dst + 4) = f32x4{x[4], x[5], x[6], x[7]};
    }
}

// conv weight (Cout, Cin, 3) -> (Cout, 3*Cin) with k = tap*Cin + c  (matches gemm A_CONV3); Cin % 8 == 0
__device__ __forceinline__ void pack_conv3_body(const float* __restrict__ w, int Cout, int Cin, float* __restrict__ out,
                                                int vb, int vgrid, bool split) {   // vb / vgrid: block id / grid size of this job
    const int64_t groups = (int64_t)Cout * 3 * (Cin / 8);
    for (int64_t gi = (int64_t)vb * 256 + threadIdx.x; gi < groups; gi += (int64_t)vgrid * 256) {
        const int c8 = (int)(gi % (Cin / 8));
        const int tap = (int)((gi / (Cin / 8)) % 3);
        const int o = (int)(gi / (3 * (Cin / 8)));
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = w[((int64_t)o * Cin + 8 * c8 + e) * 3 + tap];
        store_group8(out + (int64_t)o * 3 * Cin + (int64_t)tap * Cin + 8 * c8, x, split);
    }
}
// fp32 variant for a Cin that is only a multiple of 4 (small problems that run the register-staged kernel)
__device__ __forceinline__ void pack_conv3_scalar_body(const float* __restrict__ w, int Cout, int Cin, float* __restrict__ out,
                                                       int vb, int vgrid) {
    const int64_t total = (int64_t)Cout * Cin * 3;
    for (int64_t i = (int64_t)vb * 256 + threadIdx.x; i < total; i += (int64_t)vgrid * 256) {
        const int tap = (int)(i % 3);
        const int c = (int)((i / 3) % Cin);
        const int o = (int)(i / (3 * Cin));
        out[(int64_t)o * 3 * Cin + (int64_t)tap * Cin + c] = w[i];
    }
}

// a plain (rows, K) matrix copied row by row (K % 8 == 0): the out-projection and pw2 weights for the split GEMMs
__device__ __forceinline__ void pack_copy_body(const float* __restrict__ w, int64_t n, float* __restrict__ out, int vb,
                                               int vgrid, bool split) {
    typedef gemm::f32x4_u v4;
    for (int64_t gi = (int64_t)vb * 256 + threadIdx.x; gi < n / 8; gi += (int64_t)vgrid * 256) {
        const v4 a = *(const v4*)(w + 8 * gi), c = *(const v4*)(w + 8 * gi + 4);
        const float x[8] = {a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
        store_group8(out + 8 * gi, x, split);
    }
}

// q/k/v projections as ONE GEMM: rows [q_w; k_w; v_w] (3*512 x 256) and the three biases behind each other
__device__ __forceinline__ void pack_qkv_body(const float* __restrict__ qw, const float* __restrict__ kw,
                                              const float* __restrict__ vw, const float* __restrict__ qb,
                                              const float* __restrict__ kb, const float* __restrict__ vb_,
                                              float* __restrict__ w, float* __restrict__ bias, int vb, int vgrid, bool split) {
    typedef gemm::f32x4_u v4;
    const int n = INNER * D;
    for (int gi = vb * 256 + threadIdx.x; gi < 3 * n / 8; gi += vgrid * 256) {
        const int i = 8 * gi, which = i / n, j = i - which * n;
        const float* src = (which == 0 ? qw : (which == 1 ? kw : vw)) + j;
        const v4 a = *(const v4*)src, c = *(const v4*)(src + 4);
        const float x[8] = {a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
        store_group8(w + i, x, split);
        if (j < INNER) {
            const float* bs = which == 0 ? qb : (which == 1 ? kb : vb_);
#pragma unroll
            for (int e = 0; e < 8; ++e) bias[which * INNER + j + e] = bs[j + e];
        }
    }
}

// pw1 (1024 x 256, rows 0..511 values, 512..1023 gates of the GLU, ddsp/pcmer.py conformer conv module) re-ordered
// for the gated-pair GEMM epilogue: packed rows 64t..64t+31 = values, 64t+32..64t+63 = gates of channels 32t..32t+31.
__device__ __forceinline__ void pack_glu_body(const float* __restrict__ w, const float* __restrict__ bias,
                                              float* __restrict__ wo, float* __restrict__ bo, int vb, int vgrid, bool split) {
    for (int i = vb * 256 + threadIdx.x; i < 2 * INNER * (D / 8); i += vgrid * 256) {
        const int p = i / (D / 8), k8 = (i % (D / 8)) * 8;
        const int t = p >> 6, within = p & 63;
        const int src = within < 32 ? 32 * t + within : INNER + 32 * t + (within - 32);
        const f32x4 a = *(const f32x4*)(w + (size_t)src * D + k8), c = *(const f32x4*)(w + (size_t)src * D + k8 + 4);
        const float x[8] = {a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
        store_group8(wo + (size_t)p * D + k8, x, split);
        if (k8 == 0) bo[p] = bias[src];
    }
}

struct EpiGlu {  // out[m][c] = (a + bias_a) * sigmoid(g + bias_g), formed inside the GEMM (see gemm_f32.h kGatedPair)
    static constexpr bool kGatedPair = true;
    float* out;          // (rows, 512)
    const float* bias;   // packed like the weight rows
    __device__ __forceinline__ float col(int n) const { return bias[n]; }
    __device__ __forceinline__ void store4(int, int m, int n, f32x4 v) const { *(f32x4*)(out + (int64_t)m * INNER + n) = v; }
};

struct EpiSplit3 {  // column block n / 512 selects the destination matrix (q, k or v), each (rows, 512)
    float* out[3];
    const float* bias;
    __device__ __forceinline__ float col(int n) const { return bias[n]; }
    __device__ __forceinline__ void operator()(int, int m, int n, float v, float cb) const {
        out[n >> 9][(int64_t)m * INNER + (n & (INNER - 1))] = v + cb;
    }
    static constexpr bool kStore4 = true;
    __device__ __forceinline__ bool vec_ok() const {
        return (((uintptr_t)out[0] | (uintptr_t)out[1] | (uintptr_t)out[2]) % 16) == 0;
    }
    __device__ __forceinline__ void store4(int, int m, int n, f32x4 v) const {
        *(f32x4*)(out[n >> 9] + (int64_t)m * INNER + (n & (INNER - 1))) = v + *(const gemm::f32x4_u*)(bias + n);
    }
};

// W[o][:] = g[o] * v[o][:] / ||v[o]||_2   (old-style weight_norm, ddsp/unit2control.py:61); one wave per row
__device__ __forceinline__ void weight_norm_body(const float* __restrict__ g, const float* __restrict__ v, int n_out,
                                                 int n_in, float* __restrict__ w, int vb, bool split) {
    const int lane = threadIdx.x & 63;
    const int o = vb * 4 + (threadIdx.x >> 6);
    if (o >= n_out) return;
    const float* row = v + (int64_t)o * n_in;
    float ss = 0.f;
    for (int i = lane; i < n_in; i += 64) ss = fmaf(row[i], row[i], ss);
    ss = wave_sum(ss);
    const float scale = g[o] / sqrtf(ss);
    if (n_in % 8 == 0) {
        for (int i = 8 * lane; i < n_in; i += 512) {
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = row[i + e] * scale;
            store_group8(w + (int64_t)o * n_in + i, x, split);
        }
    } else {
        for (int i = lane; i < n_in; i += 64) w[(int64_t)o * n_in + i] = row[i] * scale;
    }
}

// All weight preparation of one forward in ONE launch (it used to be 6-7: two conv packs, the head's weight norm,
// three QKV packs, the GLU re-ordering): the jobs are independent, each gets a range of blocks.  It runs when the
// context's prepared-weight slot does not already hold this layout of these weights (U2CBufs::wstate), and on every call
// that has no slot (weights without a change counter, stream capture).
struct PrepArgs {
    ddsp_u2c_weights w;
    float *w1, *w2, *wh, *wqkv, *bqkv, *wglu, *bglu, *wdw, *wout, *wpw2;
    int end[7];          // one past the last block of: conv1 | conv2 | head | qkv (3 layers) | glu (3 layers, may be empty) |
                         // out-projection + pw2 copies (3 layers each, split mode only) | dw taps
    int qkv_blocks, glu_blocks, copy_blocks;   // blocks per layer
    int split;           // the packed matrices are written as bf16 hi/lo groups (gemm::Args::B_split)
};
__global__ void __launch_bounds__(256) u2c_prepare_kernel(PrepArgs a) {
    const int b = blockIdx.x;
    const bool split = a.split != 0;
    if (b < a.end[0]) {
        if (a.w.n_unit % 8 == 0)
            pack_conv3_body(a.w.prenet_conv1_w, D, a.w.n_unit, a.w1, b, a.end[0], split);
        else
            pack_conv3_scalar_body(a.w.prenet_conv1_w, D, a.w.n_unit, a.w1, b, a.end[0]);
    } else if (b < a.end[1]) {
        pack_conv3_body(a.w.prenet_conv2_w, D, D, a.w2, b - a.end[0], a.end[1] - a.end[0], split);
    } else if (b < a.end[2]) {
        weight_norm_body(a.w.head_g, a.w.head_v, a.w.n_out, D, a.wh, b - a.end[1], split);
    } else if (b < a.end[3]) {
        const int r = b - a.end[2], l = r / a.qkv_blocks;
        const ddsp_u2c_layer& L = a.w.layer[l];
        pack_qkv_body(L.q_w, L.k_w, L.v_w, L.q_b, L.k_b, L.v_b, a.wqkv + (size_t)l * 3 * INNER * D,
                      a.bqkv + (size_t)l * 3 * INNER, r - l * a.qkv_blocks, a.qkv_blocks, split);
    } else if (b < a.end[4]) {
        const int r = b - a.end[3], l = r / a.glu_blocks;
        const ddsp_u2c_layer& L = a.w.layer[l];
        pack_glu_body(L.cm_pw1_w, L.cm_pw1_b, a.wglu + (size_t)l * 2 * INNER * D, a.bglu + (size_t)l * 2 * INNER,
                      r - l * a.glu_blocks, a.glu_blocks, split);
    } else if (b < a.end[5]) {
        const int r = b - a.end[4], j = r / a.copy_blocks, l = j >> 1;     // job j: layer j/2, out-projection | pw2
        const ddsp_u2c_layer& L = a.w.layer[l];
        pack_copy_body((j & 1) ? L.cm_pw2_w : L.out_w, (int64_t)D * INNER, ((j & 1) ? a.wpw2 : a.wout) + (size_t)l * D * INNER,
                       r - j * a.copy_blocks, a.copy_blocks, true);
    } else {
        // depthwise taps (512, 1, 31) -> [tap][channel], all three layers: 3 * 31 * 512 elements
        for (int i = (b - a.end[5]) * 256 + threadIdx.x; i < 3 * DWK * INNER; i += (a.end[6] - a.end[5]) * 256) {
            const int l = i / (DWK * INNER), r = i - l * DWK * INNER;
            const int t = r / INNER, c = r - t * INNER;
            a.wdw[i] = a.w.layer[l].cm_dw_w[c * DWK + t];
        }
    }
}

// ---- GroupNorm(4, 256) over (64 channels x all frames) per utterance + LeakyReLU -------------------
constexpr int GN_LANES = 16;   // frame lanes (waves) per block of the statistics kernel
// part != null (small batches, conv1 run as a K-split): x[row][ch] is first completed as bias[ch] + sum_s part[s][row][ch]
// (rows = all frames of the call) and written back for the normalisation pass.
__global__ void __launch_bounds__(64 * GN_LANES) groupnorm_stats_kernel(float* __restrict__ x, int Fr, float* __restrict__ stats,
                                                                       const float* __restrict__ part = nullptr,
                                                                       const float* __restrict__ bias = nullptr, int64_t rows = 0,
                                                                       const int* __restrict__ n_frames = nullptr) {
    // block = (group g, utterance b); 1024 threads = 64 channels x 16 frame lanes.  (With 4 frame lanes every thread
    // walked 43 dependent loads, one in flight at a time: 14 us for 11 MB.  The sums are combined in a fixed order.)
    const int g = blockIdx.x, b = blockIdx.y;
    const int c = threadIdx.x & 63, fl = threadIdx.x >> 6;
    float* base = x + ((int64_t)b * Fr) * D + g * 64 + c;
    // ragged batch: the statistics run over the row's own nv frames (the completed rows are still written for all Fr)
    const int nv = ddsp_row_frames(n_frames, b, Fr);
    double s = 0.0, ss = 0.0;
    int f = fl;
    if (part) {
        const float* pb = part + ((int64_t)b * Fr) * D + g * 64 + c;
        const float bc = bias[g * 64 + c];
        for (int ff = fl; ff < Fr; ff += GN_LANES) {
            const int64_t o = (int64_t)ff * D;
            const float v = ((pb[o] + pb[rows * D + o]) + (pb[2 * rows * D + o] + pb[3 * rows * D + o])) + bc;
            base[o] = v;
            if (ff < nv) {
                s += (double)v;
                ss += (double)v * (double)v;
            }
        }
        f = Fr;
    }
    for (; f + GN_LANES < nv; f += 2 * GN_LANES) {          // two independent loads per trip
        const double v0 = (double)base[(int64_t)f * D], v1 = (double)base[(int64_t)(f + GN_LANES) * D];
        s += v0 + v1;
        ss += v0 * v0 + v1 * v1;
    }
    if (f < nv) {
        const double v = (double)base[(int64_t)f * D];
        s += v;
        ss += v * v;
    }
    s = wave_sum_d(s);
    ss = wave_sum_d(ss);
    __shared__ double red[2 * GN_LANES];
    if ((threadIdx.x & 63) == 0) {
        red[fl] = s;
        red[GN_LANES + fl] = ss;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = 64.0 * nv;
        double S = 0.0, SS = 0.0;
        for (int i = 0; i < GN_LANES; ++i) {
            S += red[i];
            SS += red[GN_LANES + i];
        }
        const double mean = S / n;
        double var = SS / n - mean * mean;
        if (var < 0) var = 0;
        stats[(b * 4 + g) * 2 + 0] = (float)mean;
        stats[(b * 4 + g) * 2 + 1] = (float)(1.0 / sqrt(var + 1e-5));
    }
}

__global__ void __launch_bounds__(256) groupnorm_lrelu_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int64_t rows, int Fr,
                                                              float* __restrict__ out, int split,
                                                              const int* __restrict__ n_frames = nullptr) {
    // ragged batch: frames past a row's own count are written as 0 - the second prenet convolution pads with zeros there
    // split != 0: the output is the A operand of a split-bf16 GEMM and is written as bf16 hi/lo groups (8 channels = two
    // neighbouring threads; rows * 64 threads, so a pair never straddles a wave)
    const int64_t total = rows * (D / 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / (D / 4);
        const int c4 = (int)(i % (D / 4)) * 4;
        const int b = (int)(m / Fr), g = c4 >> 6;
        const float mean = stats[(b * 4 + g) * 2], rstd = stats[(b * 4 + g) * 2 + 1];
        const f32x4 v = *(const f32x4*)(x + m * D + c4);
        const f32x4 ga = *(const f32x4*)(gamma + c4), be = *(const f32x4*)(beta + c4);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = fmaf((v[j] - mean) * rstd, ga[j], be[j]);
            o[j] = y > 0.f ? y : 0.01f * y;
        }
        if (n_frames && (int)(m % Fr) >= ddsp_row_frames(n_frames, b, Fr)) o = f32x4{0.f, 0.f, 0.f, 0.f};
        if (split)
            *(ddsp_u32x4*)(out + m * D + c4) = ddsp_split4_pair(o, (i & 1) != 0, 1);
        else
            *(f32x4*)(out + m * D + c4) = o;
    }
}

// ---- side embeddings: x += Lin(ln(1+f0/700)) + Lin(phase/pi) + Lin(volume) + speaker ---------------
// The additions are the epilogue of the second prenet convolution (no launch and no pass over x of their own).
struct EpiEmbed {
    float* out;                 // (rows, 256)
    const float* bias;          // conv2 bias
    const float *f0, *phase, *vol;
    ddsp_u2c_weights w;
    const int64_t* spk_id;
    int64_t n_spk_id;
    MixArgs mix;
    int Fr;
    int* err;
    int64_t zstride;            // K-split launches: batch z stores its partial product at out + z * zstride, z = 0 adds bias + embeddings
    __device__ __forceinline__ float col(int n) const { return bias[n]; }
    __device__ __forceinline__ float embed(int m, int n, float v) const {
        const float lf0 = logf(1.0f + __fdiv_rn(f0[m], 700.0f));
        const float ph = __fdiv_rn(phase[m], 3.14159274101257324f);
        v += fmaf(lf0, w.f0_w[n], w.f0_b[n]);
        v += fmaf(ph, w.phase_w[n], w.phase_b[n]);
        v += fmaf(vol[m], w.volume_w[n], w.volume_b[n]);
        if (mix.ids_dev) {   // the row's own mix from the device tables (weights per row or per frame), terms in slot order
            const int* ri = mix.ids_dev + (int64_t)(m / Fr) * mix.n;
            const float* rw = mix.w_dev + (int64_t)(mix.per_frame ? m : m / Fr) * mix.n;   // weights of the frame, or of the row
            for (int k = 0; k < mix.n; ++k) {
                const int id = ri[k];
                if (id >= 1 && id <= w.n_spk)
                    v += rw[k] * w.spk_table[(id - 1) * D + n];
                else
                    __hip_atomic_store(err, DDSP_DEV_ERR_SPK_ID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        } else if (mix.n > 0) {
            for (int k = 0; k < mix.n; ++k) v += mix.w[k] * w.spk_table[(mix.ids[k] - 1) * D + n];
        } else {
            const int64_t id = spk_id[n_spk_id == 1 ? 0 : m / Fr];
            if (id >= 1 && id <= w.n_spk)
                v += w.spk_table[(id - 1) * D + n];
            else
                __hip_atomic_store(err, DDSP_DEV_ERR_SPK_ID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return v;
    }
    __device__ __forceinline__ void operator()(int z, int m, int n, float v, float cb) const {
        out[z * zstride + (int64_t)m * D + n] = z == 0 ? embed(m, n, v + cb) : v;
    }
    static constexpr bool kStore4 = true;
    __device__ __forceinline__ bool vec_ok() const { return ((uintptr_t)out % 16) == 0 && zstride % 4 == 0; }
    __device__ __forceinline__ void store4(int z, int m, int n, f32x4 v) const {
        if (z != 0) {
            *(f32x4*)(out + z * zstride + (int64_t)m * D + n) = v;
            return;
        }
        *(f32x4*)(out + (int64_t)m * D + n) = embed4(m, n, v);
    }
    // bias + the side embeddings of row m for columns n .. n + 3 (the operation order of store4 above, which calls it)
    __device__ __forceinline__ f32x4 embed4(int m, int n, f32x4 v) const {
        typedef gemm::f32x4_u v4;
        v += *(const v4*)(bias + n);
        const float lf0 = logf(1.0f + __fdiv_rn(f0[m], 700.0f));
        const float ph = __fdiv_rn(phase[m], 3.14159274101257324f);
        const float vl = vol[m];
        const v4 fw = *(const v4*)(w.f0_w + n), fb = *(const v4*)(w.f0_b + n);
        const v4 pw = *(const v4*)(w.phase_w + n), pb = *(const v4*)(w.phase_b + n);
        const v4 vw = *(const v4*)(w.volume_w + n), vb = *(const v4*)(w.volume_b + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] += fmaf(lf0, fw[j], fb[j]);
            v[j] += fmaf(ph, pw[j], pb[j]);
            v[j] += fmaf(vl, vw[j], vb[j]);
        }
        if (mix.ids_dev) {
            const int* ri = mix.ids_dev + (int64_t)(m / Fr) * mix.n;
            const float* rw = mix.w_dev + (int64_t)(mix.per_frame ? m : m / Fr) * mix.n;   // weights of the frame, or of the row
            for (int k = 0; k < mix.n; ++k) {
                const int id = ri[k];
                if (id >= 1 && id <= w.n_spk) {
                    const v4 e = *(const v4*)(w.spk_table + (id - 1) * D + n);
                    const float wk = rw[k];
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] += wk * e[j];
                } else {
                    __hip_atomic_store(err, DDSP_DEV_ERR_SPK_ID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        } else if (mix.n > 0) {
            for (int k = 0; k < mix.n; ++k) {
                const v4 e = *(const v4*)(w.spk_table + (mix.ids[k] - 1) * D + n);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] += mix.w[k] * e[j];
            }
        } else {
            const int64_t id = spk_id[n_spk_id == 1 ? 0 : m / Fr];
            if (id >= 1 && id <= w.n_spk) {
                const v4 e = *(const v4*)(w.spk_table + (id - 1) * D + n);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] += e[j];
            } else {
                __hip_atomic_store(err, DDSP_DEV_ERR_SPK_ID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        return v;
    }
};

// the same additions as the `Pre` of gemm::kernel_res_ln: second prenet convolution + embeddings + the first LayerNorm in one kernel
struct PreEmbed {
    EpiEmbed e;
    struct State {};
    template <int RB>
    __device__ __forceinline__ void load(State&, const gemm::LnArgs&, int, int, int, int, int) const {}
    __device__ __forceinline__ f32x4 apply(const State&, const gemm::LnArgs&, int, int, int m, int c0, f32x4 acc) const {
        return e.embed4(m, c0, acc);
    }
};

// ---- LayerNorm over 256 channels, one wave per row (4 channels per lane) ----------------------------
// Small batches (K-split GEMMs, see u2c_forward): the row to normalise is first completed here,
//   x_out[m] = x[m] + bias + sum_s part[s][m]   (the residual GEMM's epilogue, deferred: its K range was cut into KS_SPLITS
// workgroups per tile that each stored a partial product), written back for the next residual and then normalised.
struct LnPending {
    const float* part;   // [KS_SPLITS][rows][D] or null
    const float* bias;   // or null
    float* x_out;
    int has_res;         // the kernel's x argument is the residual to add (else the row is the partial sum alone)
};
constexpr int KS_SPLITS = 4;
constexpr int KS_MAX_ROWS = 256;   // up to 4 row tiles x 4 column tiles x 4 splits = 64 workgroups (344 rows measured slower than whole-K launches)
// rows from which the inference forward writes its activations pre-split (with the fused-GLU 128x128 tiling)
constexpr int64_t U2C_PRESPLIT_MIN_ROWS = 8192;
// rows from which pw2 forms the depthwise convolution in its own operand stage (gemm_ln.h A_DWCONV).  Measured against the two
// launches at 11008 rows only; between 8192 rows and this the pair stays, as tests/test_gpu_models.py pins it there
constexpr int64_t U2C_DWCONV_FUSE_MIN_ROWS = 10240;
// (utterance, head) pairs from which the non-causal inference attention runs on the fused split-bf16 kernel
constexpr int64_t ATTN_BF16_MIN = 256;
__global__ void __launch_bounds__(256) layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int64_t rows,
                                                        float* __restrict__ out, int split, LnPending pend = LnPending{nullptr, nullptr, nullptr, 0}) {
    // split != 0: the row is written as bf16 hi/lo groups (A operand of a split-bf16 GEMM): lanes 2j, 2j+1 own one group
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;
    f32x4 v;
    if (pend.part) {
        const f32x4 p0 = *(const f32x4*)(pend.part + m * D + lane * 4), p1 = *(const f32x4*)(pend.part + (rows + m) * D + lane * 4);
        const f32x4 p2 = *(const f32x4*)(pend.part + (2 * rows + m) * D + lane * 4), p3 = *(const f32x4*)(pend.part + (3 * rows + m) * D + lane * 4);
        v = (p0 + p1) + (p2 + p3);
        if (pend.bias) v = v + *(const f32x4*)(pend.bias + lane * 4);
        if (pend.has_res) v = *(const f32x4*)(x + m * D + lane * 4) + v;
        *(f32x4*)(pend.x_out + m * D + lane * 4) = v;
    } else {
        v = *(const f32x4*)(x + m * D + lane * 4);
    }
    const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / D);
    f32x4 d;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        d[j] = v[j] - mean;
        ss = fmaf(d[j], d[j], ss);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) * (1.0f / D) + 1e-5f);
    const f32x4 ga = *(const f32x4*)(gamma + lane * 4), be = *(const f32x4*)(beta + lane * 4);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaf(d[j] * rstd, ga[j], be[j]);
    if (split)
        *(ddsp_u32x4*)(out + m * D + lane * 4) = ddsp_split4_pair(o, (lane & 1) != 0, 1);
    else
        *(f32x4*)(out + m * D + lane * 4) = o;
}

// ---- softmax-kernel feature map (ddsp/pcmer.py:123-159), in place on the projected rows ---------------
// feat rows (rows8 = B*Fr*8, LDF): raw = data . P^T ; data rows (rows8, 64).
// query: r*(exp(dn*raw - diag - max_j(dn*raw)) + 1e-4) ; key: r*exp(dn*raw - diag + 1e-4)
template <bool QUERY>
__global__ void __launch_bounds__(256) feature_map_kernel(float* __restrict__ feat, const float* __restrict__ data,
                                                          int64_t rows8) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows8) return;
    const float dn = 0.35355339059327373f;   // 64^-0.25
    const float ratio = 0.06131393394849658f;  // 266^-0.5
    const float x = data[r * DH + lane];
    const float diag = wave_sum(x * x) * 0.5f * (dn * dn);
    float* row = feat + r * LDF;
    float dd[5];
    float mx = -3.0e38f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int j = lane + 64 * i;
        dd[i] = (j < NF) ? dn * row[j] : -3.0e38f;
        mx = fmaxf(mx, dd[i]);
    }
    if (QUERY) mx = wave_max(mx);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int j = lane + 64 * i;
        if (j < NF) {
            float o;
            if (QUERY)
                o = ratio * (expf((dd[i] - diag) - mx) + 1e-4f);
            else
                o = ratio * expf((dd[i] - diag) + 1e-4f);
            row[j] = o;
        } else if (j < LDF) {
            row[j] = 0.f;
        }
    }
}

// ks[b,h,j] = sum_n k'[b,n,h,j]   block = (b*8+h): 72 threads x 16 bytes cover the 288 padded features of a row, 8 frame
// lanes walk the frames with two rows in flight each and meet in the LDS (one thread per feature walking all frames alone
// read at 1.2 TB/s: 41 us per call at the training shape)
__global__ void __launch_bounds__(KS_T * 8) key_sum_kernel(const float* __restrict__ kf, int Fr, float* __restrict__ ks) {
    const int bh = blockIdx.x, b = bh / H, h = bh % H;
    const int j4 = threadIdx.x % KS_T, fl = threadIdx.x / KS_T;
    const float* base = kf + (((int64_t)b * Fr) * H + h) * LDF + 4 * j4;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    int n = fl;
    for (; n + 8 < Fr; n += 16) {
        s0 += *(const f32x4*)(base + (int64_t)n * H * LDF);
        s1 += *(const f32x4*)(base + (int64_t)(n + 8) * H * LDF);
    }
    if (n < Fr) s0 += *(const f32x4*)(base + (int64_t)n * H * LDF);
    __shared__ f32x4 red[KS_T * 8];
    red[threadIdx.x] = s0 + s1;
    __syncthreads();
    if (fl == 0) {
        f32x4 t = red[j4];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += red[i * KS_T + j4];
        *(f32x4*)(ks + (int64_t)bh * LDF + 4 * j4) = t;
    }
}

// dinv[r] = 1 / (q'[r,:] . ks[b,h,:] + 1e-8)   one wave per (frame, head) row
__global__ void __launch_bounds__(256) attn_denominator_kernel(const float* __restrict__ qf, const float* __restrict__ ks,
                                                               int Fr, int64_t rows8, float* __restrict__ dinv) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows8) return;
    const int h = (int)(r % H);
    const int64_t b = (r / H) / Fr;
    const float* q = qf + r * LDF;
    const float* k = ks + (b * H + h) * LDF;
    float s = 0.f;
    for (int j = lane; j < NF; j += 64) s = fmaf(q[j], k[j], s);
    s = wave_sum(s);
    if (lane == 0) dinv[r] = 1.0f / (s + 1e-8f);
}

// ---- causal linear attention (ddsp/pcmer.py:170-188, `c: true`), inference ---------------------------------------------------
// out[n] = (q'_n . sum_{m<=n} k'_m (x) v_m) / (q'_n . (sum_{m<=n} k'_m + 1e-6)).  One workgroup per (utterance, head) walks
// the frames in order; thread t owns channel e = t & 63 of rows j = (t >> 6) + 4 i of the running 266 x 64 state (67 registers).
// `fast_transformers.CausalDotProduct` (the numerator) is a third-party CUDA extension that is not in the image: it is
// restated from its definition; the normaliser is the reference's own code.  Correct-first: one frame per step, two barriers.
__global__ void __launch_bounds__(256) causal_attention_kernel(const float* __restrict__ qf, const float* __restrict__ kf,
                                                               const float* __restrict__ v, int Fr, float* __restrict__ out) {
    constexpr int ROWS = (NF + 3) / 4;       // 67
    __shared__ float sq[LDF], sk[LDF], sv[DH], part[4 * DH], dpart[4];
    const int bh = blockIdx.x, b = bh / H, h = bh % H;
    const int t = threadIdx.x, e = t & 63, r0 = t >> 6;
    float S[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) S[i] = 0.f;
    float ksum[2] = {0.f, 0.f};              // running key sums of features t and t + 256
    for (int n = 0; n < Fr; ++n) {
        const int64_t row8 = ((int64_t)b * Fr + n) * H + h;
        for (int j = t; j < LDF; j += 256) {
            sq[j] = qf[row8 * LDF + j];
            sk[j] = kf[row8 * LDF + j];
        }
        if (t < DH) sv[t] = v[((int64_t)b * Fr + n) * INNER + h * DH + t];
        __syncthreads();
        const float ve = sv[e];
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int j = r0 + 4 * i;
            if (j < NF) {
                S[i] = fmaf(sk[j], ve, S[i]);
                acc = fmaf(sq[j], S[i], acc);
            }
        }
        part[r0 * DH + e] = acc;
        // denominator: q' . (cumulative k' + eps), features t and t + 256
        float d = 0.f;
        if (t < NF) {
            ksum[0] += sk[t];
            d = sq[t] * (ksum[0] + 1e-6f);
        }
        if (t + 256 < NF) {
            ksum[1] += sk[t + 256];
            d = fmaf(sq[t + 256], ksum[1] + 1e-6f, d);
        }
        d = wave_sum(d);
        if ((t & 63) == 0) dpart[t >> 6] = d;
        __syncthreads();
        if (t < DH) {
            const float num = (part[t] + part[DH + t]) + (part[2 * DH + t] + part[3 * DH + t]);
            const float den = (dpart[0] + dpart[1]) + (dpart[2] + dpart[3]);
            out[((int64_t)b * Fr + n) * INNER + h * DH + t] = num * (1.0f / den);
        }
    }
}

// ---- conformer conv module pieces --------------------------------------------------------------------
__global__ void __launch_bounds__(256) glu_kernel(const float* __restrict__ g1, int64_t rows, float* __restrict__ out) {
    const int64_t total = rows * (INNER / 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / (INNER / 4);
        const int c4 = (int)(i % (INNER / 4)) * 4;
        const f32x4 a = *(const f32x4*)(g1 + m * 2 * INNER + c4);
        const f32x4 g = *(const f32x4*)(g1 + m * 2 * INNER + INNER + c4);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = a[j] * (1.0f / (1.0f + expf(-g[j])));
        *(f32x4*)(out + m * INNER + c4) = o;
    }
}

// The same convolution + SiLU for the inference forward at large batches, two ADJACENT channels per thread (round 3).
// The one-channel kernel above is bound by vector-instruction issue, not by memory (r02_e_pmc_sq_synth.txt: 2300 instructions
// per wave for 32 outputs of 64 channels, VALU 0.62 at ~4 cycles per instruction, 24.5 us for 45 MB): 31 multiply-adds per
// output are its floor.  With a channel PAIR per thread the pair is the packed operand - taps, window and accumulator of the two
// channels sit in adjacent registers as they come from memory (8-byte loads), so every `v_pk_fma_f32` does two outputs and no
// register re-alignment is needed (the packed form ACROSS frames of round 2 needed moves for every other window position).
// Sigmoid by v_exp_f32 / v_rcp_f32 (~2 ulp).  Split output: the four lanes of a channel octet exchange their bf16 pairs so
// that each stores 8 contiguous bytes of the (8 hi | 8 lo) group.
typedef float f32x2_dw __attribute__((ext_vector_type(2)));
template <int RUN>
__global__ void __launch_bounds__(256, 3) dwconv_pair_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, int B, int Fr,
                                                          float* __restrict__ out, int left, int split,
                                                          const int* __restrict__ n_frames = nullptr) {
    const int cp = blockIdx.x * 256 + threadIdx.x;      // channel pair (INNER / 2 = 256 pairs: one block in x)
    const int c = 2 * cp;
    const int runs = (Fr + RUN - 1) / RUN;
    const int b = blockIdx.y / runs, f0 = (blockIdx.y % runs) * RUN;
    f32x2_dw wt[DWK];
#pragma unroll
    for (int t = 0; t < DWK; ++t) wt[t] = *(const f32x2_dw*)(w + t * INNER + c);      // [tap][channel] copy
    const float* xb = x + ((int64_t)b * Fr) * INNER + c;
    const int n_in = ddsp_row_frames(n_frames, b, Fr);   // ragged batch: input frames >= n_b read as 0
    f32x2_dw win[RUN + DWK - 1];
#pragma unroll
    for (int i = 0; i < RUN + DWK - 1; ++i) {
        const int f = f0 + i - left;
        win[i] = (f >= 0 && f < n_in) ? *(const f32x2_dw*)(xb + (int64_t)f * INNER) : f32x2_dw{0.f, 0.f};
    }
    const f32x2_dw bi = *(const f32x2_dw*)(bias + c);
    const int q = threadIdx.x & 3;                       // position in the channel octet
#pragma unroll
    for (int o = 0; o < RUN; ++o) {
        f32x2_dw acc = bi;
#pragma unroll
        for (int t = 0; t < DWK; ++t) acc = __builtin_elementwise_fma(wt[t], win[o + t], acc);
        f32x2_dw y;
#pragma unroll
        for (int e = 0; e < 2; ++e)
            y[e] = acc[e] * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * acc[e]));
        const bool ok = f0 + o < Fr;
        float* dst = out + ((int64_t)b * Fr + f0 + o) * INNER + c;
        if (split) {
            // octet = lanes 4g..4g+3 (channels 8g..8g+7): lane q holds bf16 pairs h_q, l_q; the group is [h0 h1 h2 h3 | l0 l1 l2 l3]
            typedef __bf16 bf16x2_dw __attribute__((ext_vector_type(2)));
            const uint32_t h = __builtin_bit_cast(uint32_t, __builtin_convertvector(y, bf16x2_dw));
            const f32x2_dw rem = y - f32x2_dw{__builtin_bit_cast(float, h << 16), __builtin_bit_cast(float, h & 0xffff0000u)};
            const uint32_t l = __builtin_bit_cast(uint32_t, __builtin_convertvector(rem, bf16x2_dw));
            // lane 0 stores (h0, h1), lane 1 (h2, h3), lane 2 (l0, l1), lane 3 (l2, l3)
            const int lane = threadIdx.x & 63, base = lane & ~3;
            const int s0 = base + 2 * (q & 1), s1 = s0 + 1;
            const uint32_t h0 = (uint32_t)__shfl((int)h, s0, 64), h1 = (uint32_t)__shfl((int)h, s1, 64);
            const uint32_t l0 = (uint32_t)__shfl((int)l, s0, 64), l1 = (uint32_t)__shfl((int)l, s1, 64);
            if (ok) {
                uint32_t* g = (uint32_t*)(out + ((int64_t)b * Fr + f0 + o) * INNER + (c & ~7)) + 2 * q;
                g[0] = q < 2 ? h0 : l0;
                g[1] = q < 2 ? h1 : l1;
            }
        } else if (ok) {
            *(f32x2_dw*)dst = y;
        }
    }
}

// The pair kernel above holds 46 frames of window and 31 taps per thread (168 registers: three waves per SIMD) and every wave runs
// load -> products -> store in lockstep with its round: 0.45 of its cycles wait.  LDS-tiled form (round 3): a workgroup stages
// 64 + 30 frames x 64 channels ONCE with 16-byte loads (1.47x read amplification instead of 2.9x, six loads per thread instead
// of 46) beside the 31 x 64 tap table, a thread makes 8 frames x 2 channels from a register window filled by 8-byte LDS reads;
// 158 registers (three waves per SIMD, as before - at four the compiler spills 40), 32 KB of LDS; the workgroups of a CU are in
// different phases.  Row-kernel family 0.081 -> 0.070 ms per step (21.5 -> 17.8 us per launch).
constexpr int DWT_F = 64, DWT_C = 64, DWT_RUN = 8;
__global__ void __launch_bounds__(256, 3) dwconv_tile_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, int B, int Fr,
                                                             float* __restrict__ out, int left, int split,
                                                             const int* __restrict__ n_frames = nullptr) {
    constexpr int ROWS = DWT_F + DWK - 1;
    __shared__ float tile[ROWS * DWT_C];
    __shared__ float taps[DWK * DWT_C];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * DWT_C;
    const int ftiles = (Fr + DWT_F - 1) / DWT_F;
    const int b = blockIdx.y / ftiles, f0 = (blockIdx.y % ftiles) * DWT_F;
    const float* xb = x + ((int64_t)b * Fr) * INNER + c0;
    const int n_in = ddsp_row_frames(n_frames, b, Fr);   // ragged batch: input frames >= n_b read as 0
#pragma unroll
    for (int k = 0; k < (ROWS * (DWT_C / 4) + 255) / 256; ++k) {
        const int i = tid + 256 * k;
        if (i < ROWS * (DWT_C / 4)) {
            const int row = i / (DWT_C / 4), c4 = i % (DWT_C / 4);
            const int f = f0 + row - left;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (f >= 0 && f < n_in) v = *(const f32x4*)(xb + (int64_t)f * INNER + 4 * c4);
            *(f32x4*)(tile + row * DWT_C + 4 * c4) = v;
        }
    }
    for (int i = tid; i < DWK * (DWT_C / 4); i += 256) {
        const int t = i / (DWT_C / 4), c4 = i % (DWT_C / 4);
        *(f32x4*)(taps + t * DWT_C + 4 * c4) = *(const f32x4*)(w + t * INNER + c0 + 4 * c4);      // [tap][channel] copy
    }
    __syncthreads();
    const int cp = tid & 31, fg = tid >> 5;               // channel pair of the tile, group of 8 frames
    const int c = c0 + 2 * cp, fo = DWT_RUN * fg;
    f32x2_dw win[DWT_RUN + DWK - 1];
#pragma unroll
    for (int i = 0; i < DWT_RUN + DWK - 1; ++i) win[i] = *(const f32x2_dw*)(tile + (fo + i) * DWT_C + 2 * cp);
    const f32x2_dw bi = *(const f32x2_dw*)(bias + c);
    f32x2_dw acc[DWT_RUN];
#pragma unroll
    for (int o = 0; o < DWT_RUN; ++o) acc[o] = bi;
#pragma unroll
    for (int t = 0; t < DWK; ++t) {
        const f32x2_dw wt = *(const f32x2_dw*)(taps + t * DWT_C + 2 * cp);
#pragma unroll
        for (int o = 0; o < DWT_RUN; ++o) acc[o] = __builtin_elementwise_fma(wt, win[o + t], acc[o]);
    }
    const int q = tid & 3;                                // position in the channel octet
#pragma unroll
    for (int o = 0; o < DWT_RUN; ++o) {
        f32x2_dw y;
#pragma unroll
        for (int e = 0; e < 2; ++e)
            y[e] = acc[o][e] * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * acc[o][e]));
        const int f = f0 + fo + o;
        const bool ok = f < Fr;
        if (split) {
            typedef __bf16 bf16x2_dw __attribute__((ext_vector_type(2)));
            const uint32_t h = __builtin_bit_cast(uint32_t, __builtin_convertvector(y, bf16x2_dw));
            const f32x2_dw rem = y - f32x2_dw{__builtin_bit_cast(float, h << 16), __builtin_bit_cast(float, h & 0xffff0000u)};
            const uint32_t l = __builtin_bit_cast(uint32_t, __builtin_convertvector(rem, bf16x2_dw));
            const int lane = tid & 63, base = lane & ~3;
            const int s0 = base + 2 * (q & 1), s1 = s0 + 1;
            const uint32_t h0 = (uint32_t)__shfl((int)h, s0, 64), h1 = (uint32_t)__shfl((int)h, s1, 64);
            const uint32_t l0 = (uint32_t)__shfl((int)l, s0, 64), l1 = (uint32_t)__shfl((int)l, s1, 64);
            if (ok) {
                uint32_t* g = (uint32_t*)(out + ((int64_t)b * Fr + f) * INNER + (c & ~7)) + 2 * q;
                g[0] = q < 2 ? h0 : l0;
                g[1] = q < 2 ? h1 : l1;
            }
        } else if (ok) {
            *(f32x2_dw*)(out + ((int64_t)b * Fr + f) * INNER + c) = y;
        }
    }
}

// the prepared weights (u2c_prepare_kernel, performer_p3): from the arena, or (cached != null) from the context's slot
static void plan_weights(Arena& a, U2CBufs& bf, const ddsp_u2c_weights& w) {
    bf.w1 = a.get((size_t)D * 3 * w.n_unit);
    bf.w2 = a.get((size_t)D * 3 * D);
    bf.wh = a.get((size_t)w.n_out * D);
    bf.wqkv = a.get((size_t)3 * 3 * INNER * D);
    bf.bqkv = a.get((size_t)3 * 3 * INNER);
    bf.wglu = a.get((size_t)3 * 2 * INNER * D);    // pw1 re-ordered for the fused GLU epilogue (inference)
    bf.bglu = a.get((size_t)3 * 2 * INNER);
    bf.wdw = a.get((size_t)3 * DWK * INNER);         // depthwise taps as [tap][channel]
    bf.wout = a.get((size_t)3 * D * INNER);          // out-projection / pw2 weights as bf16 hi/lo groups (split GEMMs)
    bf.wpw2 = a.get((size_t)3 * D * INNER);
    bf.p3 = a.get((size_t)3 * PERFORMER_P3_BYTES / 4);  // projection matrices as bf16 pieces (split-bf16 attention)
}

}  // namespace

namespace u2c {

void plan_forward(Arena& a, U2CBufs& bf, const ddsp_u2c_weights& w, int64_t B, int64_t Fr, bool keep, bool weights_cached) {
    const size_t M = (size_t)(B * Fr), M8 = M * H;
    if (!weights_cached) plan_weights(a, bf, w);
    bf.t1 = a.get(M * D);
    bf.t2 = a.get(M * D);
    bf.gst = a.get((size_t)B * 4 * 2);
    bf.y_final = a.get(M * D);
    bf.kpart = a.get((size_t)KS_SPLITS * (M <= KS_MAX_ROWS ? M : 1) * D);   // K-split partial products (small batches only)
    auto one = [&](LayerBufs& L, float* x_in) {
        L.x_in = x_in;
        L.y = a.get(M * D);
        L.q = a.get(M * INNER);
        L.k = a.get(M * INNER);
        L.v = a.get(M * INNER);
        L.qf = a.get(M8 * LDF);
        L.kf = a.get(M8 * LDF);
        L.ks = a.get((size_t)B * H * PERFORMER_KS_STRIDE);           // (the fused inference kernels pad features to 272)
        L.cx = a.get((size_t)B * H * (PERFORMER_CTXS_FLOATS > PERFORMER_LDJ * DH ? PERFORMER_CTXS_FLOATS : PERFORMER_LDJ * DH));
        L.dinv = a.get(M8);
        L.attn = a.get(M * INNER);
        L.g1 = a.get(M * 2 * INNER);
        if (keep) {
            L.x_mid = a.get(M * D);
            L.y2 = a.get(M * D);
            L.glu = a.get(M * INNER);
            L.pre = a.get(M * INNER);
            L.dwo = a.get(M * INNER);
            L.x_out = a.get(M * D);
        } else {
            L.x_mid = L.x_in;  // residuals in place
            L.x_out = L.x_in;
            L.y2 = L.y;
            L.glu = L.q;       // q / k are dead once the attention output exists
            L.dwo = L.k;
            L.pre = nullptr;
        }
    };
    float* x0 = a.get(M * D);
    one(bf.l[0], x0);
    if (keep) {
        one(bf.l[1], bf.l[0].x_out);
        one(bf.l[2], bf.l[1].x_out);
    } else {
        bf.l[1] = bf.l[0];
        bf.l[2] = bf.l[0];
    }
}

int u2c_forward(ddsp_ctx* ctx, hipStream_t st, const ddsp_u2c_weights& w, const U2CInputs& in, U2CBufs& bf, float* ctrl) {
    const int64_t B = in.B, Fr = in.Fr, M = B * Fr, M8 = M * H;
    const int iM = (int)M;
    const size_t n_w1 = (size_t)D * 3 * w.n_unit, n_w2 = (size_t)D * 3 * D, n_wh = (size_t)w.n_out * D;
    // product arithmetic of the Linear / conv GEMMs (gemm::Args::math): inference uses the split-bf16 mode, the
    // training forward (activations kept for the backward pass) stays on fp32 MFMA like the backward GEMMs
    // (ctx->math 4 = split-bf16 products with every operand split inside the GEMM loops: the pre-round-2 path, kept for
    // test_presplit_operands_give_the_same_bits)
    const int lin_math = bf.l[0].pre ? 0 : (ctx->math == 4 ? DDSP_MATH_SPLIT_BF16 : ctx->math);
    const float* zero_page = nullptr;   // source of the conv taps that fall off an utterance (LDS-DMA conv GEMM)
    if (int rc = ddsp_zero_page(ctx, &zero_page)) return rc;
    int* dev_err = nullptr;
    if (int rc = ddsp_dev_error_ptr(ctx, &dev_err)) return rc;
    // Inference: GLU is formed inside the pw1 GEMM (half the store, no glu kernel) - on the 128x128 DMA tile when there are
    // enough rows for it (glu_large), else on 64x128 tiles of 4 waves (round 3: one launch and one round trip of the
    // 2 x 512-wide pw1 output fewer per layer).  Training keeps pw1's raw output for the backward pass and the separate
    // glu kernel.
    const bool glu_large = !bf.l[0].pre && (int64_t)((M + 127) / 128) * (2 * INNER / 128) >= 512;
    bool fuse_glu = !bf.l[0].pre;
    for (int l = 0; l < 3; ++l)
        fuse_glu = fuse_glu && ((uintptr_t)w.layer[l].cm_pw1_w % 16) == 0;
    // Split-bf16 products at a size where every GEMM of the network runs the LDS-DMA kernel: nothing is split inside the
    // GEMM loops.  The weights are packed as bf16 hi/lo groups by the preparation launch (B_split) and the producers of
    // the A operands (GroupNorm+LeakyReLU, the LayerNorms, the attention kernel) write them in that layout (A_split);
    // conv1 reads the caller's fp32 units: it alone still splits A in the kernel.
    // (presplit_w: the weights alone, at any batch size - every GEMM of the inference forward runs the DMA kernel now, which
    // then splits only its A operand in the loop (mode 7); presplit: the activations too, from the size at which the fused-GLU
    // tiling is used)
    const bool presplit_w = lin_math == DDSP_MATH_SPLIT_BF16 && ctx->math != 4 && w.n_unit % 32 == 0 &&
                            w.n_unit + 32 <= DDSP_ZERO_FLOATS && w.n_out >= 256 && ((uintptr_t)in.units % 16) == 0;
    const bool presplit = presplit_w && fuse_glu && glu_large && M >= U2C_PRESPLIT_MIN_ROWS;
    const bool attn_bf16 = !bf.l[0].pre && lin_math == DDSP_MATH_SPLIT_BF16 && B * H >= ATTN_BF16_MIN && !w.causal;
    const int asplit = presplit ? 1 : 0;
    // A handful of rows (the real-time block: 87): the N = 256, K = 512 residual GEMMs (out-projection, pw2) would run on 8
    // workgroups walking 16 k-steps each.  Their K range is cut over KS_SPLITS workgroups per tile instead (32-96 workgroups,
    // 4 k-steps each, partial products stored) and the sum + bias + residual is formed by the LayerNorm that follows.
    const bool ksplit = !bf.l[0].pre && M <= KS_MAX_ROWS;
    LnPending pending{nullptr, nullptr, nullptr, 0};
    auto residual_gemm = [&](gemm::Args g, const float* x_res, float* x_dst, const float* bias) {
        // x_dst = x_res + A B^T + bias, now or (ksplit) when the next LayerNorm reads it
        if (ksplit && gemm::dma_ok(g) && g.K % (32 * KS_SPLITS) == 0) {
            const int kc = g.K / KS_SPLITS;
            g.K = kc;
            g.sA_hi = kc;
            g.sB_hi = kc;
            gemm::EpiStore e{bf.kpart, D, nullptr, 1, M * D, 0};
            gemm::dma_go<64, 64, gemm::EpiStore, 4, 4>(st, g, KS_SPLITS, e);
            pending = LnPending{bf.kpart, bias, x_dst, 1};
            return x_res;   // the LayerNorm reads the residual from here
        }
        gemm::EpiResidual e{x_dst, x_res, D, bias};
        gemm::launch<true, true, gemm::A_PLAIN>(st, g, 1, e);
        return (const float*)x_dst;
    };
    // Large batches with pre-split operands: the residual layer AND the LayerNorm that follows it in one kernel (gemm_ln.h: a
    // workgroup owns 64 rows x all 256 columns; same bits as the two launches).
    // DDSP_GEMM_LN=0 restores the pair (test_residual_layernorm_in_the_model_is_bit_identical)
    static int gemm_ln_on = -1;
    if (gemm_ln_on < 0) {
        const char* e = getenv("DDSP_GEMM_LN");
        gemm_ln_on = (e && e[0] == '0') ? 0 : 1;
    }
    static int64_t gemm_ln_min = -1;   // DDSP_GEMM_LN_MIN: rows from which the fused kernel runs (the same test lowers it)
    if (gemm_ln_min < 0) {
        const char* e = getenv("DDSP_GEMM_LN_MIN");
        // (measured: B = 8 / 1376 rows 0.476 -> 0.519 ms, B = 24 / 4128 rows 0.826 -> 0.839 ms per forward WITH the fused kernel -
        // a few workgroups each pull 640 KB of operands through one CU's load path; B = 64 / 11008 rows 1.138 -> 1.126)
        gemm_ln_min = e ? atoll(e) : 8192;
    }
    bool ln_done = false;   // the next LayerNorm's output has been written by the producer of its input
    auto ln_args = [&](const gemm::Args& g, const float* x_res, float* x_dst, const float* bias, const float* gamma,
                       const float* beta, float* y_out) {
        return gemm::LnArgs{g.A, g.B_split, g.lda, g.ldb, g.M, g.K, bias, x_res, x_dst, gamma, beta, y_out, asplit};
    };
    // (the A operand pre-split at large batches, fp32 below; small batches keep the separate LayerNorm, which sums their K-split partials)
    auto ln_fusable = [&](const gemm::Args& g, const gemm::LnArgs& a) {
        return gemm_ln_on && !ksplit && !bf.l[0].pre && g.math == DDSP_MATH_SPLIT_BF16 && g.B_split && (g.A_split || !asplit) &&
               g.N == D && M >= gemm_ln_min && gemm::res_ln_ok(a);
    };
    const int want_state = 1 | (presplit_w ? 2 : 0) | (fuse_glu ? 4 : 0);
    const bool prepared = bf.wstate && (*bf.wstate & 7) == want_state;
    const bool p3_ready = prepared && (*bf.wstate & 8);
    if (!prepared) {   // weight preparation, one launch (u2c_prepare_kernel)
        PrepArgs pa;
        pa.w = w;
        pa.w1 = bf.w1;
        pa.w2 = bf.w2;
        pa.wh = bf.wh;
        pa.wqkv = bf.wqkv;
        pa.bqkv = bf.bqkv;
        pa.wglu = bf.wglu;
        pa.bglu = bf.bglu;
        pa.wout = bf.wout;
        pa.wpw2 = bf.wpw2;
        pa.split = presplit_w ? 1 : 0;
        pa.qkv_blocks = 192;
        pa.glu_blocks = 128;
        pa.copy_blocks = 32;
        pa.end[0] = (int)grid_for((int64_t)n_w1 / 4, 256, 256);
        pa.end[1] = pa.end[0] + (int)grid_for((int64_t)n_w2 / 8, 256, 256);
        pa.end[2] = pa.end[1] + (w.n_out + 3) / 4;
        pa.end[3] = pa.end[2] + 3 * pa.qkv_blocks;
        pa.end[4] = pa.end[3] + (fuse_glu ? 3 * pa.glu_blocks : 0);
        pa.end[5] = pa.end[4] + (presplit_w ? 6 * pa.copy_blocks : 0);
        pa.end[6] = pa.end[5] + 48;
        pa.wdw = bf.wdw;
        PROF(PF_U2C_PREP, 0, 8.0 * (n_w1 + n_w2 + n_wh + 3.0 * 3 * INNER * D + (fuse_glu ? 3.0 * 2 * INNER * D : 0.0) +
                                    (presplit_w ? 6.0 * D * INNER : 0.0)),
             hipLaunchKernelGGL(u2c_prepare_kernel, dim3((unsigned)pa.end[6]), dim3(256), 0, st, pa));
        if (bf.wstate) *bf.wstate = want_state;
    }
    if (attn_bf16 && !p3_ready) {   // the three projection matrices as bf16 pieces for the split attention kernels, one launch
        PROF(PF_U2C_PREP, 0, 3.0 * (4.0 * NF * DH + PERFORMER_P3_BYTES),
             performer_p3(st, w.layer[0].proj, w.layer[1].proj, w.layer[2].proj, bf.p3));
        if (bf.wstate) *bf.wstate |= 8;
    }
    // with B_split the GEMM reads ONLY the split copy: both pointers name the same packed matrix
    auto set_b = [&](gemm::Args& g, const float* packed, int a_is_split) {
        g.math = lin_math;
        if (presplit_w) {
            g.B = packed;
            g.B_split = packed;
            g.A_split = a_is_split;
        }
    };
    // DDSP_DW_PAIR=1: the register pair kernel instead of the LDS-tiled one (test_tiled_depthwise_convolution_matches_the_register_kernel)
    static const bool dw_tiled = [] { const char* e = getenv("DDSP_DW_PAIR"); return !(e && e[0] == '1'); }();
    bool conv_split = false;
    // ---- prenet: conv k3 -> GroupNorm(4) -> LeakyReLU -> conv k3 ----
    {
        gemm::Args g = gemm::make(in.units, w.n_unit, bf.w1, 3 * w.n_unit, iM, D, 3 * w.n_unit);
        set_b(g, bf.w1, 0);
        g.tap_shift = w.causal ? -1 : 0;
        g.Fr = (int)Fr;
        g.Cin = w.n_unit;
        g.zeros = zero_page;
        // (small batches: the k = 3 Cin range of the two prenet convolutions is cut over KS_SPLITS workgroups per tile as
        // well; conv1's partial products are summed by the GroupNorm statistics pass, conv2's by the first LayerNorm)
        conv_split = ksplit && gemm::dma_ok(g) && g.K % (32 * KS_SPLITS) == 0 && w.n_unit % 32 == 0 && (3 * D) % (32 * KS_SPLITS) == 0 &&
                     w.n_unit + 32 <= DDSP_ZERO_FLOATS;
        if (conv_split) {
            g.K /= KS_SPLITS;
            g.kz = g.K;
            gemm::EpiStore e{bf.kpart, D, nullptr, 1, M * D, 0};
            PROF(PF_U2C_GEMM_CONV3, 2.0 * M * D * 3 * w.n_unit, 4.0 * M * (w.n_unit + D),
                 (gemm::dma_go<64, 64, gemm::EpiStore, 4, 4, gemm::A_CONV3>(st, g, KS_SPLITS, e)));
        } else {
            gemm::EpiStore e{bf.t1, D, w.prenet_conv1_b, 1, 0, 0};
            PROF(PF_U2C_GEMM_CONV3, 2.0 * M * D * 3 * w.n_unit, 4.0 * M * (w.n_unit + D),
                 (gemm::launch<true, true, gemm::A_CONV3>(st, g, 1, e)));
        }
    }
    PROF(PF_U2C_ROWWISE, 0, 4.0 * M * D,
         hipLaunchKernelGGL(groupnorm_stats_kernel, dim3(4, (unsigned)B), dim3(64 * GN_LANES), 0, st, bf.t1, (int)Fr, bf.gst,
                            conv_split ? bf.kpart : nullptr, w.prenet_conv1_b, M, in.n_frames));
    PROF(PF_U2C_ROWWISE, 0, 8.0 * M * D,
         hipLaunchKernelGGL(groupnorm_lrelu_kernel, dim3(grid_for(M * (D / 4))), dim3(256), 0, st, bf.t1, bf.gst,
                            w.prenet_gn_w, w.prenet_gn_b, M, (int)Fr, bf.t2, asplit, in.n_frames));
    float* x = bf.l[0].x_in;
    {
        gemm::Args g = gemm::make(bf.t2, D, bf.w2, 3 * D, iM, D, 3 * D);
        set_b(g, bf.w2, asplit);
        g.tap_shift = w.causal ? -1 : 0;
        g.Fr = (int)Fr;
        g.Cin = D;
        g.zeros = zero_page;
        // the side embeddings (f0, phase, volume, speaker) are added in this GEMM's epilogue
        if (conv_split) {
            g.K /= KS_SPLITS;
            g.kz = g.K;
            EpiEmbed e{bf.kpart, w.prenet_conv2_b, in.f0, in.phase, in.volume, w, in.spk_id, in.n_spk_id, in.mix, (int)Fr, dev_err, M * D};
            PROF(PF_U2C_GEMM_CONV3, 2.0 * M * D * 3 * D, 8.0 * M * D,
                 (gemm::dma_go<64, 64, EpiEmbed, 4, 4, gemm::A_CONV3>(st, g, KS_SPLITS, e)));
            pending = LnPending{bf.kpart, nullptr, x, 0};   // layer 0's LayerNorm sums the four partial products into x
        } else {
            EpiEmbed e{x, w.prenet_conv2_b, in.f0, in.phase, in.volume, w, in.spk_id, in.n_spk_id, in.mix, (int)Fr, dev_err, 0};
            // large batches: the convolution, the embeddings AND the first block's LayerNorm in one kernel (gemm_ln.h with the
            // 3-tap loader; same bits as the pair of launches)
            gemm::LnArgs la = ln_args(g, x, x, w.prenet_conv2_b, w.layer[0].norm_w, w.layer[0].norm_b, bf.l[0].y);
            la.Fr = (int)Fr;
            la.Cin = D;
            la.tap_shift = g.tap_shift;
            la.zeros = zero_page;
            if (ln_fusable(g, la) && g.A_split && D + 32 <= DDSP_ZERO_FLOATS) {
                PROF(PF_U2C_GEMM_CONV3, 2.0 * M * D * 3 * D, 12.0 * M * D,
                     DDSP_HIP(ctx, (gemm::launch_res_ln_rb<2, true, gemm::A_CONV3, PreEmbed>(st, la, PreEmbed{e}))));
                ln_done = true;
            } else
                PROF(PF_U2C_GEMM_CONV3, 2.0 * M * D * 3 * D, 8.0 * M * D, (gemm::launch<true, true, gemm::A_CONV3>(st, g, 1, e)));
        }
    }
    DDSP_LAUNCH_CHECK(ctx);

    const unsigned rows_g = (unsigned)ceil_div64(M, 4), rows8_g = (unsigned)ceil_div64(M8, 4);
    // training forward: the random-feature projections (M*8, 64) x (266, 64)^T of q and k, then the exp passes; q' and k'
    // stay in the arena for the backward pass
    auto feature_maps = [&](const LayerBufs& b, const float* proj) {
        gemm::Args g = gemm::make(b.q, DH, proj, DH, (int)M8, NF, DH);
        gemm::EpiStore e{b.qf, LDF, nullptr, 1, 0, 0};
        PROF(PF_U2C_GEMM_FEAT, 2.0 * M8 * NF * DH, 4.0 * M8 * (DH + NF), (gemm::launch<true, true, gemm::A_PLAIN>(st, g, 1, e)));
        g.A = b.k;
        e.C = b.kf;
        PROF(PF_U2C_GEMM_FEAT, 2.0 * M8 * NF * DH, 4.0 * M8 * (DH + NF), (gemm::launch<true, true, gemm::A_PLAIN>(st, g, 1, e)));
        PROF(PF_U2C_ROWWISE, 0, 4.0 * M8 * (2 * NF + DH),
             hipLaunchKernelGGL(feature_map_kernel<true>, dim3(rows8_g), dim3(256), 0, st, b.qf, b.q, M8));
        PROF(PF_U2C_ROWWISE, 0, 4.0 * M8 * (2 * NF + DH),
             hipLaunchKernelGGL(feature_map_kernel<false>, dim3(rows8_g), dim3(256), 0, st, b.kf, b.k, M8));
    };
    const float* ln_src = nullptr;   // where the next LayerNorm finds the residual stream (null: the layer's own x_in)
    for (int l = 0; l < 3; ++l) {
        const ddsp_u2c_layer& L = w.layer[l];
        LayerBufs& b = bf.l[l];
        // -- x_mid = x_in + to_out(linear_attention(LN(x_in)))
        if (!ln_done)
            PROF(PF_U2C_ROWWISE, 0, 8.0 * M * D,
                 hipLaunchKernelGGL(layernorm_kernel, dim3(rows_g), dim3(256), 0, st, ln_src ? ln_src : b.x_in, L.norm_w, L.norm_b, M, b.y, asplit, pending));
        ln_done = false;
        pending = LnPending{nullptr, nullptr, nullptr, 0};
        {
            gemm::Args g = gemm::make(b.y, D, bf.wqkv + (size_t)l * 3 * INNER * D, D, iM, 3 * INNER, D);
            set_b(g, bf.wqkv + (size_t)l * 3 * INNER * D, asplit);
            EpiSplit3 e{{b.q, b.k, b.v}, bf.bqkv + (size_t)l * 3 * INNER};
            PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * 3 * INNER * D, 4.0 * M * (D + 3 * INNER),
                 (gemm::launch<true, true, gemm::A_PLAIN>(st, g, 1, e)));
        }
        if (attn_bf16) {
            // inference, split-bf16 products, enough (utterance, head) pairs to fill the chip with one workgroup each:
            // the LDS-staged bf16 kernels (performer_attn_bf16.hip); the output is written as the out-projection's A operand
            void* p3 = (char*)bf.p3 + (size_t)l * PERFORMER_P3_BYTES;
            // both sides in one kernel per (utterance, head): ctx and ks stay in its LDS (round 3)
            PROF(PF_U2C_GEMM_CTX, 8.0 * M8 * NF * DH, 4.0 * M * 4 * INNER,
                 DDSP_HIP(ctx, performer_fused_bf16(st, b.q, b.k, b.v, p3, (int)B, (int)Fr, b.attn, asplit, in.n_frames)));
        } else if (w.causal && !b.pre) {
            // causal mode, inference: chunked linear attention in one kernel (performer_attn.hip); q' / k' never reach HBM
            PROF(PF_U2C_GEMM_ATTNOUT, 2.0 * M8 * (3.0 * NF * DH + 16.0 * (NF + DH)) + 4.0 * M8 * NF * DH, 4.0 * M * 4 * INNER,
                 performer_causal(st, b.q, b.k, b.v, L.proj, (int)B, (int)Fr, b.attn));
        } else if (w.causal) {
            // causal mode, training forward: the feature maps, then the sequential causal attention kernel
            feature_maps(b, L.proj);
            PROF(PF_U2C_GEMM_ATTNOUT, 4.0 * M8 * NF * DH, 4.0 * M8 * (2 * NF + 2 * DH),
                 hipLaunchKernelGGL(causal_attention_kernel, dim3((unsigned)(B * H)), dim3(256), 0, st, b.qf, b.kf, b.v, (int)Fr, b.attn));
        } else if (!b.pre) {
            // inference: fused feature maps + linear attention (performer_attn.hip); q'/k' never reach HBM
            PROF(PF_U2C_GEMM_CTX, 4.0 * M8 * NF * DH, 4.0 * M * 2 * INNER,
                 performer_kv(st, b.k, b.v, L.proj, (int)B, (int)Fr, b.cx, b.ks, in.n_frames));
            PROF(PF_U2C_GEMM_ATTNOUT, 4.0 * M8 * NF * DH, 4.0 * M * 2 * INNER,
                 performer_q(st, b.q, L.proj, b.cx, b.ks, (int)B, (int)Fr, b.attn));
        } else {
            // training forward, non-causal: the feature maps, key sums, context and output through GEMMs + row kernels
            feature_maps(b, L.proj);
            // ragged batch: k' = 0 over a row's padding, so that the key sums and the context run over its own frames
            if (in.n_frames) PROF(PF_U2C_ROWWISE, 0, 0, zero_padding_frames(st, b.kf, in.n_frames, B, Fr, H * LDF));
            PROF(PF_U2C_ROWWISE, 0, 4.0 * M8 * NF,
                 hipLaunchKernelGGL(key_sum_kernel, dim3((unsigned)(B * H)), dim3(KS_T * 8), 0, st, b.kf, (int)Fr, b.ks));
            {   // ctx[b,h] (266 x 64) = k'^T v : A stored [n][j] (K x M), B stored [n][e] (K x N)
                gemm::Args g = gemm::make(b.kf, (int64_t)H * LDF, b.v, INNER, NF, DH, (int)Fr);
                g.zdiv = H;
                g.sA_hi = (int64_t)Fr * H * LDF;
                g.sA_lo = LDF;
                g.sB_hi = (int64_t)Fr * INNER;
                g.sB_lo = DH;
                gemm::EpiStore e{b.cx, DH, nullptr, 1, (int64_t)NF * DH, 0};
                PROF(PF_U2C_GEMM_CTX, 2.0 * M8 * NF * DH, 4.0 * M8 * (NF + DH),
                     (gemm::launch_tile<64, 64, false, false, gemm::A_PLAIN>(st, g, (int)(B * H), e)));
            }
            PROF(PF_U2C_ROWWISE, 0, 4.0 * M8 * NF,
                 hipLaunchKernelGGL(attn_denominator_kernel, dim3(rows8_g), dim3(256), 0, st, b.qf, b.ks, (int)Fr, M8, b.dinv));
            {   // out[b,n,h,:] = dinv * (q'[b,n,h,:] ctx[b,h])
                gemm::Args g = gemm::make(b.qf, (int64_t)H * LDF, b.cx, DH, (int)Fr, DH, NF);
                g.zdiv = H;
                g.sA_hi = (int64_t)Fr * H * LDF;
                g.sA_lo = LDF;
                g.sB_hi = (int64_t)H * NF * DH;
                g.sB_lo = (int64_t)NF * DH;
                EpiAttnOut e{b.attn, b.dinv, (int)Fr};
                PROF(PF_U2C_GEMM_ATTNOUT, 2.0 * M8 * NF * DH, 4.0 * M8 * (NF + DH),
                     (gemm::launch_tile<64, 64, true, false, gemm::A_PLAIN>(st, g, (int)(B * H), e)));
            }
        }
        {
            gemm::Args g = gemm::make(b.attn, INNER, L.out_w, INNER, iM, D, INNER);
            set_b(g, bf.wout + (size_t)l * D * INNER, attn_bf16 ? asplit : 0);
            const gemm::LnArgs la = ln_args(g, b.x_in, b.x_mid, L.out_b, L.cm_ln_w, L.cm_ln_b, b.y2);
            if (ln_fusable(g, la)) {
                PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * D * INNER, 4.0 * M * (INNER + 4 * D), DDSP_HIP(ctx, gemm::launch_res_ln(st, la, g.A_split != 0)));
                ln_done = true;
                ln_src = b.x_mid;
            } else
                PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * D * INNER, 4.0 * M * (INNER + 2 * D), ln_src = residual_gemm(g, b.x_in, b.x_mid, L.out_b));
        }
        // -- x_out = x_mid + conv_module(x_mid)
        if (!ln_done)
            PROF(PF_U2C_ROWWISE, 0, 8.0 * M * D,
                 hipLaunchKernelGGL(layernorm_kernel, dim3(rows_g), dim3(256), 0, st, ln_src, L.cm_ln_w, L.cm_ln_b, M, b.y2, asplit, pending));
        ln_done = false;
        pending = LnPending{nullptr, nullptr, nullptr, 0};
        if (fuse_glu) {
            gemm::Args g = gemm::make(b.y2, D, bf.wglu + (size_t)l * 2 * INNER * D, D, iM, 2 * INNER, D);
            set_b(g, bf.wglu + (size_t)l * 2 * INNER * D, asplit);
            EpiGlu e{b.glu, bf.bglu + (size_t)l * 2 * INNER};
            DDSP_REQUIRE(ctx, gemm::dma_ok(g) && ((uintptr_t)b.glu % 16) == 0, "unit2ctrl: fused GLU needs aligned activations");
            if (glu_large) {
                PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * 2 * INNER * D, 4.0 * M * (D + INNER),
                     (gemm::dma_go<128, 128, EpiGlu, 2>(st, g, 1, e)));
            } else {
                PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * 2 * INNER * D, 4.0 * M * (D + INNER),
                     (gemm::dma_go<64, 128, EpiGlu, 3, 4>(st, g, 1, e)));
            }
        } else {
            {
                gemm::Args g = gemm::make(b.y2, D, L.cm_pw1_w, D, iM, 2 * INNER, D);
                g.math = lin_math;
                gemm::EpiStore e{b.g1, 2 * INNER, L.cm_pw1_b, 1, 0, 0};
                PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * 2 * INNER * D, 4.0 * M * (D + 2 * INNER),
                     (gemm::launch<true, true, gemm::A_PLAIN>(st, g, 1, e)));
            }
            PROF(PF_U2C_ROWWISE, 0, 12.0 * M * INNER,
                 hipLaunchKernelGGL(glu_kernel, dim3(grid_for(M * (INNER / 4))), dim3(256), 0, st, b.g1, M, b.glu));
        }
        // Large batches on split operands: the convolution + SiLU is formed in pw2's own operand stage (gemm_ln.h A_DWCONV): no
        // launch, no (M, 512) round trip.  Same bits.  Training, fp32 products, the register-pair switch, batches below
        // U2C_DWCONV_FUSE_MIN_ROWS and batches of short utterances keep the two launches.
        gemm::LnArgs dwl{};
        bool dw_fused = false;
        {
            gemm::Args g = gemm::make(b.glu, INNER, L.cm_pw2_w, INNER, iM, D, INNER);
            set_b(g, bf.wpw2 + (size_t)l * D * INNER, asplit);
            const float* n_g = l + 1 < 3 ? w.layer[l + 1].norm_w : w.final_ln_w;
            const float* n_b = l + 1 < 3 ? w.layer[l + 1].norm_b : w.final_ln_b;
            dwl = ln_args(g, b.x_mid, b.x_out, L.cm_pw2_b, n_g, n_b, l + 1 < 3 ? bf.l[l + 1].y : bf.y_final);
            dwl.Fr = (int)Fr;
            dwl.zeros = zero_page;
            dwl.dw_taps = bf.wdw + (size_t)l * DWK * INNER;
            dwl.dw_bias = L.cm_dw_b;
            dwl.n_frames = in.n_frames;
            dwl.dw_left = w.causal ? DWK - 1 : DWK / 2;
            dw_fused = asplit && dw_tiled && M >= U2C_DWCONV_FUSE_MIN_ROWS && B * ((Fr + 15) / 16) >= 512 && ln_fusable(g, dwl) && gemm::res_ln_dwconv_ok(dwl) &&
                       gemm::res_ln_dwconv_fills(B, Fr);
        }
        if (dw_fused) {
            PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * D * INNER + 2.0 * M * INNER * DWK, 4.0 * M * (INNER + 4 * D),
                 DDSP_HIP(ctx, gemm::launch_res_ln_dwconv(st, dwl)));
            ln_done = true;
            ln_src = b.x_out;
            DDSP_LAUNCH_CHECK(ctx);
            continue;
        }
        PROF(PF_U2C_ROWWISE, 2.0 * M * INNER * DWK, 8.0 * M * INNER,
             if (!b.pre && dw_tiled && B * ((Fr + 15) / 16) >= 512)
                 // inference, large batches: LDS-staged tiles of 64 frames x 64 channels
                 hipLaunchKernelGGL(dwconv_tile_kernel, dim3(INNER / DWT_C, (unsigned)(B * ((Fr + DWT_F - 1) / DWT_F))), dim3(256), 0, st,
                                    b.glu, bf.wdw + (size_t)l * DWK * INNER, L.cm_dw_b, (int)B, (int)Fr, b.dwo, w.causal ? DWK - 1 : DWK / 2, asplit, in.n_frames);
             else if (!b.pre && B * ((Fr + 15) / 16) >= 512)
                 // inference, large batches: two channels per thread on packed multiply-adds, runs of 16 frames
                 hipLaunchKernelGGL((dwconv_pair_kernel<16>), dim3(1, (unsigned)(B * ((Fr + 15) / 16))), dim3(256), 0, st,
                                    b.glu, bf.wdw + (size_t)l * DWK * INNER, L.cm_dw_b, (int)B, (int)Fr, b.dwo, w.causal ? DWK - 1 : DWK / 2, asplit, in.n_frames);
             else if (B * ((Fr + DW_RUN - 1) / DW_RUN) >= 64)
                 hipLaunchKernelGGL((dwconv_kernel<true, false>), dim3(INNER / 256, (unsigned)(B * ((Fr + DW_RUN - 1) / DW_RUN))),
                                    dim3(256), 0, st, b.glu, bf.wdw + (size_t)l * DWK * INNER, L.cm_dw_b, (int)B, (int)Fr, b.dwo, b.pre, 1, INNER, w.causal ? DWK - 1 : DWK / 2, asplit, in.n_frames);
             else   // a few utterances (the real-time block): runs of 8 frames, four times as many workgroups
                 hipLaunchKernelGGL((dwconv_kernel<true, false, 8>), dim3(INNER / 256, (unsigned)(B * ((Fr + 7) / 8))),
                                    dim3(256), 0, st, b.glu, bf.wdw + (size_t)l * DWK * INNER, L.cm_dw_b, (int)B, (int)Fr, b.dwo, b.pre, 1, INNER, w.causal ? DWK - 1 : DWK / 2, asplit, in.n_frames));
        {
            gemm::Args g = gemm::make(b.dwo, INNER, L.cm_pw2_w, INNER, iM, D, INNER);
            set_b(g, bf.wpw2 + (size_t)l * D * INNER, asplit);
            // (the LayerNorm behind pw2 is the next layer's, or the final one)
            const float* n_g = l + 1 < 3 ? w.layer[l + 1].norm_w : w.final_ln_w;
            const float* n_b = l + 1 < 3 ? w.layer[l + 1].norm_b : w.final_ln_b;
            float* n_y = l + 1 < 3 ? bf.l[l + 1].y : bf.y_final;
            const gemm::LnArgs la = ln_args(g, b.x_mid, b.x_out, L.cm_pw2_b, n_g, n_b, n_y);
            if (ln_fusable(g, la)) {
                PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * D * INNER, 4.0 * M * (INNER + 4 * D), DDSP_HIP(ctx, gemm::launch_res_ln(st, la, g.A_split != 0)));
                ln_done = true;
                ln_src = b.x_out;
            } else
                PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * D * INNER, 4.0 * M * (INNER + 2 * D), ln_src = residual_gemm(g, b.x_mid, b.x_out, L.cm_pw2_b));
        }
        DDSP_LAUNCH_CHECK(ctx);
    }
    // ---- LayerNorm -> weight-normed head ----
    if (!ln_done)
        PROF(PF_U2C_ROWWISE, 0, 8.0 * M * D,
             hipLaunchKernelGGL(layernorm_kernel, dim3(rows_g), dim3(256), 0, st, ln_src, w.final_ln_w, w.final_ln_b,
                                M, bf.y_final, asplit, pending));
    {
        gemm::Args g = gemm::make(bf.y_final, D, bf.wh, D, iM, w.n_out, D);
        set_b(g, bf.wh, asplit);
        gemm::EpiStore e{ctrl, w.n_out, w.head_b, 1, 0, 0};
        gemm::WsStore ew{ctrl, w.n_out, w.head_b};
        // Large batches: the wave-specialised kernel (gemm_ws.h: loader / product waves, epilogue pieces riding in the next
        // tile) once its 128x128 tiles make at least two rounds over the 256 CUs.  Same bits as kernel_dma.  Which layers:
        // measured INSIDE the forward (rocprofv3, B = 64: DESIGN section 9) - the head gains (31.7 -> 28.4 us), QKV and
        // pw1 + GLU do not (42.5 -> 43.9, 25.0 -> 27.9 us, although alone, with operands resident in the L2, they run
        // 44.5 -> 38.8 and 30.0 -> 25.3), so only the head uses it.
        const bool use_ws = presplit_w && g.math == DDSP_MATH_SPLIT_BF16 && gemm::ws_ok(g) && g.N % 128 == 0 &&
                            (int64_t)((g.M + 127) / 128) * (g.N / 128) >= 512;
        if (use_ws && ew.vec_ok()) {
            PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * w.n_out * D, 4.0 * M * (D + w.n_out),
                 DDSP_HIP(ctx, (gemm::ws_go<128, 128, gemm::WsStore, 4>(st, g, ew))));
        } else {
            PROF(PF_U2C_GEMM_LINEAR, 2.0 * M * w.n_out * D, 4.0 * M * (D + w.n_out),
                 (gemm::launch<true, true, gemm::A_PLAIN>(st, g, 1, e)));
        }
    }
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

int check_inputs(ddsp_ctx* ctx, const ddsp_u2c_weights* wp, const float* units, const float* f0_frames,
                 const float* phase_frames, const float* volume, const int64_t* spk_id, int64_t n_spk_id,
                 const int64_t* mix_ids_host, const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, U2CInputs& in) {
    DDSP_REQUIRE(ctx, ctx && wp && units && f0_frames && phase_frames && volume, "ddsp_unit2ctrl: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && B <= 4096 && Fr >= 1 && B * Fr < (1 << 26), "ddsp_unit2ctrl: bad shape (B <= 4096 per call)");
    DDSP_REQUIRE(ctx, n_mix >= 0 && n_mix <= 16, "ddsp_unit2ctrl: at most 16 mixed speakers");
    DDSP_REQUIRE(ctx, n_mix > 0 || (spk_id && (n_spk_id == 1 || n_spk_id == B)), "ddsp_unit2ctrl: spk_id must hold 1 or B ids");
    DDSP_REQUIRE(ctx, n_mix == 0 || (mix_ids_host && mix_w_host), "ddsp_unit2ctrl: mix arrays missing");
    DDSP_REQUIRE(ctx, wp->n_unit >= 4 && wp->n_unit % 4 == 0 && wp->n_out >= 1 && wp->n_spk >= 1, "ddsp_unit2ctrl: bad widths");
    DDSP_REQUIRE(ctx, wp->causal == 0 || wp->causal == 1, "ddsp_unit2ctrl: causal must be 0 or 1");
    for (int k = 0; k < n_mix; ++k)
        DDSP_REQUIRE(ctx, mix_ids_host[k] >= 1 && mix_ids_host[k] <= wp->n_spk, "ddsp_unit2ctrl: mixed speaker id out of range");
    in.units = units;
    in.f0 = f0_frames;
    in.phase = phase_frames;
    in.volume = volume;
    in.spk_id = spk_id;
    in.n_spk_id = n_spk_id;
    in.mix.n = n_mix;
    for (int i = 0; i < n_mix; ++i) {
        in.mix.ids[i] = mix_ids_host[i];
        in.mix.w[i] = mix_w_host[i];
    }
    in.B = B;
    in.Fr = Fr;
    return DDSP_OK;
}

}  // namespace u2c

// the inference forward behind ddsp_unit2ctrl_fwd, ddsp_unit2ctrl_fwd_rowmix and ddsp_unit2ctrl_fwd_framemix (n_frames null or the counts: the same launches)
static int unit2ctrl_fwd_any(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* wp, const float* units,
                             const float* f0_frames, const float* phase_frames, const float* volume,
                             const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host,
                             const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, const int32_t* n_frames, float* ctrl,
                             const int32_t* mix_ids_dev = nullptr, const float* mix_w_dev = nullptr, int K = 0,
                             int mix_per_frame = 0) {
    U2CInputs in;
    int rc = check_inputs(ctx, wp, units, f0_frames, phase_frames, volume, spk_id, n_spk_id, mix_ids_host, mix_w_host,
                          n_mix, B, Fr, in);
    if (rc) return rc;
    in.n_frames = (const int*)n_frames;
    if (mix_ids_dev) {   // a mix per row: K columns of the two device tables replace the by-value arrays
        in.mix.n = K;
        in.mix.ids_dev = (const int*)mix_ids_dev;
        in.mix.w_dev = mix_w_dev;
        in.mix.per_frame = mix_per_frame;   // mix_w_dev is (B, Fr, K): weights of every frame
    }
    DDSP_REQUIRE(ctx, ctrl, "ddsp_unit2ctrl_fwd: null ctrl");
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    if (B == 0) return DDSP_OK;
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    const ddsp_u2c_weights w = *wp;
    U2CBufs bf;
    Arena wdry{ctx, true, 0, 0};
    plan_weights(wdry, bf, w);
    ddsp_weight_slot* slot;
    if ((rc = ddsp_weight_slot_take(ctx, st, ctx->u2c_slot, &w, offsetof(ddsp_u2c_weights, version), w.version, wdry.total, &slot)))
        return rc;
    const bool cached = slot != nullptr;
    if (cached) {
        Arena wa{ctx, false, 0, 0};
        wa.ext = slot->dev;
        wa.ext_cap = slot->bytes;
        plan_weights(wa, bf, w);
        if (wa.rc) return wa.rc;
        bf.wstate = &slot->state;
    }
    // (the arena is sized for a call WITHOUT the slot too: a capture that follows warm-up calls must not have to grow it)
    Arena dry{ctx, true, 0, 0};
    {
        U2CBufs scratch_plan;
        plan_forward(dry, scratch_plan, w, B, Fr, false, false);
    }
    rc = ddsp_scratch_reserve_bytes(ctx, dry.total + 4096);
    if (rc) return rc;
    ddsp_scratch_reset(ctx);
    Arena a{ctx, false, 0, 0};
    plan_forward(a, bf, w, B, Fr, false, cached);
    if (a.rc) return a.rc;
    return u2c_forward(ctx, st, w, in, bf, ctrl);
}

extern "C" int ddsp_u2c_dwconv_pw2(ddsp_ctx* ctx, void* stream, const float* glu, const float* taps, const float* dw_bias,
                                   const float* W_split, const float* bias, const float* res, const float* gamma,
                                   const float* beta, const int* n_frames, int B, int Fr, int causal, int fused, float* scratch,
                                   float* X, float* Y) {
    DDSP_REQUIRE(ctx, ctx && glu && taps && dw_bias && W_split && bias && res && gamma && beta && X && Y && (fused || scratch),
                 "ddsp_u2c_dwconv_pw2: null argument");
    DDSP_REQUIRE(ctx, B >= 1 && Fr >= 1 && (int64_t)B * Fr < (1 << 26), "ddsp_u2c_dwconv_pw2: bad shape");
    const float* zero_page = nullptr;
    if (int rc = ddsp_zero_page(ctx, &zero_page)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int M = B * Fr, left = causal ? DWK - 1 : DWK / 2;
    gemm::LnArgs a{fused ? glu : scratch, W_split, INNER, INNER, M, INNER, bias, res, X, gamma, beta, Y, 1};
    a.Fr = Fr;
    a.zeros = zero_page;
    a.dw_taps = taps;
    a.dw_bias = dw_bias;
    a.n_frames = n_frames;
    a.dw_left = left;
    DDSP_REQUIRE(ctx, gemm::res_ln_dwconv_ok(a) && ((uintptr_t)glu % 16) == 0, "ddsp_u2c_dwconv_pw2: 16-byte aligned operands");
    DDSP_ENTER_DEVICE(ctx);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    if (fused) {
        DDSP_HIP(ctx, gemm::launch_res_ln_dwconv(st, a));
    } else {
        hipLaunchKernelGGL(dwconv_tile_kernel, dim3(INNER / DWT_C, (unsigned)(B * ((Fr + DWT_F - 1) / DWT_F))), dim3(256), 0, st, glu,
                           taps, dw_bias, B, Fr, scratch, left, 1, n_frames);
        DDSP_HIP(ctx, gemm::launch_res_ln(st, a, true));
    }
    ddsp_prof_end(ctx, st, 2.0 * M * (double)D * INNER + 2.0 * M * (double)INNER * DWK, 4.0 * M * (INNER + 4.0 * D));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// n_frames (null: every row has Fr frames) makes the batch ragged: row b has n_frames[b] frames (device array, int32,
// 1 <= n_frames[b] <= Fr) inside the padded (B, Fr, ...) inputs.  The places that look across frames stop at the row's own end:
// the GroupNorm statistics, the zero padding of the second prenet convolution, the key sums and the context of the linear
// attention, the depthwise convolution's input.  The first convolution reads its input as the caller left it: units of frames
// >= n_frames[b] must be 0 (ddsp_ragged_frames).  Rows of ctrl past a row's count hold values that mean nothing.
extern "C" int ddsp_unit2ctrl_fwd(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* wp, const float* units,
                                  const float* f0_frames, const float* phase_frames, const float* volume,
                                  const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host,
                                  const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, const int32_t* n_frames,
                                  float* ctrl) {
    return unit2ctrl_fwd_any(ctx, stream, wp, units, f0_frames, phase_frames, volume, spk_id, n_spk_id, mix_ids_host, mix_w_host,
                             n_mix, B, Fr, n_frames, ctrl);
}

// A speaker mix per batch row from device tables (include/ddsp_amd.h): the launches of ddsp_unit2ctrl_fwd, whose embedding
// epilogue reads row m / Fr of the tables.  check_inputs sees a one-slot host mix {1: 0} (the speaker path it then needs no
// spk_id for); unit2ctrl_fwd_any replaces it by the tables.
extern "C" int ddsp_unit2ctrl_fwd_rowmix(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* wp, const float* units,
                                         const float* f0_frames, const float* phase_frames, const float* volume,
                                         const int32_t* mix_ids_dev, const float* mix_w_dev, int K, int64_t B, int64_t Fr,
                                         const int32_t* n_frames, float* ctrl) {
    DDSP_REQUIRE(ctx, ctx && mix_ids_dev && mix_w_dev, "ddsp_unit2ctrl_fwd_rowmix: null mix table");
    DDSP_REQUIRE(ctx, K >= 1 && K <= 16, "ddsp_unit2ctrl_fwd_rowmix: 1 <= K <= 16 mixed speakers per row");
    const int64_t one_id = 1;
    const float zero_w = 0.f;
    return unit2ctrl_fwd_any(ctx, stream, wp, units, f0_frames, phase_frames, volume, nullptr, 0, &one_id, &zero_w, 1, B, Fr,
                             n_frames, ctrl, mix_ids_dev, mix_w_dev, K);
}

// A speaker mix per FRAME (include/ddsp_amd.h): the row-mix call whose weight table has a row for every frame, mix_w_dev
// (B, Fr, K); the epilogue reads the weights at row m of the GEMM, the ids still at m / Fr.
extern "C" int ddsp_unit2ctrl_fwd_framemix(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* wp, const float* units,
                                           const float* f0_frames, const float* phase_frames, const float* volume,
                                           const int32_t* mix_ids_dev, const float* mix_w_dev, int K, int64_t B, int64_t Fr,
                                           const int32_t* n_frames, float* ctrl) {
    DDSP_REQUIRE(ctx, ctx && mix_ids_dev && mix_w_dev, "ddsp_unit2ctrl_fwd_framemix: null mix table");
    DDSP_REQUIRE(ctx, K >= 1 && K <= 16, "ddsp_unit2ctrl_fwd_framemix: 1 <= K <= 16 mixed speakers per frame");
    const int64_t one_id = 1;
    const float zero_w = 0.f;
    return unit2ctrl_fwd_any(ctx, stream, wp, units, f0_frames, phase_frames, volume, nullptr, 0, &one_id, &zero_w, 1, B, Fr,
                             n_frames, ctrl, mix_ids_dev, mix_w_dev, K, 1);
}

// ---- a training step's pair: a forward that leaves its activations in a caller-owned region, a backward that starts from them ----
extern "C" int64_t ddsp_unit2ctrl_keep_bytes(const ddsp_u2c_weights* wp, int64_t B, int64_t Fr) {
    if (!wp || B < 0 || Fr < 1) return -1;
    U2CBufs bf;
    Arena dry{nullptr, true, 0, 0};
    plan_forward(dry, bf, *wp, B, Fr, true);
    return (int64_t)dry.total + 256;
}

// n_frames: the counts of a ragged batch, or null (every row has Fr frames); units of frames >= n_frames[b] must be 0, as for
// ddsp_unit2ctrl_fwd.  Activations of the padding frames are kept too, finite and without meaning.
extern "C" int ddsp_unit2ctrl_fwd_keep(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* wp, const float* units,
                                       const float* f0_frames, const float* phase_frames, const float* volume,
                                       const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host,
                                       const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, const int32_t* n_frames,
                                       void* keep, int64_t keep_bytes, float* ctrl) {
    U2CInputs in;
    int rc = check_inputs(ctx, wp, units, f0_frames, phase_frames, volume, spk_id, n_spk_id, mix_ids_host, mix_w_host,
                          n_mix, B, Fr, in);
    if (rc) return rc;
    in.n_frames = (const int*)n_frames;
    DDSP_REQUIRE(ctx, ctrl && keep && ((uintptr_t)keep % 256) == 0, "ddsp_unit2ctrl_fwd_keep: null ctrl / keep, or keep not 256-byte aligned");
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    if (B == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    U2CBufs bf;
    Arena k{ctx, false, 0, 0, (char*)keep, (size_t)keep_bytes};
    plan_forward(k, bf, *wp, B, Fr, true);
    DDSP_REQUIRE(ctx, !k.rc, "ddsp_unit2ctrl_fwd_keep: keep_bytes is smaller than ddsp_unit2ctrl_keep_bytes says");
    return u2c_forward(ctx, (hipStream_t)stream, *wp, in, bf, ctrl);
}
