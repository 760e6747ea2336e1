// What the halves of the unit -> control network share (unit2ctrl_fwd.hip: weight preparation, the forward kernels and the
// forward pass; unit2ctrl_bwd.hip: the backward kernels and the backward pass; unit2ctrl_feat_bwd.hip: the fused feature-map
// adjoint of the attention): the model's constants, the templates both passes instantiate, and the buffer plan of a forward
// pass, which the backward pass re-runs or starts from.
// The kernels and their argument types live in the anonymous namespace (their symbols are the same in every file); the host
// types and functions that cross between the files are in namespace u2c (MixArgs too: U2CInputs carries it).
#pragma once
#include "common.h"

namespace {

constexpr int D = 256;        // model width
constexpr int H = 8;          // heads
constexpr int DH = 64;        // head dim
constexpr int INNER = 512;    // H*DH, also the conv-module inner width
constexpr int NF = 266;       // random features, int(64*ln 64)
constexpr int LDF = 268;      // padded leading dim of feature rows (16-byte aligned rows)
constexpr int DWK = 31;       // depthwise kernel
// threads per padded feature row in key_sum_kernel / weighted_key_sum_kernel
constexpr int KS_T = LDF / 4;
static_assert(LDF % 4 == 0 && KS_T * 8 <= 1024, "key_sum block");
// the projection prepared for attn_feat_bwd_kernel: 16-byte vectors in FB_KS k-steps (266 features padded to 288)
constexpr int FB_KS = 9;
constexpr int FB_PT_VEC = FB_KS * 4 * 64 * 2;

#define PROF(id, flops, bytes, ...)              \
    do {                                          \
        ddsp_prof_begin(ctx, st, id);             \
        __VA_ARGS__;                              \
        ddsp_prof_end(ctx, st, (double)(flops), (double)(bytes)); \
    } while (0)

inline unsigned grid_for(int64_t total, int per_block = 256, int cap = 8192) {
    int64_t g = (total + per_block - 1) / per_block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

struct EpiAttnOut {  // out[(b*Fr+n)*512 + h*64 + e] = dinv[(b*Fr+n)*8+h] * acc   (z = b*8+h, m = n, col = e); dinv null -> 1
    float* out;
    const float* dinv;
    int Fr;
    __device__ __forceinline__ float col(int) const { return 0.f; }
    __device__ __forceinline__ void operator()(int z, int m, int e, float v, float) const {
        const int b = z / H, h = z % H;
        const int64_t row = (int64_t)b * Fr + m;
        out[row * INNER + h * DH + e] = dinv ? dinv[row * H + h] * v : v;
    }
};

// depthwise Conv1d(k=31, pad 15, groups=512) over frames + SiLU; weight (512,1,31).
// One thread owns one channel for a run of DW_RUN consecutive frames of one utterance: its 31 taps and a
// sliding window of DW_RUN+30 inputs stay in registers (1.9 loads per output instead of 31); lanes walk
// channels, so every load/store of a wavefront is one contiguous 256-B row segment.  The taps are addressed as
// w[c*wsc + t*wst]: the forward pass reads a copy laid out [tap][channel] (wsc = 1, wst = 512; made by the weight
// preparation launch) so that the 31 tap loads are contiguous rows too - in the (512, 31) parameter layout every
// tap load of a wavefront touches 64 cache lines, which cost more than the convolution itself.
constexpr int DW_RUN = 32;
// SILU: apply SiLU (forward) and optionally keep the pre-activation; FLIP: correlate with reversed taps and no
// bias (the input-gradient of the same convolution).
template <bool SILU, bool FLIP, int RUN = DW_RUN>
__global__ void __launch_bounds__(256) dwconv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, int B, int Fr,
                                                     float* __restrict__ out, float* __restrict__ pre, int wsc, int wst,
                                                     int left, int split,     // left = DWK / 2: centred taps; DWK - 1: causal taps (frames t-30 .. t)
                                                     const int* __restrict__ n_frames = nullptr) {   // ragged batch: input frames >= n_b read as 0 (FLIP: the input gradient is 0 there - the caller clears it)
    // split != 0 (forward, inference): `out` is written as bf16 hi/lo groups of 8 channels (A operand of the pw2 GEMM)
    const int c = blockIdx.x * 256 + threadIdx.x;       // channel (INNER = 512 -> 2 blocks in x)
    const int runs = (Fr + RUN - 1) / RUN;
    const int b = blockIdx.y / runs, f0 = (blockIdx.y % runs) * RUN;
    float wt[DWK];
#pragma unroll
    for (int t = 0; t < DWK; ++t) wt[t] = w[c * wsc + (FLIP ? DWK - 1 - t : t) * wst];
    const float* xb = x + ((int64_t)b * Fr) * INNER + c;
    const int n_in = ddsp_row_frames(n_frames, b, Fr);
    float win[RUN + DWK - 1];
#pragma unroll
    for (int i = 0; i < RUN + DWK - 1; ++i) {
        const int f = f0 + i - left;
        win[i] = (f >= 0 && f < n_in) ? xb[(int64_t)f * INNER] : 0.f;
    }
    const float bi = FLIP ? 0.f : bias[c];
#pragma unroll
    for (int o = 0; o < RUN; ++o) {
        float acc = bi;
#pragma unroll
        for (int t = 0; t < DWK; ++t) acc = fmaf(wt[t], win[o + t], acc);
        if (f0 + o < Fr) {
            const int64_t idx = ((int64_t)b * Fr + f0 + o) * INNER + c;
            if (SILU) {
                if (pre) pre[idx] = acc;
                const float y = acc * (1.0f / (1.0f + expf(-acc)));
                if (split)
                    ((uint32_t*)out)[idx] = ddsp_split1_group8(y, threadIdx.x & 63);
                else
                    out[idx] = y;
            } else {
                out[idx] = acc;
            }
        }
    }
}

// Ragged batch: x[b][f][0 .. C) = 0 for the frames f >= n_b of every row (C % 4 == 0, 16-byte aligned rows).  A selection, so
// whatever the padding held is gone.  The training forward clears k' with it (the key sums and the context then run over a
// row's own frames), the backward pass the gradients that a frame sum spread over the padding (d_k, d_v).
__global__ void __launch_bounds__(256) zero_padding_frames_kernel(float* __restrict__ x, const int* __restrict__ n_frames,
                                                                  int64_t B, int Fr, int C4) {
    const int64_t total = B * Fr * C4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t row = idx / C4;
        if ((int)(row % Fr) >= ddsp_row_frames(n_frames, row / Fr, Fr)) ((f32x4*)x)[idx] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
inline void zero_padding_frames(hipStream_t st, float* x, const int* n_frames, int64_t B, int64_t Fr, int C) {
    hipLaunchKernelGGL(zero_padding_frames_kernel, dim3(grid_for(B * Fr * (C / 4))), dim3(256), 0, st, x, n_frames, B, (int)Fr, C / 4);
}

}  // namespace

namespace u2c {

// speaker mix of a call (up to 16 table rows and their weights; n == 0: the spk_id path).  One mix for the whole batch travels
// by value in ids / w; a mix per batch row (ddsp_unit2ctrl_fwd_rowmix, inference) lives in two device tables of n columns,
// ids_dev (B, n) 1-based and w_dev (B, n), and ids / w are then unused.  per_frame (ddsp_unit2ctrl_fwd_framemix): w_dev is
// (B * Fr, n), a row of weights for every frame; ids_dev stays one row per batch row.
struct MixArgs {
    int n;
    long long ids[16];
    float w[16];
    const int* ids_dev = nullptr;
    const float* w_dev = nullptr;
    int per_frame = 0;
};

// ---- buffers of one forward pass --------------------------------------------------------------------------------
// Inference aliases the three layers onto one set and updates the residual stream in place; training keeps every
// activation the adjoints need (about 38 KB per frame and layer).
struct LayerBufs {
    float *x_in, *y, *q, *k, *v, *qf, *kf, *ks, *cx, *dinv, *attn, *x_mid, *y2, *g1, *glu, *pre, *dwo, *x_out;
};
struct U2CBufs {
    float *w1, *w2, *wh, *wqkv, *bqkv, *wglu, *bglu, *wdw, *wout, *wpw2, *p3, *t1, *t2, *gst, *y_final, *kpart;
    LayerBufs l[3];
    // the weight buffers live in the context's prepared-weight slot: what it holds (bit 0 prepared, bit 1 with split copies, bit 2
    // in fused-GLU order, bit 3 attention pieces), updated by the forward that prepares; null: prepare on every call
    int* wstate = nullptr;
};

struct Arena {  // sizes first (dry run), then pointers
    ddsp_ctx* ctx;
    bool dry;
    size_t total;
    int rc;
    char* ext = nullptr;   // a caller-owned region instead of the context's scratch (kept activations of a training step)
    size_t ext_cap = 0;
    float* get(size_t n_floats) {
        const size_t bytes = ((n_floats * sizeof(float) + 255) & ~(size_t)255) + 256;
        if (dry) {
            total += bytes;
            return nullptr;
        }
        if (ext) {
            if (total + bytes > ext_cap) {
                rc = DDSP_ERR_ARG;
                return nullptr;
            }
            float* p = reinterpret_cast<float*>(ext + total);
            total += bytes;
            return p;
        }
        void* p = nullptr;
        const int r = ddsp_scratch_get(ctx, n_floats * sizeof(float), &p);
        if (r) rc = r;
        return (float*)p;
    }
};

struct U2CInputs {
    const float *units, *f0, *phase, *volume;
    const int64_t* spk_id;
    int64_t n_spk_id;
    MixArgs mix;
    int64_t B, Fr;
    const int* n_frames = nullptr;   // device, B entries: frames of each row of a ragged batch; null: every row has Fr
};

// the buffers of a forward pass from the arena; keep: training (every layer's activations), else inference (one aliased set);
// weights_cached: the prepared weights are already planned in the context's slot
void plan_forward(Arena& a, U2CBufs& bf, const ddsp_u2c_weights& w, int64_t B, int64_t Fr, bool keep, bool weights_cached = false);
// the forward pass into planned buffers; ctrl (B*Fr, n_out)
int u2c_forward(ddsp_ctx* ctx, hipStream_t st, const ddsp_u2c_weights& w, const U2CInputs& in, U2CBufs& bf, float* ctrl);
// argument checks shared by every entry point; fills `in`
int check_inputs(ddsp_ctx* ctx, const ddsp_u2c_weights* wp, const float* units, const float* f0_frames, const float* phase_frames,
                 const float* volume, const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host, const float* mix_w_host,
                 int n_mix, int64_t B, int64_t Fr, U2CInputs& in);


// unit2ctrl_feat_bwd.hip, the fused feature-map adjoints of a non-causal layer in split-bf16 arithmetic.
// n (266, 64) matrices P -> dst (n x FB_PT_VEC 16-byte vectors): the projection's layout of the second product
void feat_proj_prep(hipStream_t st, const float* P, int n, float* dst);
// From d_num and d_D of layer buffers b: d_ctx and d_ks into dcx / dks, then d_q (written over d_num), d_k and d_v.  pt: the
// layer's prepared projection; dcxt: room for d_ctx of every (utterance, head) in that layout
int attn_feat_bwd(ddsp_ctx* ctx, hipStream_t st, const LayerBufs& b, const float* proj, const float* pt, float* dnum,
                  const float* dD, float* dcx, float* dks, float* dcxt, float* dk, float* dv, int64_t B, int64_t Fr);

}  // namespace u2c
