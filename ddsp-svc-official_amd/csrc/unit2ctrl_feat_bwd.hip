// a15 (backward, round 3): the fused adjoint of the attention's two feature-map sides in split-bf16 arithmetic, for the
// non-causal network (unit2ctrl_bwd.hip runs the rest of the backward pass; its fp32 and causal paths take the five-launch chain).
#include "wgrad_bf16.h"
#include "u2c.h"

namespace {

// ---- fused adjoint of one feature-map side of the attention (round 3, split-bf16 arithmetic) ----
// What five launches did through HBM (EpiRowOuter product -> feature_map_bwd_kernel -> product with the projection), one wavefront
// does in registers for 16 frames of one (utterance, head):
//   S[j][n]  = sum_k mat[j][k] rows[n][k] + rowscale[n] colvec[j]        (j: 266 features, k: 64; 17 x 2 x 3 MFMA 16x16x32)
//   dd       = S * E(feat);  t[n] = sum_j dd;  d_feat = dn (dd - [j == argmax_j feat] t)   (query side; key side: no arg-max term)
//   out[n][d] = sum_j d_feat[j][n] P[j][d] - dn^2 t[n] src[n][d]         (9 x 4 x 3 MFMA)
// The first product is taken transposed (features on the M axis), so a lane owns one frame and 4 consecutive features per
// 16-feature block: the sums over features are in-lane plus two cross-lane steps, and those registers ARE the K operand of the
// second product when the projection is stored in the matching slot order (feat_proj_prep_kernel: slot (g, s) of k-step ks
// holds feature 32 ks + 4 g + s for s < 4 and 32 ks + 16 + 4 g + s - 4 above).  A linear map of a gradient: 3 split products.
__global__ void __launch_bounds__(256) feat_proj_prep_kernel(const float* __restrict__ P, ddsp_u32x4* __restrict__ dst) {
    const int idx = blockIdx.x * 256 + threadIdx.x;   // (ks, blk, lane)
    if (idx >= FB_KS * 4 * 64) return;
    P += (int64_t)blockIdx.y * NF * DH;               // (blockIdx.y > 0: one (266, 64) matrix per (utterance, head) - d_ctx for the d_v product)
    dst += (int64_t)blockIdx.y * FB_PT_VEC;
    const int lane = idx & 63, blk = (idx >> 6) & 3, ks = idx >> 8;
    const int d = 16 * blk + (lane & 15), g = lane >> 4;
    float x[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int j = 32 * ks + (s < 4 ? 4 * g + s : 16 + 4 * g + s - 4);
        x[s] = j < NF ? P[(int64_t)j * DH + d] : 0.f;
    }
    ddsp_u32x4 hi, lo;
    ddsp_split8(x, hi, lo);
    dst[(idx >> 6) * 128 + lane] = hi;   // planar: 64 lanes of hi, then 64 lanes of lo (conflict-free 16-byte LDS reads)
    dst[(idx >> 6) * 128 + 64 + lane] = lo;
}
struct FeatBwdArgs {
    const float* rows;       // query side: d_num (M, 512);            key side: v (M, 512)
    const float* mat;        // query side: ctx (B*H, NF, DH);          key side: d_ctx
    const float* rowscale;   // query side: d_D (M8);                   key side: null (1)
    const float* colvec;     // query side: ks (B*H, LDF);              key side: d_ks
    const float* feat;       // q' / k' (M8, LDF)
    const ddsp_u32x4* pt;    // prepared projection
    const float* proj;       // query side: the projection as stored (NF, DH) - the arg-max term of the feature-map adjoint is the
                             // rank-1 correction -dn t P[arg] of the epilogue (exact fp32) instead of 68 compares per lane
    const float* src;        // q / k (M, 512)
    float* out;              // d_q / d_k (M, 512)
    int Fr;
    const ddsp_u32x4* mat_t; // key side: d_ctx of every (utterance, head) in the projection's layout, for d_v = k' d_ctx; or null
    float* out_v;            // d_v (M, 512)
};
typedef __bf16 fb_bf16x8 __attribute__((ext_vector_type(8)));
constexpr int FB_WAVES = 4;                                 // 16-frame tiles per workgroup
constexpr int FB_MAT_VEC = 17 * 2 * 64 * 2;                 // 16-byte vectors of the staged, split `mat` operand
// LDS: one region holds the split matrix during the first product and the prepared projection during the second (74 816 bytes:
// two workgroups per CU - at ~250 VGPRs a SIMD holds two wavefronts, one of each), then the column vector
constexpr int FB_REGION_VEC = FB_PT_VEC > FB_MAT_VEC ? FB_PT_VEC : FB_MAT_VEC;
constexpr int FB_LDS_BYTES = (FB_REGION_VEC + 68) * 16;
template <bool QUERY>
__global__ void __launch_bounds__(64 * FB_WAVES, 2) attn_feat_bwd_kernel(FeatBwdArgs a) {
    extern __shared__ ddsp_u32x4 fb_lds[];
    ddsp_u32x4* const mats = fb_lds;                  // [blk 17][k-half 2][hi | lo][lane 64]: the A operand of the first product
    ddsp_u32x4* const pts = fb_lds;                   // later: the prepared projection, as stored
    f32x4* const cvs = reinterpret_cast<f32x4*>(fb_lds + FB_REGION_VEC);   // colvec (LDF = 268 floats = 67 vectors)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    // blockIdx.x = (utterance, head), blockIdx.y = 64-frame block: workgroups are dealt to the XCDs round-robin in x-major
    // order, so the full blocks come first and the short tail blocks (172 frames: 4 + 4 + 3 tiles) last
    const int bh = blockIdx.x, b = bh / H, h = bh % H;
    const int f0 = (blockIdx.y * FB_WAVES + wave) * 16;
    const bool active = f0 < a.Fr;                    // (idle wavefronts of a tail block still stage and meet the barriers)
    const bool live = f0 + n < a.Fr;
    const int f = live ? f0 + n : a.Fr - 1;
    const int64_t row = ((int64_t)b * a.Fr + f) * H + h;
    const float dn = 0.35355339059327373f, ratio = 0.06131393394849658f;

    {   // stage: every thread splits its share of the (266, 64) matrix once for the workgroup
        const float* mat = a.mat + (int64_t)bh * NF * DH;
        constexpr int NT = 64 * FB_WAVES, MAT_IT = (17 * 2 * 64 + NT - 1) / NT;
        f32x4 mu[MAT_IT], mv[MAT_IT];
#pragma unroll
        for (int i = 0; i < MAT_IT; ++i) {   // all loads of the stage are issued before the first use
            const int e = threadIdx.x + i * NT;
            const int el = e & 63, kh = (e >> 6) & 1, blk = e >> 7;
            const int j = 16 * blk + (el & 15);
            mu[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            mv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (e < 17 * 2 * 64 && j < NF) {
                const float* p = mat + (int64_t)j * DH + 32 * kh + 8 * (el >> 4);
                mu[i] = *(const f32x4*)p;
                mv[i] = *(const f32x4*)(p + 4);
            }
        }
#pragma unroll
        for (int i = 0; i < MAT_IT; ++i) {
            const int e = threadIdx.x + i * NT;
            if (e < 17 * 2 * 64) {
                const float x[8] = {mu[i][0], mu[i][1], mu[i][2], mu[i][3], mv[i][0], mv[i][1], mv[i][2], mv[i][3]};
                ddsp_u32x4 hi, lo;
                ddsp_split8(x, hi, lo);
                mats[(e >> 6) * 128 + (e & 63)] = hi;
                mats[(e >> 6) * 128 + 64 + (e & 63)] = lo;
            }
        }
        if (threadIdx.x < LDF / 4) cvs[threadIdx.x] = *(const f32x4*)(a.colvec + (int64_t)bh * LDF + 4 * threadIdx.x);
    }
    fb_bf16x8 xh[2], xl[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
        const float* p = a.rows + row * DH + 32 * kh + 8 * g;
        const f32x4 u = *(const f32x4*)p, v = *(const f32x4*)(p + 4);
        const float x[8] = {u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
        ddsp_u32x4 hi, lo;
        ddsp_split8(x, hi, lo);
        xh[kh] = __builtin_bit_cast(fb_bf16x8, hi);
        xl[kh] = __builtin_bit_cast(fb_bf16x8, lo);
    }
    // this lane's slice of the feature row (17 x 16 bytes, the only large HBM stream of the kernel), the row scale and the
    // epilogue's source row: in flight while the first product runs
    const float* fr = a.feat + row * LDF;
    f32x4 fvv[17];
#pragma unroll
    for (int blk = 0; blk < 17; ++blk) {
        fvv[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (16 * blk + 4 * g < NF) fvv[blk] = *(const f32x4*)(fr + 16 * blk + 4 * g);   // (rows are LDF = 268 floats: the last group that holds a feature is 264..267)
    }
    const float rs = QUERY ? a.rowscale[row] : 1.0f;
    f32x4 s4[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) s4[blk] = *(const f32x4*)(a.src + row * DH + 16 * blk + 4 * g);
    __syncthreads();
    f32x4 S[17];
#pragma unroll
    for (int blk = 0; blk < 17; ++blk) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (active) {
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) {
                const ddsp_u32x4* p = mats + (blk * 2 + kh) * 128 + lane;
                const fb_bf16x8 mh = __builtin_bit_cast(fb_bf16x8, p[0]), ml = __builtin_bit_cast(fb_bf16x8, p[64]);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ml, xh[kh], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mh, xl[kh], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mh, xh[kh], acc, 0, 0, 0);
            }
        }
        S[blk] = acc;
    }
    __syncthreads();   // every wavefront is done with the matrix
    if (!QUERY && a.mat_t) {
        // key side, d_v[n][d] = sum_j k'[n][j] d_ctx[j][d]: the lane's slice of k' is already the K operand (same slot order as
        // d_feat below), d_ctx^T in the projection's layout (one launch of feat_proj_prep_kernel per layer) takes the region first
        const ddsp_u32x4* src_t = a.mat_t + (int64_t)bh * FB_PT_VEC;
#pragma unroll
        for (int i = 0; i < FB_PT_VEC / 64 / FB_WAVES; ++i) {
            const int piece = wave + FB_WAVES * i;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src_t + 64 * piece + lane),
                                             (__attribute__((address_space(3))) void*)(pts + 64 * piece), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        f32x4 o3[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) o3[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (active) {
#pragma unroll
            for (int ks = 0; ks < FB_KS; ++ks) {
                float y[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    y[r] = 32 * ks + 4 * g + r < NF ? fvv[2 * ks][r] : 0.f;
                    y[4 + r] = (2 * ks + 1 < 17 && 32 * ks + 16 + 4 * g + r < NF) ? fvv[2 * ks + 1 < 17 ? 2 * ks + 1 : 16][r] : 0.f;
                }
                ddsp_u32x4 hi, lo;
                ddsp_split8(y, hi, lo);
                const fb_bf16x8 yh = __builtin_bit_cast(fb_bf16x8, hi), yl = __builtin_bit_cast(fb_bf16x8, lo);
#pragma unroll
                for (int blk = 0; blk < 4; ++blk) {
                    const ddsp_u32x4* p = pts + (ks * 4 + blk) * 128 + lane;
                    const fb_bf16x8 ph = __builtin_bit_cast(fb_bf16x8, p[0]), pl = __builtin_bit_cast(fb_bf16x8, p[64]);
                    o3[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl, yh, o3[blk], 0, 0, 0);
                    o3[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, yl, o3[blk], 0, 0, 0);
                    o3[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, yh, o3[blk], 0, 0, 0);
                }
            }
            if (live) {
#pragma unroll
                for (int blk = 0; blk < 4; ++blk) *(f32x4*)(a.out_v + row * DH + 16 * blk + 4 * g) = o3[blk];
            }
        }
        __syncthreads();   // done with d_ctx^T
    }
    // the projection streams into the same region (no registers)
#pragma unroll
    for (int i = 0; i < FB_PT_VEC / 64 / FB_WAVES; ++i) {
        const int piece = wave + FB_WAVES * i;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.pt + 64 * piece + lane),
                                         (__attribute__((address_space(3))) void*)(pts + 64 * piece), 16, 0, 0);
    }
    static_assert(FB_PT_VEC % (64 * FB_WAVES) == 0, "whole 1 KiB pieces per wavefront");
    // feature-map adjoint on the registers (feature of S[blk][r]: 16 blk + 4 g + r) while the projection arrives
    float t = 0.f, best = -3.0e38f;
    int arg = 0x7fffffff;
#pragma unroll
    for (int blk = 0; blk < 17; ++blk) {
        const int j0 = 16 * blk + 4 * g;
        const f32x4 fv = fvv[blk];
        f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
        if (j0 < NF) c4 = cvs[4 * blk + g];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool valid = blk < 16 || j0 + r < NF;   // (only the last block holds pad features)
            const float E = QUERY ? fv[r] - ratio * 1e-4f : fv[r];
            const float dd = valid ? fmaf(rs, c4[r], S[blk][r]) * E : 0.f;
            S[blk][r] = dd;
            t += dd;
            if (QUERY && valid && fv[r] > best) {
                best = fv[r];
                arg = j0 + r;
            }
        }
    }
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    if (QUERY) {   // first index of the row maximum, like feature_map_bwd_kernel
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(arg, o, 64);
            if (ob > best || (ob == best && oa < arg)) {
                best = ob;
                arg = oa;
            }
        }
    }
    f32x4 pa[4];
    if (QUERY) {   // row `arg` of the projection (arg is the same in the four lanes of a frame), in flight under the second product
        const int ja = arg < NF ? arg : 0;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) pa[blk] = *(const f32x4*)(a.proj + (int64_t)ja * DH + 16 * blk + 4 * g);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!active) return;
    f32x4 o4[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) o4[blk] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < FB_KS; ++ks) {
        float y[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            y[r] = dn * S[2 * ks][r];
            y[4 + r] = 2 * ks + 1 < 17 ? dn * S[2 * ks + 1 < 17 ? 2 * ks + 1 : 16][r] : 0.f;
        }
        ddsp_u32x4 hi, lo;
        ddsp_split8(y, hi, lo);
        const fb_bf16x8 yh = __builtin_bit_cast(fb_bf16x8, hi), yl = __builtin_bit_cast(fb_bf16x8, lo);
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            const ddsp_u32x4* p = pts + (ks * 4 + blk) * 128 + lane;
            const fb_bf16x8 ph = __builtin_bit_cast(fb_bf16x8, p[0]), pl = __builtin_bit_cast(fb_bf16x8, p[64]);
            o4[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl, yh, o4[blk], 0, 0, 0);
            o4[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, yl, o4[blk], 0, 0, 0);
            o4[blk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph, yh, o4[blk], 0, 0, 0);
        }
    }
    if (!live) return;
    const float coef = -(dn * dn) * t;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
        const int64_t off = row * DH + 16 * blk + 4 * g;
        f32x4 r4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            r4[r] = fmaf(coef, s4[blk][r], o4[blk][r]);
            if (QUERY) r4[r] = fmaf(arg < NF ? -dn * t : 0.f, pa[blk][r], r4[r]);
        }
        *(f32x4*)(a.out + off) = r4;
    }
}

}  // namespace

namespace u2c {

void feat_proj_prep(hipStream_t st, const float* P, int n, float* dst) {
    hipLaunchKernelGGL(feat_proj_prep_kernel, dim3((FB_KS * 4 * 64 + 255) / 256, (unsigned)n), dim3(256), 0, st, P,
                       reinterpret_cast<ddsp_u32x4*>(dst));
}

int attn_feat_bwd(ddsp_ctx* ctx, hipStream_t st, const LayerBufs& b, const float* proj, const float* pt, float* dnum,
                  const float* dD, float* dcx, float* dks, float* dcxt, float* dk, float* dv, int64_t B, int64_t Fr) {
    // d_ctx = q'^T d_num: the frames are the slow axis of both operands, so it runs on the weight-gradient kernel with one
    // problem per (utterance, head)
    wgrad::Args g;
    g.dY = b.qf;
    g.ldy = (int64_t)H * LDF;
    g.O = NF;
    g.X = dnum;
    g.ldx = INNER;
    g.C = DH;
    g.taps = 1;
    g.tap_shift = 0;
    g.Fr = (int)Fr;
    g.M = Fr;
    g.chunk = 32;
    g.partial = dcx;
    g.bias_partial = dks;          // d_ks = q'^T d_D rides in the staging threads (was weighted_key_sum_kernel)
    g.ldb = LDF;
    g.bias_w = dD;
    g.ldw = H;
    g.sW_hi = (int64_t)Fr * H;
    g.sW_lo = 1;
    g.zdiv = H;
    g.sY_hi = (int64_t)Fr * H * LDF;
    g.sY_lo = LDF;
    g.sX_hi = (int64_t)Fr * INNER;
    g.sX_lo = DH;
    wgrad::launch<1, 1>(st, g, (int)(B * H));   // (128-row tiles: no difference, 5.72 / 5.75 ms over two runs)
    const dim3 fgrid((unsigned)(B * H), (unsigned)((Fr + 16 * FB_WAVES - 1) / (16 * FB_WAVES)));
    DDSP_ONCE_PER_DEVICE(ctx, DDSP_HIP(ctx, hipFuncSetAttribute((const void*)attn_feat_bwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, FB_LDS_BYTES));
                         DDSP_HIP(ctx, hipFuncSetAttribute((const void*)attn_feat_bwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, FB_LDS_BYTES)));
    const ddsp_u32x4* ptv = reinterpret_cast<const ddsp_u32x4*>(pt);
    // d_v = k' d_ctx folded into the key side: d_ctx of every (utterance, head) in the projection's layout
    feat_proj_prep(st, dcx, (int)(B * H), dcxt);
    FeatBwdArgs fq{dnum, b.cx, dD, b.ks, b.qf, ptv, proj, b.q, dnum, (int)Fr, nullptr, nullptr};
    hipLaunchKernelGGL(attn_feat_bwd_kernel<true>, fgrid, dim3(64 * FB_WAVES), FB_LDS_BYTES, st, fq);
    FeatBwdArgs fk{b.v, dcx, nullptr, dks, b.kf, ptv, nullptr, b.k, dk, (int)Fr, reinterpret_cast<const ddsp_u32x4*>(dcxt), dv};
    hipLaunchKernelGGL(attn_feat_bwd_kernel<false>, fgrid, dim3(64 * FB_WAVES), FB_LDS_BYTES, st, fk);
    return DDSP_OK;
}

}  // namespace u2c
