// a4 (attention part): fused softmax-kernel feature maps + linear attention, one wavefront per work item, no
// feature-map round trip through HBM.
//
// Replaces, for inference, the chain  [k P^T GEMM -> exp pass -> key sums -> k'^T v GEMM]  and
// [q P^T GEMM -> max/exp pass -> 1/D pass -> q' ctx GEMM]  of ddsp/pcmer.py:69-77,123-159 (unit2ctrl_fwd.hip keeps
// the unfused chain for training, whose backward needs q' and k').  The 94 MB q'/k' matrices per layer never
// exist: a 16 x 16 tile of projected values lives in the MFMA accumulator (4 registers), is exponentiated in place
// and is fed straight back as the next product's operand - accumulator register t of lane group g is the index
// 4g + t of the dimension the next product sums over, which is exactly the 16x16x4 operand layout (k = lane >> 4)
// with the four k of step t permuted; the other operand applies the same permutation.
//   K kernel, item (b, h, 16-feature tile jt): for each 16-frame tile:  S = k_tile P_jt^T (frames x features, lane
//     column = feature), k' = r*exp(dn*S - diag + eps), ks += column sums, ctx_jt (16 features x 64) += k'^T v_tile
//     (output block et of a lane = channel 4c + et, so v is read as one float4 per frame).
//     ctx leaves TRANSPOSED, ctxT[e][j] with row stride 272, so that the Q kernel reads its operand as float4.
//   Q kernel, item (b, h, 16-frame tile ft): for each feature tile  S^T = P_jt q_tile^T (features x frames, lane
//     column = frame), running row maximum (see below), q' in place, D += q'.ks, out^T (64 x 16 frames) +=
//     ctxT_jt q'; the lane then owns 4 consecutive channels of one frame per 16-channel block: float4 stores.
// 16-wide tiles pad 266 features to 272 and 172 frames to 176 (4.6 % of the MACs; 32-wide tiles: 21 %), need ~100
// registers (4 waves per SIMD cover the L2 latency and each other's exp / dependent-MFMA bubbles; the 32-wide
// version sat at 1-2 waves and 43 % MFMA duty), and the first product's operands are read with the permuted-k trick
// (lane group g owns k = 16g..16g+15 of a 64-long row: four 16-byte loads), so there is no LDS staging and no
// barrier.  The four waves of a workgroup take four neighbouring tiles of the SAME (utterance, head): they read the
// same rows at about the same time, so three of the four reads hit the CU's L1.  All arithmetic fp32.
#include "performer_attn.h"

#include <stdlib.h>

namespace {

constexpr int H = 8, DH = 64, INNER = 512, NF = 266;
constexpr int LDJ = PERFORMER_LDJ;             // 272 = 17 feature tiles
constexpr int NJT = LDJ / 16;                  // 17
constexpr int KST = PERFORMER_KS_STRIDE;       // per (utterance, head): ks[272] | column-sum parts[17][64] | ks-sum parts[17]
constexpr int OFF_CPART = LDJ, OFF_KPART = LDJ + NJT * DH;
constexpr int KV_GROUPS = (NJT + 3) / 4;       // workgroups (4 waves = 4 feature tiles) per (utterance, head)
constexpr float DN = 0.35355339059327373f;     // 64^-0.25
constexpr float RATIO = 0.06131393394849658f;  // 266^-0.5
constexpr float EPS = 1e-4f;
constexpr float LOG2E = 1.44269504088896341f;
// Everything inside the exponentials is carried in the base-2 domain (v_exp_f32 IS exp2): the projection operand is
// pre-scaled by dn*log2(e), and -diag = -0.5*dn^2*|x|^2 enters through ONE extra MFMA step whose k-slot g carries
// lane group g's partial sum of squares against the constant below - the matrix pipe does the cross-group sum and
// the broadcast along the tile, no shuffles.  fp32 MFMA and vector ALU instructions do not overlap on this chip
// (SQ_VALU_MFMA_COEXEC_CYCLES = 0, busy + VALU-active cycles add up to the wave time), so every vector instruction
// removed from these loops is matrix time won.
constexpr float PSCALE = DN * LOG2E;
constexpr float NEG_HALF = -0.5f * DN * DN * LOG2E;
constexpr float KOFF = EPS * LOG2E - 4.0276409f;   // eps (inside the key exponential) and log2(266^-0.5)
constexpr float MASKED = -1000.f;                  // exp2 -> 0: pad features / frames are switched off in the C init

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// 16 consecutive floats of a 64-float row (the quarter this lane group owns)
__device__ __forceinline__ void load_quarter_row(const float* __restrict__ row, float (&dst)[16]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const f32x4_t v = *(const f32x4_t*)(row + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[4 * c + e] = v[e];
    }
}

// sum / max over the four lane groups (lanes c, c+16, c+32, c+48)
__device__ __forceinline__ float group_sum(float x) {
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    return x;
}
__device__ __forceinline__ float group_max(float x) {
    x = fmaxf(x, __shfl_xor(x, 16, 64));
    x = fmaxf(x, __shfl_xor(x, 32, 64));
    return x;
}

// PART: the item's frame tiles are dealt over the four waves of a workgroup (tile ft to wave ft & 3) and the partial sums meet
// in the LDS - for few (utterance, head) pairs, where one wave per item walks all tiles alone and the chip is mostly empty
template <bool PART>
__device__ __forceinline__ void performer_kv_item(const float* __restrict__ k, const float* __restrict__ v,
                                                  const float* __restrict__ P, int Fr, const int* __restrict__ n_frames,
                                                  float* __restrict__ ctxT, float* __restrict__ ks, int bh, int jt,
                                                  int ft_first = 0, float* __restrict__ part = nullptr) {
    constexpr int FSTEP = PART ? 4 : 1;
    const int b = bh / H, h = bh % H;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int j = 16 * jt + c;                  // this lane's feature (column of S, row of ctx)
    // out-of-range rows are CLAMPED (finite garbage), and switched off through the accumulator's initial value
    float pb[16];
    load_quarter_row(P + (int64_t)(j < NF ? j : NF - 1) * DH + 16 * g, pb);
#pragma unroll
    for (int s = 0; s < 16; ++s) pb[s] *= PSCALE;
    // the sums run over the row's own frames: all Fr, or (ragged batch) the first nv of them
    const int nv = ddsp_row_frames(n_frames, b, Fr);
    const int n_ft = (nv + 15) / 16;
    f32x4_t c_full, c_last;                      // C init of a full frame tile / of the last (ragged) one
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        c_full[r] = j < NF ? KOFF : MASKED;
        c_last[r] = (j < NF && 16 * (n_ft - 1) + 4 * g + r < nv) ? KOFF : MASKED;
    }
    f32x4_t acc[4];
#pragma unroll
    for (int et = 0; et < 4; ++et) acc[et] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    f32x4_t ksum4 = {0.f, 0.f, 0.f, 0.f};
    const float* kb = k + ((int64_t)b * Fr) * INNER + h * DH;     // wave-uniform bases, 32-bit lane offsets
    const float* vb = v + ((int64_t)b * Fr) * INNER + h * DH;
    const int last = nv - 1;
    // One frame tile.  `cur` holds its k rows, `nxt` receives the next tile's: the two buffers swap roles from tile to
    // tile (loop unrolled by two below).  A copy `ka = kn` at the end of the tile looks harmless but the compiler
    // spreads its v_movs through the FIRST product, which then waits for rows loaded a few MFMAs earlier - the
    // prefetch is gone and every tile pays an L2 round trip.
    auto tile = [&](int ft, const float (&cur)[16], float (&nxt)[16]) {
        // v operand of the second product: frames 4g+t (t = k-step); output block et covers channels 4c + et, so
        // that the four blocks of a lane are ONE 16-byte load per frame
        f32x4_t vv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            int f = 16 * ft + 4 * g + t;
            f = f < nv ? f : last;
            vv[t] = *(const f32x4_t*)(vb + f * INNER + 4 * c);
        }
        // next tile's k rows (used only in the next call)
        int nf = 16 * (ft + FSTEP) + c;
        nf = nf < nv ? nf : last;
        load_quarter_row(kb + nf * INNER + 16 * g, nxt);
        // all eight loads of the tile are issued HERE, a whole product ahead of their first use
        __builtin_amdgcn_sched_barrier(0);
        float ss = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) ss = fmaf(cur[s], cur[s], ss);
        // two independent accumulator chains (even / odd k-steps), summed afterwards
        f32x4_t S = ft == n_ft - 1 ? c_last : c_full;
        f32x4_t S2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 16; s += 2) {
            S = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[s], pb[s], S, 0, 0, 0);
            S2 = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[s + 1], pb[s + 1], S2, 0, 0, 0);
        }
        S2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ss, NEG_HALF, S2, 0, 0, 0);
        S += S2;
        f32x4_t kf;
#pragma unroll
        for (int r = 0; r < 4; ++r) kf[r] = __builtin_amdgcn_exp2f(S[r]);   // row 4g+r = frame within the tile
        ksum4 += kf;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int et = 0; et < 4; ++et)
                acc[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[t], vv[t][et], acc[et], 0, 0, 0);
    };
    float ka[16], kc[16];
    {
        const int f0 = 16 * ft_first + c;
        load_quarter_row(kb + (f0 < nv ? f0 : last) * INNER + 16 * g, ka);
    }
#pragma unroll 1
    for (int ft = ft_first; ft < n_ft; ft += 2 * FSTEP) {
        tile(ft, ka, kc);
        if (ft + FSTEP < n_ft) tile(ft + FSTEP, kc, ka);
    }
    if constexpr (PART) {
        // waves 1..3 hand their partial sums to wave 0 (added in wave order: the result does not depend on timing)
        const int wave = threadIdx.x >> 6;
        if (wave > 0) {
            f32x4_t* dst = (f32x4_t*)part + ((wave - 1) * 5) * 64 + lane;
#pragma unroll
            for (int et = 0; et < 4; ++et) dst[et * 64] = acc[et];
            dst[4 * 64] = ksum4;
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const f32x4_t* src = (const f32x4_t*)part + (w * 5) * 64 + lane;
#pragma unroll
            for (int et = 0; et < 4; ++et) acc[et] += src[et * 64];
            ksum4 += src[4 * 64];
        }
    }
    float* kr = ks + (int64_t)bh * KST;
    const float ksum = group_sum((ksum4[0] + ksum4[1]) + (ksum4[2] + ksum4[3]));
    if (g == 0) kr[j] = ksum;                                    // pad features 266..271 are exact zeros
    float ktot = ksum;                                           // sum over this tile's 16 features (lanes c)
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) ktot += __shfl_xor(ktot, m, 64);
    if (lane == 0) kr[OFF_KPART + jt] = ktot;
    // acc[et][r] = ctx[feature 16jt + 4g + r][channel 4c + et]  ->  ctxT[channel][feature], 4 features per store
    float* cd = ctxT + (int64_t)bh * DH * LDJ + 16 * jt + 4 * g;
#pragma unroll
    for (int et = 0; et < 4; ++et) {
        *(f32x4_t*)(cd + (int64_t)(4 * c + et) * LDJ) = acc[et];
        // this tile's share of the column sums of ctx (the Q kernel's eps term)
        const float part = group_sum((acc[et][0] + acc[et][1]) + (acc[et][2] + acc[et][3]));
        if (g == 0) kr[OFF_CPART + jt * DH + 4 * c + et] = part;
    }
}

__global__ void __launch_bounds__(256, 4) performer_kv_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                              const float* __restrict__ P, int Fr,
                                                              float* __restrict__ ctxT, float* __restrict__ ks,
                                                              const int* __restrict__ n_frames) {
    // 1-D grid, XCD-aware: workgroups id and id+8 share an XCD (and its L2), so all feature tiles of one
    // (utterance, head) - which re-read the same k and v rows - are dealt to ONE XCD (id & 7)
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int grp = slot % KV_GROUPS, bh = (slot / KV_GROUPS) * 8 + xcd;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jt = 4 * grp + wave;
    if (jt >= NJT) return;
    performer_kv_item<false>(k, v, P, Fr, n_frames, ctxT, ks, bh, jt);
}

// one (utterance, head, feature tile) per workgroup, its frame tiles over the four waves (few work items: see PART above)
__global__ void __launch_bounds__(256, 4) performer_kv_split_kernel(const float* __restrict__ k, const float* __restrict__ v,
                                                                    const float* __restrict__ P, int Fr,
                                                                    float* __restrict__ ctxT, float* __restrict__ ks,
                                                                    const int* __restrict__ n_frames) {
    __shared__ float part[3 * 5 * 64 * 4];
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int jt = slot % NJT, bh = (slot / NJT) * 8 + xcd;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    performer_kv_item<true>(k, v, P, Fr, n_frames, ctxT, ks, bh, jt, wave, part);
}

// PART = false: one wavefront walks all 17 feature tiles of its frame tile and stores the result.
// PART = true (few work items: the real-time block, strong-scaled shards): the wavefront walks the feature tiles jt0 .. jt1-1
// only and leaves (row maximum, D, out^T) relative to ITS maximum in `part` - the four waves of a workgroup share one frame
// tile and are combined at their common maximum by performer_q_split_kernel.
template <bool PART>
__device__ __forceinline__ void performer_q_item(const float* __restrict__ q, const float* __restrict__ P,
                                                 const float* __restrict__ ctxT, const float* __restrict__ ks, int Fr,
                                                 float* __restrict__ attn, int bh, int ft, int jt0 = 0, int jt1 = NJT,
                                                 float* __restrict__ part = nullptr) {
    const int b = bh / H, h = bh % H;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int frame = 16 * ft + c;              // this lane's frame (column of S^T and of out^T)
    float qb[16];
    load_quarter_row(q + ((int64_t)b * Fr + (frame < Fr ? frame : Fr - 1)) * INNER + h * DH + 16 * g, qb);
    float ss = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) ss = fmaf(qb[s], qb[s], ss);
#pragma unroll
    for (int s = 0; s < 16; ++s) qb[s] *= PSCALE;
    // (the row maximum runs over the projections WITHOUT the diagonal term, ddsp/pcmer.py:73: diag stays a separate
    // per-frame constant of the exponent, it does not cancel against the maximum)
    const float diag2 = -NEG_HALF * group_sum(ss);
    const float* kr = ks + (int64_t)bh * KST;
    const float* cd = ctxT + (int64_t)bh * DH * LDJ;
    const int coff = c * LDJ + 4 * g;
    // eps terms: column sums of ctx (lane = channel) and sum of ks, from the parts the K kernel left per feature tile
    float cs_lane = 0.f, ks_tot = lane < NJT ? kr[OFF_KPART + lane] : 0.f;
#pragma unroll
    for (int t = 0; t < NJT; ++t) cs_lane += kr[OFF_CPART + t * DH + lane];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) ks_tot += __shfl_xor(ks_tot, m, 64);

    // The feature tiles are consumed one at a time with a running row maximum (the softmax-kernel stabiliser of
    // ddsp/pcmer.py:69-77 is the maximum over ALL 266 features): when a tile raises the maximum of a frame, what
    // that frame has accumulated so far is rescaled by exp(old - new).  The eps term of q' = r*(exp(.) + eps) does
    // not scale, so it is carried as eps * (column sums of ctx) and eps * sum(ks) and added at the end.
    float m_run = -3.0e38f;
    f32x4_t Dacc = {0.f, 0.f, 0.f, 0.f};
    f32x4_t o[4];
#pragma unroll
    for (int et = 0; et < 4; ++et) o[et] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    f32x4_t c_last;                              // C init of the last feature tile: features 266..271 switched off
#pragma unroll
    for (int r = 0; r < 4; ++r) c_last[r] = 16 * (NJT - 1) + 4 * g + r < NF ? 0.f : MASKED;
    float pa[16];
    {
        int j0 = 16 * jt0 + c;
        j0 = j0 < NF ? j0 : NF - 1;
        load_quarter_row(P + j0 * DH + 16 * g, pa);
    }
#pragma unroll 2
    for (int jt = jt0; jt < jt1; ++jt) {
        // operands of this tile's second product (features 16jt + 4g + t): in flight under the first product
        f32x4_t ca[4];
#pragma unroll
        for (int et = 0; et < 4; ++et) ca[et] = *(const f32x4_t*)(cd + 16 * jt + (coff + 16 * et * LDJ));
        const f32x4_t kv = *(const f32x4_t*)(kr + 16 * jt + 4 * g);
        float pn[16];
        int jn = 16 * (jt + 1) + c;
        jn = jn < NF ? jn : NF - 1;
        load_quarter_row(P + jn * DH + 16 * g, pn);
        __builtin_amdgcn_sched_barrier(0);           // loads first, see the K kernel
        f32x4_t S = jt == NJT - 1 ? c_last : f32x4_t{0.f, 0.f, 0.f, 0.f};
        f32x4_t S2 = {0.f, 0.f, 0.f, 0.f};           // (two independent chains, see the K kernel)
#pragma unroll
        for (int s = 0; s < 16; s += 2) {
            S = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s], qb[s], S, 0, 0, 0);
            S2 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[s + 1], qb[s + 1], S2, 0, 0, 0);
        }
        S += S2;
        const float tmax = group_max(fmaxf(fmaxf(S[0], S[1]), fmaxf(S[2], S[3])));
        const float m_new = fmaxf(m_run, tmax);
        const float sc = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        const float dm = m_run + diag2;
        Dacc *= sc;
#pragma unroll
        for (int et = 0; et < 4; ++et) o[et] *= sc;
        f32x4_t u;
#pragma unroll
        for (int r = 0; r < 4; ++r) u[r] = __builtin_amdgcn_exp2f(S[r] - dm);
        Dacc += u * kv;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int et = 0; et < 4; ++et)
                o[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[et][t], u[t], o[et], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 16; ++s) pa[s] = pn[s];
    }
    if constexpr (PART) {
        // [21][64] floats per wave: m | D partial sums (4) | out^T (16), lane-major rows
        part[lane] = m_run;
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(1 + r) * 64 + lane] = Dacc[r];
#pragma unroll
        for (int et = 0; et < 4; ++et)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[(5 + 4 * et + r) * 64 + lane] = o[et][r];
        return;
    }
    const float Dsum = group_sum((Dacc[0] + Dacc[1]) + (Dacc[2] + Dacc[3]));
    const float D = RATIO * fmaf(EPS, ks_tot, Dsum);
    const float dinv = RATIO / (D + 1e-8f);
    // o[et][r] = out^T[channel 16et + 4g + r][frame c]
    float* orow = attn + ((int64_t)b * Fr + frame) * INNER + h * DH + 4 * g;
    const float cs_eps = EPS * cs_lane;
#pragma unroll
    for (int et = 0; et < 4; ++et) {
        f32x4_t res;
#pragma unroll
        for (int r = 0; r < 4; ++r) res[r] = (o[et][r] + __shfl(cs_eps, 16 * et + 4 * g + r, 64)) * dinv;
        if (frame < Fr) *(f32x4_t*)(orow + 16 * et) = res;
    }
}

__global__ void __launch_bounds__(256, 4) performer_q_kernel(const float* __restrict__ q, const float* __restrict__ P,
                                                             const float* __restrict__ ctxT, const float* __restrict__ ks,
                                                             int Fr, int n_grp, float* __restrict__ attn) {
    // XCD-aware 1-D grid (see performer_kv_kernel): the frame tiles of one (utterance, head) share ctx / ks / P
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int grp = slot % n_grp, bh = (slot / n_grp) * 8 + xcd;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ft = 4 * grp + wave;
    if (16 * ft >= Fr) return;
    performer_q_item<false>(q, P, ctxT, ks, Fr, attn, bh, ft);
}

// Few work items (B * 8 * ceil(Fr / 16) <= 1024: the real-time block has 48, a strong-scaled shard of 8 clips 704): one
// wavefront per frame tile walks 17 feature tiles one after the other and the launch is a single 15 us dependency chain
// (round 2: 3 x 15.6 us of the 0.39 ms real-time block).  Here the four waves of a workgroup share ONE frame tile and take 5 / 4
// / 4 / 4 feature tiles each; their partial results meet in the LDS at the common row maximum (the exact maximum over all 266
// features, as the eps term of the reference's softmax_kernel needs it), and wave w finishes channel block w.
__global__ void __launch_bounds__(256, 4) performer_q_split_kernel(const float* __restrict__ q, const float* __restrict__ P,
                                                                   const float* __restrict__ ctxT, const float* __restrict__ ks,
                                                                   int Fr, int n_ft, float* __restrict__ attn) {
    __shared__ float part[4][21 * 64];
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int ft = slot % n_ft, bh = (slot / n_ft) * 8 + xcd;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jt0 = wave == 0 ? 0 : 1 + 4 * wave, jt1 = 5 + 4 * wave;      // 0..5 | 5..9 | 9..13 | 13..17
    performer_q_item<true>(q, P, ctxT, ks, Fr, attn, bh, ft, jt0, jt1, part[wave]);
    __syncthreads();
    const int b = bh / H, h = bh % H;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int frame = 16 * ft + c;
    float m = part[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = fmaxf(m, part[w][lane]);
    float Dl = 0.f;
    f32x4_t o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float sc = __builtin_amdgcn_exp2f(part[w][lane] - m);
        float dw = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dw += part[w][(1 + r) * 64 + lane];
            o[r] = fmaf(part[w][(5 + 4 * wave + r) * 64 + lane], sc, o[r]);      // channel block et = wave
        }
        Dl = fmaf(dw, sc, Dl);
    }
    const float* kr = ks + (int64_t)bh * KST;
    float cs_lane = 0.f, ks_tot = lane < NJT ? kr[OFF_KPART + lane] : 0.f;
#pragma unroll
    for (int t = 0; t < NJT; ++t) cs_lane += kr[OFF_CPART + t * DH + lane];
#pragma unroll
    for (int mm = 1; mm < 64; mm <<= 1) ks_tot += __shfl_xor(ks_tot, mm, 64);
    const float Dsum = group_sum(Dl);
    const float D = RATIO * fmaf(EPS, ks_tot, Dsum);
    const float dinv = RATIO / (D + 1e-8f);
    const float cs_eps = EPS * cs_lane;
    f32x4_t res;
#pragma unroll
    for (int r = 0; r < 4; ++r) res[r] = (o[r] + __shfl(cs_eps, 16 * wave + 4 * g + r, 64)) * dinv;
    if (frame < Fr) *(f32x4_t*)(attn + ((int64_t)b * Fr + frame) * INNER + h * DH + 4 * g + 16 * wave) = res;
}

// ---- causal linear attention in chunks (ddsp/pcmer.py:170-188, `c: true`; round 3) ---------------------------------------------
// out_n = q'_n . S_n / (q'_n . (z_n + 1e-6)),  S_n = sum_{m<=n} k'_m (x) v_m,  z_n = sum_{m<=n} k'_m.  `fast_transformers.CausalDotProduct`
// (the numerator) is a third-party CUDA extension that is not in the image: restated from its definition; the normaliser is the
// reference's own code.  For a chunk of 16 frames:   out = [ Q' S_prev + tril(Q' K'^T) V ] / [ Q' (z_prev + 1e-6) + rowsum(tril(Q' K'^T)) ],
// then S_prev += K'^T V, z_prev += colsum(K').  One workgroup (4 wavefronts) owns one (utterance, head) and walks its chunks;
// every product runs on v_mfma_f32_16x16x4_f32:
//   F  feature maps: wave w takes the 16-feature tiles w, w + 4, ... (its rows of dn*log2(e)*P stay in registers for the whole
//      launch): dash = x P^T for x = q and k (frames x features), k' finished at once into the LDS, q' after the row maximum
//      has been exchanged through the LDS;
//   A  (K' Q'^T), kframes x qframes, the feature range cut over the four waves, partial tiles through the LDS;
//   O  wave w owns channels 16w .. 16w + 15 of the output: out^T = V^T tril(A) (the summed, masked tile IS the operand: its
//      accumulator layout has lane = qframe, register = kframe) + S^T Q'^T (S lives in this wave's accumulators, 17 tiles of
//      16 features x 16 channels, and an accumulator register is again the k-slot the product wants); the denominators on the
//      vector ALU from the same Q' registers;
//   S  S += K'^T V for the wave's channels, z += column sums.
// Nothing but q, k, v is read and the attention output written (the sequential kernel below read q', k' - 190 MB a layer - that a
// GEMM and a row kernel had written).  All arithmetic fp32.
constexpr int CC = 16;                  // frames per chunk
constexpr int CPF = LDJ + 4;            // pitch of a q' / k' row in the LDS: 16-byte reads of 16 consecutive rows hit 16 different bank quads
constexpr int CPD = DH + 4;             // pitch of a q / k / v row
typedef float f32x4c __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0)

__global__ void __launch_bounds__(256, 2) performer_causal_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ v, const float* __restrict__ P, int Fr,
                                                                  float* __restrict__ out) {
    constexpr int MAXT = (NJT + 3) / 4;   // 5 feature tiles per wave at most
    __shared__ float qs[CC * CPD], ks_[CC * CPD], vs[CC * CPD], Qf[CC * CPF], Kf[CC * CPF], ATp[4 * 256], z[LDJ], diagq[CC], diagk[CC],
        pmax[4 * CC];
    const int bh = blockIdx.x, b = bh / H, h = bh % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, kq = lane >> 4;
    // this wave's rows of the scaled projection matrix: tile c <-> features 16 (w + 4 c) + n, elements 16 kq .. 16 kq + 15
    float pf[MAXT][16];
#pragma unroll
    for (int c = 0; c < MAXT; ++c) {
        const int j = 16 * (w + 4 * c) + n;
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
            f32x4c x = {0.f, 0.f, 0.f, 0.f};
            if (j < NF) x = *(const f32x4c*)(P + (int64_t)j * DH + 16 * kq + 4 * e4);
#pragma unroll
            for (int e = 0; e < 4; ++e) pf[c][4 * e4 + e] = PSCALE * x[e];
        }
    }
    f32x4c S[NJT];                         // S[t][r] = S_state[feature 16 t + 4 kq + r][channel 16 w + n]
#pragma unroll
    for (int t = 0; t < NJT; ++t) S[t] = f32x4c{0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < LDJ; i += 256) z[i] = 0.f;

    // chunk staging: thread <-> 4 consecutive channels of one frame, for each of q, k, v
    const int sf = tid >> 4, sc = 4 * (tid & 15);
    const float* base = q + ((int64_t)b * Fr) * INNER + h * DH + sc;
    const int64_t koff = k - q, voff = v - q;
    f32x4c rq, rk, rv;
    auto fetch = [&](int f0) {
        const int f = f0 + sf;
        rq = rk = rv = f32x4c{0.f, 0.f, 0.f, 0.f};
        if (f < Fr) {
            const float* src = base + (int64_t)f * INNER;
            rq = *(const f32x4c*)src;
            rk = *(const f32x4c*)(src + koff);
            rv = *(const f32x4c*)(src + voff);
        }
    };
    auto row_sum16 = [&](float x) {       // over the 16 lanes that share a frame
        x += __shfl_xor(x, 1, 64);
        x += __shfl_xor(x, 2, 64);
        x += __shfl_xor(x, 4, 64);
        x += __shfl_xor(x, 8, 64);
        return x;
    };
    auto stage = [&]() {
        *(f32x4c*)(qs + sf * CPD + sc) = rq;
        *(f32x4c*)(ks_ + sf * CPD + sc) = rk;
        *(f32x4c*)(vs + sf * CPD + sc) = rv;
        const float dq = row_sum16(rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3]);
        const float dk = row_sum16(rk[0] * rk[0] + rk[1] * rk[1] + rk[2] * rk[2] + rk[3] * rk[3]);
        if ((tid & 15) == 0) {
            diagq[sf] = NEG_HALF * dq;    // -0.5 dn^2 |x|^2 in the base-2 domain
            diagk[sf] = NEG_HALF * dk;
        }
    };
    fetch(0);
    stage();
    __syncthreads();

    for (int f0 = 0; f0 < Fr; f0 += CC) {
        if (f0 + CC < Fr) fetch(f0 + CC);
        // ---- F: dash = x P^T on the wave's feature tiles; k' finished, q' waits for the row maximum ----
        float qa[16], ka[16];
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
            const f32x4c a = *(const f32x4c*)(qs + n * CPD + 16 * kq + 4 * e4), c = *(const f32x4c*)(ks_ + n * CPD + 16 * kq + 4 * e4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                qa[4 * e4 + e] = a[e];
                ka[4 * e4 + e] = c[e];
            }
        }
        const f32x4c dgk = *(const f32x4c*)(diagk + 4 * kq), dgq = *(const f32x4c*)(diagq + 4 * kq);
        f32x4c dq[MAXT];
        f32x4c mx = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
#pragma unroll
        for (int c = 0; c < MAXT; ++c) {
            const int t = w + 4 * c;
            if (t < NJT) {
                f32x4c dk = {0.f, 0.f, 0.f, 0.f};
                dq[c] = f32x4c{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    dq[c] = MFMA16(qa[s], pf[c][s], dq[c]);
                    dk = MFMA16(ka[s], pf[c][s], dk);
                }
                const bool feat_ok = 16 * t + n < NF;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = feat_ok && f0 + 4 * kq + r < Fr;
                    Kf[(4 * kq + r) * CPF + 16 * t + n] = ok ? __builtin_amdgcn_exp2f(dk[r] + dgk[r] + KOFF) : 0.f;
                    if (feat_ok) mx[r] = fmaxf(mx[r], dq[c][r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = mx[r];
            m = fmaxf(m, __shfl_xor(m, 1, 64));
            m = fmaxf(m, __shfl_xor(m, 2, 64));
            m = fmaxf(m, __shfl_xor(m, 4, 64));
            m = fmaxf(m, __shfl_xor(m, 8, 64));
            mx[r] = m;
        }
        if (n == 0) *(f32x4c*)(pmax + w * CC + 4 * kq) = mx;
        __syncthreads();
        {
            const f32x4c m0 = *(const f32x4c*)(pmax + 4 * kq), m1 = *(const f32x4c*)(pmax + CC + 4 * kq),
                         m2 = *(const f32x4c*)(pmax + 2 * CC + 4 * kq), m3 = *(const f32x4c*)(pmax + 3 * CC + 4 * kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) mx[r] = dgq[r] - fmaxf(fmaxf(m0[r], m1[r]), fmaxf(m2[r], m3[r]));
        }
#pragma unroll
        for (int c = 0; c < MAXT; ++c) {
            const int t = w + 4 * c;
            if (t < NJT) {
                const bool feat_ok = 16 * t + n < NF;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Qf[(4 * kq + r) * CPF + 16 * t + n] = feat_ok ? RATIO * (__builtin_amdgcn_exp2f(dq[c][r] + mx[r]) + EPS) : 0.f;
            }
        }
        __syncthreads();
        // ---- A: this wave's share (68 features) of K' Q'^T ----
        {
            f32x4c at = {0.f, 0.f, 0.f, 0.f};
            const float* kr = Kf + n * CPF + 68 * w + kq;
            const float* qr = Qf + n * CPF + 68 * w + kq;
#pragma unroll
            for (int j = 0; j < 17; ++j) at = MFMA16(kr[4 * j], qr[4 * j], at);
            *(f32x4c*)(ATp + w * 256 + lane * 4) = at;
        }
        __syncthreads();
        // ---- O: out^T for channels 16 w .. 16 w + 15 ----
        f32x4c o = {0.f, 0.f, 0.f, 0.f};
        float den = 0.f;
        {
            f32x4c at = *(const f32x4c*)(ATp + lane * 4);
#pragma unroll
            for (int ww = 1; ww < 4; ++ww) at += *(const f32x4c*)(ATp + ww * 256 + lane * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                at[r] = 4 * kq + r <= n ? at[r] : 0.f;      // kframe <= qframe
                den += at[r];
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) o = MFMA16(vs[(4 * kq + s) * CPD + 16 * w + n], at[s], o);
        }
#pragma unroll
        for (int t = 0; t < NJT; ++t) {
            const f32x4c qv = *(const f32x4c*)(Qf + n * CPF + 16 * t + 4 * kq);
            const f32x4c zv = *(const f32x4c*)(z + 16 * t + 4 * kq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o = MFMA16(S[t][r], qv[r], o);
                den = fmaf(qv[r], zv[r] + 1e-6f, den);
            }
        }
        den += __shfl_xor(den, 16, 64);
        den += __shfl_xor(den, 32, 64);
        if (f0 + n < Fr) {
            const float inv = 1.0f / den;
            *(f32x4c*)(out + ((int64_t)b * Fr + f0 + n) * INNER + h * DH + 16 * w + 4 * kq) = o * inv;
        }
        __syncthreads();               // every wave is done with z (and with q', whose buffer the next chunk rewrites)
        // ---- S: state update for this wave's channels ----
        {
            float vb[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) vb[s] = vs[(4 * s + kq) * CPD + 16 * w + n];
#pragma unroll
            for (int t = 0; t < NJT; ++t)
#pragma unroll
                for (int s = 0; s < 4; ++s) S[t] = MFMA16(Kf[(4 * s + kq) * CPF + 16 * t + n], vb[s], S[t]);
            for (int i = tid; i < LDJ; i += 256) {
                float a = 0.f;
#pragma unroll
                for (int f = 0; f < CC; ++f) a += Kf[f * CPF + i];
                z[i] += a;
            }
        }
        __syncthreads();               // k', v of this chunk are dead
        if (f0 + CC < Fr) stage();
        __syncthreads();
    }
}

}  // namespace

// (utterance, head) pairs up to which the frame tiles of an item are dealt over four waves
constexpr int KV_SPLIT_MAX = 128;
// work items up to which the feature range is split over four waves
constexpr int Q_SPLIT_MAX = 1024;

void performer_kv(hipStream_t st, const float* k, const float* v, const float* P, int B, int Fr, float* ctxT, float* ks,
                  const int* n_frames) {
    if (B * H <= KV_SPLIT_MAX) {
        hipLaunchKernelGGL(performer_kv_split_kernel, dim3((unsigned)(NJT * B * H)), dim3(256), 0, st, k, v, P, Fr, ctxT, ks, n_frames);
        return;
    }
    // B*H is a multiple of 8, so the XCD-aware decode of the 1-D grid covers every (head, tile group) exactly once
    hipLaunchKernelGGL(performer_kv_kernel, dim3((unsigned)(KV_GROUPS * B * H)), dim3(256), 0, st, k, v, P, Fr, ctxT, ks, n_frames);
}

void performer_q(hipStream_t st, const float* q, const float* P, const float* ctxT, const float* ks, int B, int Fr,
                 float* attn) {
    const int n_grp = ((Fr + 15) / 16 + 3) / 4;
    const int n_ft = (Fr + 15) / 16;
    if ((int64_t)n_ft * B * H <= Q_SPLIT_MAX) {
        hipLaunchKernelGGL(performer_q_split_kernel, dim3((unsigned)(n_ft * B * H)), dim3(256), 0, st, q, P, ctxT, ks, Fr, n_ft, attn);
        return;
    }
    hipLaunchKernelGGL(performer_q_kernel, dim3((unsigned)(n_grp * B * H)), dim3(256), 0, st, q, P, ctxT, ks, Fr, n_grp, attn);
}

// chunked causal attention (inference): attn (B*Fr, 512) from q, k, v (B*Fr, 512) and P (266, 64)
void performer_causal(hipStream_t st, const float* q, const float* k, const float* v, const float* P, int B, int Fr, float* attn) {
    hipLaunchKernelGGL(performer_causal_kernel, dim3((unsigned)(B * H)), dim3(256), 0, st, q, k, v, P, Fr, attn);
}
