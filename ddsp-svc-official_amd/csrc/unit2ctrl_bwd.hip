// a4: backward pass of the unit -> control network (unit2ctrl_fwd.hip has the forward, u2c.h what both share): the
// row-wise adjoints, the causal attention scans, the fused feature-map adjoint of the attention, the column sums and
// split-K reductions of the parameter gradients, and the pass driver.  It starts from the activations a
// ddsp_unit2ctrl_fwd_keep call left, or re-runs the forward with its activations in the scratch arena.
#include "gemm_f32.h"
#include "wgrad_bf16.h"
#include "u2c.h"

using namespace u2c;

namespace {

// ---- backward of the causal attention (training of `c: true` networks; correct first, one frame per step) ------------------
// With S_n = sum_{m<=n} k'_m (x) v_m, z_n = sum_{m<=n} k'_m, den_n = q'_n.(z_n + 1e-6), out_n = q'_n S_n / den_n and the upstream
// d_n = dL/d out_n:   dnum_n = d_n / den_n,   dden_n = -(d_n . out_n) / den_n,
//   dq'_n = S_n dnum_n + dden_n (z_n + 1e-6)                              (forward scan, pass Q)
//   dk'_n = G_n v_n + g_n,  dv_n = G_n^T k'_n   with G_n = sum_{m>=n} q'_m (x) dnum_m,  g_n = sum_{m>=n} dden_m q'_m   (reverse scans, passes K and V)
// Passes Q and K: 320 threads, thread j owns row j of the 266 x 64 state (64 registers), so the products with a 64-vector
// are in-thread; pass V uses the forward kernel's layout (thread (e, r0) owns column e of rows r0 + 4 i), in which the
// product with a 266-vector is in-thread.  Pass Q also leaves 1/den_n and dden_n for the other two.
__global__ void __launch_bounds__(320) causal_attn_bwd_q_kernel(const float* __restrict__ qf, const float* __restrict__ kf,
                                                                const float* __restrict__ v, const float* __restrict__ dout,
                                                                const float* __restrict__ out, int Fr, float* __restrict__ dqf,
                                                                float* __restrict__ dinv_out, float* __restrict__ dden_out) {
    __shared__ float sv[2][DH], sd[2][DH], so[2][DH], red[2][8];
    const int bh = blockIdx.x, b = bh / H, h = bh % H;
    const int t = threadIdx.x;
    const bool active = t < NF;
    float S[DH];
#pragma unroll
    for (int e = 0; e < DH; ++e) S[e] = 0.f;
    float z = 0.f;
    for (int n = 0; n < Fr; ++n) {
        const int buf = n & 1;
        const int64_t row = (int64_t)b * Fr + n, row8 = row * H + h;
        if (t < DH) {
            sv[buf][t] = v[row * INNER + h * DH + t];
            sd[buf][t] = dout[row * INNER + h * DH + t];
            so[buf][t] = out[row * INNER + h * DH + t];
        }
        const float qj = active ? qf[row8 * LDF + t] : 0.f, kj = active ? kf[row8 * LDF + t] : 0.f;
        z += kj;
        const float dp = wave_sum(qj * (z + 1e-6f));
        if ((t & 63) == 0) red[buf][t >> 6] = dp;
        __syncthreads();
        const float den = ((red[buf][0] + red[buf][1]) + (red[buf][2] + red[buf][3])) + red[buf][4];
        const float dinv = 1.0f / den;
        float c = 0.f, acc = 0.f;
#pragma unroll
        for (int e = 0; e < DH; ++e) {
            c = fmaf(sd[buf][e], so[buf][e], c);
            S[e] = fmaf(kj, sv[buf][e], S[e]);
            acc = fmaf(S[e], sd[buf][e], acc);
        }
        const float dden = -c * dinv;
        if (active) dqf[row8 * LDF + t] = fmaf(dden, z + 1e-6f, acc * dinv);
        if (t == 0) {
            dinv_out[row8] = dinv;
            dden_out[row8] = dden;
        }
    }
}

__global__ void __launch_bounds__(320) causal_attn_bwd_k_kernel(const float* __restrict__ qf, const float* __restrict__ v,
                                                                const float* __restrict__ dout, const float* __restrict__ dinv_in,
                                                                const float* __restrict__ dden_in, int Fr,
                                                                float* __restrict__ dkf) {
    __shared__ float sv[2][DH], sd[2][DH];
    const int bh = blockIdx.x, b = bh / H, h = bh % H;
    const int t = threadIdx.x;
    const bool active = t < NF;
    float G[DH];
#pragma unroll
    for (int e = 0; e < DH; ++e) G[e] = 0.f;
    float g = 0.f;
    for (int n = Fr - 1; n >= 0; --n) {
        const int buf = n & 1;
        const int64_t row = (int64_t)b * Fr + n, row8 = row * H + h;
        const float di = dinv_in[row8], dd = dden_in[row8];
        if (t < DH) {
            sv[buf][t] = v[row * INNER + h * DH + t];
            sd[buf][t] = dout[row * INNER + h * DH + t] * di;   // dnum
        }
        const float qj = active ? qf[row8 * LDF + t] : 0.f;
        g = fmaf(dd, qj, g);
        __syncthreads();
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < DH; ++e) {
            G[e] = fmaf(qj, sd[buf][e], G[e]);
            acc = fmaf(G[e], sv[buf][e], acc);
        }
        if (active) dkf[row8 * LDF + t] = acc + g;
    }
}

__global__ void __launch_bounds__(256) causal_attn_bwd_v_kernel(const float* __restrict__ qf, const float* __restrict__ kf,
                                                                const float* __restrict__ dout, const float* __restrict__ dinv_in,
                                                                int Fr, float* __restrict__ dv) {
    constexpr int ROWS = (NF + 3) / 4;       // 67
    __shared__ float sq[LDF], sk[LDF], sdn[DH], part[4 * DH];
    const int bh = blockIdx.x, b = bh / H, h = bh % H;
    const int t = threadIdx.x, e = t & 63, r0 = t >> 6;
    float G[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) G[i] = 0.f;
    for (int n = Fr - 1; n >= 0; --n) {
        const int64_t row = (int64_t)b * Fr + n, row8 = row * H + h;
        for (int j = t; j < LDF; j += 256) {
            sq[j] = qf[row8 * LDF + j];
            sk[j] = kf[row8 * LDF + j];
        }
        if (t < DH) sdn[t] = dout[row * INNER + h * DH + t] * dinv_in[row8];
        __syncthreads();
        const float dne = sdn[e];
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int j = r0 + 4 * i;
            if (j < NF) {
                G[i] = fmaf(sq[j], dne, G[i]);
                acc = fmaf(sk[j], G[i], acc);
            }
        }
        part[r0 * DH + e] = acc;
        __syncthreads();
        if (t < DH) dv[row * INNER + h * DH + t] = (part[t] + part[DH + t]) + (part[2 * DH + t] + part[3 * DH + t]);
    }
}

// LayerNorm backward, one wave per row: dx = rstd*(dy*g - mean(dy*g) - xhat*mean(dy*g*xhat)) (+ res);
// gx = dy*xhat is written for the column reduction that yields d gamma.
__global__ void __launch_bounds__(256) layernorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ dy, const float* __restrict__ res,
                                                            int64_t rows, float* __restrict__ dx,
                                                            float* __restrict__ gx) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;
    const f32x4 v = *(const f32x4*)(x + m * D + lane * 4);
    const f32x4 g = *(const f32x4*)(dy + m * D + lane * 4);
    const f32x4 ga = *(const f32x4*)(gamma + lane * 4);
    const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / D);
    f32x4 xh, dg;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        xh[j] = v[j] - mean;
        ss = fmaf(xh[j], xh[j], ss);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) * (1.0f / D) + 1e-5f);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        xh[j] *= rstd;
        dg[j] = g[j] * ga[j];
        s1 += dg[j];
        s2 = fmaf(dg[j], xh[j], s2);
    }
    s1 = wave_sum(s1) * (1.0f / D);
    s2 = wave_sum(s2) * (1.0f / D);
    f32x4 o, gxo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = rstd * (dg[j] - s1 - xh[j] * s2);
        gxo[j] = g[j] * xh[j];
    }
    if (res) o += *(const f32x4*)(res + m * D + lane * 4);
    *(f32x4*)(dx + m * D + lane * 4) = o;
    *(f32x4*)(gx + m * D + lane * 4) = gxo;
}

// Column sums over rows, optionally weighted per row: out_partial[chunk][c] = sum_{r in chunk} X[r][c] * w(r).
// wmode: 0 none, 1 w = wsrc[r], 2 w = ln(1 + wsrc[r]/700), 3 w = wsrc[r]/pi     (the three side embeddings)
constexpr int CS_CHUNKS = 128;
// one column per lane, four row lanes per block: the variant for widths that are not a multiple of 4 (the odd-width heads)
// or matrices that are not 16-byte aligned; colsum_multi_kernel below does the others
__global__ void __launch_bounds__(256) colsum_partial_kernel(const float* __restrict__ X, int64_t ld, int64_t rows,
                                                             int cols, const float* __restrict__ wsrc, int wmode,
                                                             float* __restrict__ partial) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rl = threadIdx.x >> 6;
    const int64_t per = (rows + CS_CHUNKS - 1) / CS_CHUNKS;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    int64_t r1 = r0 + per;
    if (r1 > rows) r1 = rows;
    float s = 0.f;
    if (c < cols) {
        for (int64_t r = r0 + rl; r < r1; r += 4) {
            float w = 1.0f;
            if (wmode == 1) w = wsrc[r];
            else if (wmode == 2) w = logf(1.0f + __fdiv_rn(wsrc[r], 700.0f));
            else if (wmode == 3) w = __fdiv_rn(wsrc[r], 3.14159274101257324f);
            s = fmaf(X[r * ld + c], w, s);
        }
    }
    __shared__ float red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0 && c < cols)
        partial[(int64_t)blockIdx.y * cols + c] = (red[threadIdx.x] + red[threadIdx.x + 64]) +
                                                  (red[threadIdx.x + 128] + red[threadIdx.x + 192]);
}

// Up to four column sums that share their shape in ONE pass (blockIdx.z = job): the two LayerNorm / GroupNorm parameter
// gradients (sums of gx and of dA), the three side-embedding weights and their bias (the same dX under four row weights),
// or a single one.  16 bytes per lane (4 columns), four row lanes per block, two independent accumulators per lane, for
// 16-byte-aligned matrices whose width is a multiple of 4.  (Round 2: the scalar kernel above ran at 0.9 TB/s, 13 us for
// an 11 MB matrix, 54 launches per training step.)
struct ColsumJobs {
    const float* X[4];
    const float* wsrc[4];
    int wmode[4];
    float* out[4];
    int n;
};
__global__ void __launch_bounds__(256) colsum_multi_kernel(ColsumJobs jb, int64_t ld, int64_t rows, int cols,
                                                           float* __restrict__ partial) {
    const int job = blockIdx.z;
    const float* __restrict__ X = jb.X[job];
    const float* __restrict__ wsrc = jb.wsrc[job];
    const int wmode = jb.wmode[job];
    const int c = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int rl = threadIdx.x >> 6;
    const int64_t per = (rows + CS_CHUNKS - 1) / CS_CHUNKS;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    int64_t r1 = r0 + per;
    if (r1 > rows) r1 = rows;
    auto weight = [&](int64_t r) -> float {
        if (wmode == 1) return wsrc[r];
        if (wmode == 2) return logf(1.0f + __fdiv_rn(wsrc[r], 700.0f));
        if (wmode == 3) return __fdiv_rn(wsrc[r], 3.14159274101257324f);
        return 1.0f;
    };
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    if (c < cols) {
        int64_t r = r0 + rl;
        for (; r + 4 < r1; r += 8) {
            const f32x4 a = *(const f32x4*)(X + r * ld + c), b = *(const f32x4*)(X + (r + 4) * ld + c);
            const float wa = weight(r), wb = weight(r + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s0[j] = fmaf(a[j], wa, s0[j]);
                s1[j] = fmaf(b[j], wb, s1[j]);
            }
        }
        if (r < r1) {
            const f32x4 a = *(const f32x4*)(X + r * ld + c);
            const float wa = weight(r);
#pragma unroll
            for (int j = 0; j < 4; ++j) s0[j] = fmaf(a[j], wa, s0[j]);
        }
    }
    __shared__ f32x4 red[256];
    red[threadIdx.x] = s0 + s1;
    __syncthreads();
    if (rl == 0 && c < cols)
        *(f32x4*)(partial + ((int64_t)job * CS_CHUNKS + blockIdx.y) * cols + c) =
            (red[threadIdx.x] + red[threadIdx.x + 64]) + (red[threadIdx.x + 128] + red[threadIdx.x + 192]);
}
// the matching reduction: blockIdx.y = job, partial[job][chunk][cols] -> jb.out[job][cols]
__global__ void __launch_bounds__(256) reduce_multi_kernel(const float* __restrict__ partial, ColsumJobs jb, int cols) {
    const int job = blockIdx.y;
    const int i = blockIdx.x * 64 + (threadIdx.x & 63), zl = threadIdx.x >> 6;
    const float* p = partial + (int64_t)job * CS_CHUNKS * cols;
    float s0 = 0.f, s1 = 0.f;
    if (i < cols) {
#pragma unroll 4
        for (int z = zl; z < CS_CHUNKS; z += 8) {
            s0 += p[(int64_t)z * cols + i];
            s1 += p[(int64_t)(z + 4) * cols + i];
        }
    }
    __shared__ float red[256];
    red[threadIdx.x] = s0 + s1;
    __syncthreads();
    if (zl == 0 && i < cols)
        jb.out[job][i] = (red[threadIdx.x] + red[threadIdx.x + 64]) + (red[threadIdx.x + 128] + red[threadIdx.x + 192]);
}

// out[i] = sum_{z < nz} partial[z][i]  (also the split-K reduction of the weight-gradient GEMMs)
// block = 64 elements x 4 z-lanes (launch with 256 threads, ceil(n / 64) blocks): a thread adds every fourth partial in
// two chains, the lanes meet in the LDS.  (One thread per element walked 128 partials alone: 10.5 us per call, 47 calls
// per training step.)
__global__ void __launch_bounds__(256) reduce_partials_kernel(const float* __restrict__ partial, int nz, int64_t n,
                                                              float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const int zl = threadIdx.x >> 6;
    float s0 = 0.f, s1 = 0.f;
    if (i < n) {
        int z = zl;
        for (; z + 4 < nz; z += 8) {
            s0 += partial[(int64_t)z * n + i];
            s1 += partial[(int64_t)(z + 4) * n + i];
        }
        if (z < nz) s0 += partial[(int64_t)z * n + i];
    }
    __shared__ float red[256];
    red[threadIdx.x] = s0 + s1;
    __syncthreads();
    if (zl == 0 && i < n)
        out[i] = (red[threadIdx.x] + red[threadIdx.x + 64]) + (red[threadIdx.x + 128] + red[threadIdx.x + 192]);
}

__global__ void __launch_bounds__(256) silu_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ dout,
                                                       int64_t n, float* __restrict__ dpre) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = pre[i], sg = 1.0f / (1.0f + expf(-p));
        dpre[i] = dout[i] * (sg * (1.0f + p * (1.0f - sg)));
    }
}

// GLU backward: g1 = [a | g] (rows x 1024), out = a*sigmoid(g): d_a = d*s, d_g = d*a*s*(1-s)
__global__ void __launch_bounds__(256) glu_bwd_kernel(const float* __restrict__ g1, const float* __restrict__ dglu,
                                                      int64_t rows, float* __restrict__ dg1) {
    const int64_t total = rows * INNER;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / INNER;
        const int c = (int)(i % INNER);
        const float a = g1[m * 2 * INNER + c], g = g1[m * 2 * INNER + INNER + c], d = dglu[i];
        const float sg = 1.0f / (1.0f + expf(-g));
        dg1[m * 2 * INNER + c] = d * sg;
        dg1[m * 2 * INNER + INNER + c] = d * a * sg * (1.0f - sg);
    }
}

// depthwise-conv weight gradient dW[c][t] = sum_{b, f} dpre[b,f,c] * x[b, f+t-left, c] with the forward kernel's register window:
// one thread owns one channel for a run of DW_RUN frames, its DW_RUN upstream gradients and DW_RUN + 30 inputs stay in
// registers and every tap is a 32-long dot product of them (round 3; the round-2 kernel re-read 8 inputs per multiply-add
// batch through the L1 and took 79 us per layer at B = 32, memory-instruction bound).  partial[(b, run)][tap][channel]: coalesced 256-byte rows per tap; dw_wgrad_reduce_kernel sums the runs and
// transposes to the parameter's (512, 1, 31) layout.
__global__ void __launch_bounds__(256) dwconv_wgrad_run_kernel(const float* __restrict__ dpre, const float* __restrict__ x,
                                                               int B, int Fr, float* __restrict__ partial, int left,
                                                               const int* __restrict__ n_frames = nullptr) {   // ragged batch: input frames >= n_b read as 0, as the forward read them
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int runs = (Fr + DW_RUN - 1) / DW_RUN;
    const int b = blockIdx.y / runs, f0 = (blockIdx.y % runs) * DW_RUN;
    const float* dp = dpre + ((int64_t)b * Fr) * INNER + c;
    const float* xp = x + ((int64_t)b * Fr) * INNER + c;
    const int n_in = ddsp_row_frames(n_frames, b, Fr);
    float d[DW_RUN], win[DW_RUN + DWK - 1];
#pragma unroll
    for (int o = 0; o < DW_RUN; ++o) d[o] = f0 + o < Fr ? dp[(int64_t)(f0 + o) * INNER] : 0.f;
#pragma unroll
    for (int i = 0; i < DW_RUN + DWK - 1; ++i) {
        const int f = f0 + i - left;
        win[i] = (f >= 0 && f < n_in) ? xp[(int64_t)f * INNER] : 0.f;
    }
    float* out = partial + ((int64_t)blockIdx.y * DWK) * INNER + c;
#pragma unroll
    for (int t = 0; t < DWK; ++t) {
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int o = 0; o < DW_RUN; o += 2) {
            a0 = fmaf(d[o], win[o + t], a0);
            a1 = fmaf(d[o + 1], win[o + 1 + t], a1);
        }
        out[(int64_t)t * INNER] = a0 + a1;
    }
}
// dW[c][t] = sum_p partial[p][t][c]; block = 64 channels x 4 partial lanes
__global__ void __launch_bounds__(256) dw_wgrad_reduce_kernel(const float* __restrict__ partial, int np, float* __restrict__ dW) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), t = blockIdx.y, zl = threadIdx.x >> 6;
    float s0 = 0.f;
    for (int z = zl; z < np; z += 4) s0 += partial[((int64_t)z * DWK + t) * INNER + c];
    __shared__ float red[256];
    red[threadIdx.x] = s0;
    __syncthreads();
    if (zl == 0) dW[c * DWK + t] = (red[threadIdx.x] + red[threadIdx.x + 64]) + (red[threadIdx.x + 128] + red[threadIdx.x + 192]);
}

// attention output adjoint, one wave per (frame, head) row: out = num * dinv  ->  d_num = d_out*dinv (in place),
// d_D = -(d_out . out) * dinv
__global__ void __launch_bounds__(256) attn_out_bwd_kernel(float* __restrict__ d_attn, const float* __restrict__ attn,
                                                           const float* __restrict__ dinv, int64_t rows8,
                                                           float* __restrict__ dD) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows8) return;
    const int64_t off = (r / H) * INNER + (r % H) * DH + lane;
    const float d = d_attn[off], o = attn[off], di = dinv[r];
    const float dot = wave_sum(d * o);
    d_attn[off] = d * di;
    if (lane == 0) dD[r] = -dot * di;
}

// d_ks[b,h,j] = sum_n q'[b,n,h,j] * d_D[b,n,h]   (block layout of key_sum_kernel)
__global__ void __launch_bounds__(KS_T * 8) weighted_key_sum_kernel(const float* __restrict__ qf, const float* __restrict__ dD,
                                                                    int Fr, float* __restrict__ dks) {
    const int bh = blockIdx.x, b = bh / H, h = bh % H;
    const int j4 = threadIdx.x % KS_T, fl = threadIdx.x / KS_T;
    const int64_t r0 = ((int64_t)b * Fr) * H + h;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    int n = fl;
    for (; n + 8 < Fr; n += 16) {
        const f32x4 a = *(const f32x4*)(qf + (r0 + (int64_t)n * H) * LDF + 4 * j4);
        const f32x4 c = *(const f32x4*)(qf + (r0 + (int64_t)(n + 8) * H) * LDF + 4 * j4);
        const float wa = dD[r0 + (int64_t)n * H], wc = dD[r0 + (int64_t)(n + 8) * H];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s0[e] = fmaf(a[e], wa, s0[e]);
            s1[e] = fmaf(c[e], wc, s1[e]);
        }
    }
    if (n < Fr) {
        const f32x4 a = *(const f32x4*)(qf + (r0 + (int64_t)n * H) * LDF + 4 * j4);
        const float wa = dD[r0 + (int64_t)n * H];
#pragma unroll
        for (int e = 0; e < 4; ++e) s0[e] = fmaf(a[e], wa, s0[e]);
    }
    __shared__ f32x4 red[KS_T * 8];
    red[threadIdx.x] = s0 + s1;
    __syncthreads();
    if (fl == 0) {
        f32x4 t = red[j4];
#pragma unroll
        for (int i = 1; i < 8; ++i) t += red[i * KS_T + j4];
        *(f32x4*)(dks + (int64_t)bh * LDF + 4 * j4) = t;
    }
}

// feature-map adjoint, in place on d_feat: d_feat <- dn * d(dd);  coef[r] = -dn^2 * sum_j d_feat_j * E_j
// key:   feat_j = r*exp(dd_j - diag + eps)            E_j = feat_j
// query: feat_j = r*(exp(dd_j - diag - max) + eps)    E_j = feat_j - r*eps, and the max-subtraction routes -sum to argmax
template <bool QUERY>
__global__ void __launch_bounds__(256) feature_map_bwd_kernel(const float* __restrict__ feat, float* __restrict__ dfeat,
                                                              int64_t rows8, float* __restrict__ coef) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows8) return;
    const float dn = 0.35355339059327373f, ratio = 0.06131393394849658f;
    const float* f = feat + r * LDF;
    float* d = dfeat + r * LDF;
    float dd[5], fv[5];
    float t = 0.f, best = -3.0e38f;
    int arg = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int j = lane + 64 * i;
        dd[i] = 0.f;
        fv[i] = 0.f;
        if (j < NF) {
            fv[i] = f[j];
            const float E = QUERY ? fv[i] - ratio * 1e-4f : fv[i];
            dd[i] = d[j] * E;
            t += dd[i];
            if (QUERY && (fv[i] > best)) {
                best = fv[i];
                arg = j;
            }
        }
    }
    t = wave_sum(t);
    if (QUERY) {
        // first index of the row maximum (torch.max returns one arg max; ties are measure-zero for real data)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(arg, o, 64);
            if (ob > best || (ob == best && oa < arg)) {
                best = ob;
                arg = oa;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int j = lane + 64 * i;
        if (j < NF) {
            float v = dd[i];
            if (QUERY && j == arg) v -= t;
            d[j] = dn * v;
        } else if (j < LDF) {
            d[j] = 0.f;
        }
    }
    if (lane == 0) coef[r] = -(dn * dn) * t;
}

struct EpiRowOuter {  // out[(b*Fr+m)*8+h][j] = acc + rowscale[row] * colvec[(b*8+h)][j]   (z = b*8+h); rowscale null -> 1
    float* out;
    const float* rowscale;
    const float* colvec;
    int Fr;
    __device__ __forceinline__ float col(int) const { return 0.f; }
    __device__ __forceinline__ void operator()(int z, int m, int j, float v, float) const {
        const int b = z / H, h = z % H;
        const int64_t row = ((int64_t)b * Fr + m) * H + h;
        const float rs = rowscale ? rowscale[row] : 1.0f;
        out[row * LDF + j] = fmaf(rs, colvec[(int64_t)z * LDF + j], v);
    }
};

struct EpiAxpyRow {  // C[r][d] = acc + coef[r] * src[r][d]
    float* C;
    const float* coef;
    const float* src;
    int ld;
    __device__ __forceinline__ float col(int) const { return 0.f; }
    __device__ __forceinline__ void operator()(int, int m, int n, float v, float) const {
        const int64_t o = (int64_t)m * ld + n;
        C[o] = fmaf(coef[m], src[o], v);
    }
};

struct EpiAccumulate {  // C += acc
    float* C;
    int64_t ldc;
    __device__ __forceinline__ float col(int) const { return 0.f; }
    __device__ __forceinline__ void operator()(int, int m, int n, float v, float) const { C[(int64_t)m * ldc + n] += v; }
    static constexpr bool kStore4 = true;
    __device__ __forceinline__ bool vec_ok() const { return ((uintptr_t)C % 16) == 0 && ldc % 4 == 0; }
    __device__ __forceinline__ void store4(int, int m, int n, f32x4 v) const {
        f32x4* p = (f32x4*)(C + (int64_t)m * ldc + n);
        *p = *p + v;
    }
};

// GroupNorm(4) + LeakyReLU backward.  Pass 1 (per utterance, group): s1 = sum dy*g, s2 = sum dy*g*xhat over 64 ch x Fr.
__global__ void __launch_bounds__(256) groupnorm_bwd_stats_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  const float* __restrict__ dy, const float* __restrict__ stats,
                                                                  const float* __restrict__ gamma, int Fr,
                                                                  float* __restrict__ bstats,
                                                                  const int* __restrict__ n_frames = nullptr) {   // ragged batch: the row's own frames
    const int g = blockIdx.x, b = blockIdx.y;
    const int c = threadIdx.x & 63, fl = threadIdx.x >> 6;
    const int ch = g * 64 + c;
    const float mean = stats[(b * 4 + g) * 2], rstd = stats[(b * 4 + g) * 2 + 1];
    const float ga = gamma[ch];
    const int nv = ddsp_row_frames(n_frames, b, Fr);
    double s1 = 0.0, s2 = 0.0;
    for (int f = fl; f < nv; f += 4) {
        const int64_t i = ((int64_t)b * Fr + f) * D + ch;
        const float slope = y[i] > 0.f ? 1.0f : 0.01f;   // y = lrelu(gn(x)); sign(y) = sign(gn(x))
        const float dgn = dy[i] * slope;
        const float xh = (x[i] - mean) * rstd;
        s1 += (double)(dgn * ga);
        s2 += (double)(dgn * ga * xh);
    }
    s1 = wave_sum_d(s1);
    s2 = wave_sum_d(s2);
    __shared__ double red[8];
    if ((threadIdx.x & 63) == 0) {
        red[fl] = s1;
        red[4 + fl] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = 64.0 * nv;
        bstats[(b * 4 + g) * 2 + 0] = (float)((red[0] + red[1] + red[2] + red[3]) / n);
        bstats[(b * 4 + g) * 2 + 1] = (float)((red[4] + red[5] + red[6] + red[7]) / n);
    }
}

// Pass 2: dx = rstd*(dgn*gamma - m1 - xhat*m2);  also gxh = dgn*xhat and dgn itself (for d gamma / d beta column sums)
__global__ void __launch_bounds__(256) groupnorm_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                  const float* __restrict__ dy, const float* __restrict__ stats,
                                                                  const float* __restrict__ bstats,
                                                                  const float* __restrict__ gamma, int64_t rows, int Fr,
                                                                  float* __restrict__ dx, float* __restrict__ gxh,
                                                                  float* __restrict__ dgn_out,
                                                                  const int* __restrict__ n_frames = nullptr) {   // ragged batch: 0 past a row's own frames
    const int64_t total = rows * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / D;
        const int ch = (int)(i % D);
        const int b = (int)(m / Fr), g = ch >> 6;
        if (n_frames && (int)(m % Fr) >= ddsp_row_frames(n_frames, b, Fr)) {   // (d_t2 there is the conv adjoint's spill: not read)
            dx[i] = 0.f;
            gxh[i] = 0.f;
            dgn_out[i] = 0.f;
            continue;
        }
        const float mean = stats[(b * 4 + g) * 2], rstd = stats[(b * 4 + g) * 2 + 1];
        const float m1 = bstats[(b * 4 + g) * 2], m2 = bstats[(b * 4 + g) * 2 + 1];
        const float slope = y[i] > 0.f ? 1.0f : 0.01f;
        const float dgn = dy[i] * slope;
        const float xh = (x[i] - mean) * rstd;
        dx[i] = rstd * (dgn * gamma[ch] - m1 - xh * m2);
        gxh[i] = dgn * xh;
        dgn_out[i] = dgn;
    }
}

// shifted copy over the frame axis with zero fill at utterance edges: out[b,f,:] = x[b,f+shift,:]
__global__ void __launch_bounds__(256) shift_rows_kernel(const float* __restrict__ x, int64_t rows, int Fr, int C, int shift,
                                                         float* __restrict__ out) {
    const int64_t total = rows * (C / 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / (C / 4);
        const int c4 = (int)(i % (C / 4)) * 4;
        const int f = (int)(m % Fr) + shift;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (f >= 0 && f < Fr) v = *(const f32x4*)(x + (m + shift) * C + c4);
        *(f32x4*)(out + m * C + c4) = v;
    }
}

// packed (Cout, 3, Cin) gradient -> torch layout (Cout, Cin, 3)
__global__ void unpack_conv3_kernel(const float* __restrict__ packed, int Cout, int Cin, float* __restrict__ out) {
    const int64_t total = (int64_t)Cout * Cin * 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int tap = (int)(i % 3);
        const int c = (int)((i / 3) % Cin);
        const int o = (int)(i / (3 * Cin));
        out[i] = packed[(int64_t)o * 3 * Cin + (int64_t)tap * Cin + c];
    }
}

// conv weight (Cout, Cin, 3) -> transposed-conv operand (Cin, 3*Cout): out[c][tap*Cout + o] = w[o][c][2 - tap]
__global__ void pack_conv3_transposed_kernel(const float* __restrict__ w, int Cout, int Cin, float* __restrict__ out) {
    const int64_t total = (int64_t)Cout * Cin * 3;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int tap = (int)(i % 3);
        const int c = (int)((i / 3) % Cin);
        const int o = (int)(i / (3 * Cin));
        out[(int64_t)c * 3 * Cout + (int64_t)(2 - tap) * Cout + o] = w[i];
    }
}

// weight-norm backward, one wave per output row: W = g*v/|v|  ->  d_g = (dW . v)/|v|,  d_v = g/|v| * (dW - (dW.vhat) vhat)
__global__ void __launch_bounds__(256) weight_norm_bwd_kernel(const float* __restrict__ g, const float* __restrict__ v,
                                                              const float* __restrict__ dW, int n_out, int n_in,
                                                              float* __restrict__ dg, float* __restrict__ dv) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n_out) return;
    const float* vr = v + (int64_t)o * n_in;
    const float* dr = dW + (int64_t)o * n_in;
    float ss = 0.f, dot = 0.f;
    for (int i = lane; i < n_in; i += 64) {
        ss = fmaf(vr[i], vr[i], ss);
        dot = fmaf(dr[i], vr[i], dot);
    }
    ss = wave_sum(ss);
    dot = wave_sum(dot);
    const float nrm = sqrtf(ss);
    if (lane == 0) dg[o] = dot / nrm;
    const float s = g[o] / nrm, proj = dot / ss;
    for (int i = lane; i < n_in; i += 64) dv[(int64_t)o * n_in + i] = s * (dr[i] - proj * vr[i]);
}

// Gradient of the speaker table, deterministic (no float atomics: the training trajectory is chaotic enough without a
// run-to-run difference in the last bit).  Pass 1: usum[b][c] = sum_f dx[b,f,c], one block per utterance, 64 lanes x 16
// bytes across the channels, 16 frame lanes; it also reports an id outside [1, n_spk] (the row is then skipped, like the
// forward's table read).  Pass 2: one block per table row adds the utterances that use it in ascending order.
__global__ void __launch_bounds__(1024) utterance_sum_kernel(const float* __restrict__ dx, int Fr,
                                                             const int64_t* __restrict__ spk_id, int64_t n_spk_id, int n_spk,
                                                             float* __restrict__ usum, int* __restrict__ err) {
    const int64_t b = blockIdx.x;
    const int c4 = threadIdx.x & 63, fl = threadIdx.x >> 6;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int f = fl; f < Fr; f += 16) s += *(const f32x4*)(dx + ((int64_t)b * Fr + f) * D + 4 * c4);
    __shared__ f32x4 red[1024];
    red[threadIdx.x] = s;
    __syncthreads();
    if (fl == 0) {
        f32x4 t = red[c4];
#pragma unroll
        for (int i = 1; i < 16; ++i) t += red[64 * i + c4];
        *(f32x4*)(usum + b * D + 4 * c4) = t;
    }
    if (threadIdx.x == 0 && spk_id) {
        const int64_t id = spk_id[n_spk_id == 1 ? 0 : b];
        if (id < 1 || id > n_spk) __hip_atomic_store(err, DDSP_DEV_ERR_SPK_ID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
__global__ void __launch_bounds__(256) spk_table_grad_kernel(const float* __restrict__ usum, int64_t B,
                                                             const int64_t* __restrict__ spk_id, int64_t n_spk_id,
                                                             MixArgs mix, float* __restrict__ dtable) {
    const int r = blockIdx.x, c = threadIdx.x;  // D == 256 channels
    float s = 0.f;
    if (mix.n > 0) {
        float cr = 0.f;
        for (int k = 0; k < mix.n; ++k)
            if (mix.ids[k] - 1 == r) cr += mix.w[k];
        if (cr != 0.f) {
            for (int64_t b = 0; b < B; ++b) s += usum[b * D + c];
            s *= cr;
        }
    } else if (n_spk_id == 1) {
        if (spk_id[0] - 1 == r)
            for (int64_t b = 0; b < B; ++b) s += usum[b * D + c];
    } else {
        for (int64_t b = 0; b < B; ++b)
            if (spk_id[b] - 1 == r) s += usum[b * D + c];
    }
    dtable[(int64_t)r * D + c] = s;
}

// ---- helpers of the backward pass ------------------------------------------------------------------------------
// Split-K reductions of the weight gradients: dst[o*ldo + c] = sum_{z < nz} src[z][o][c], z ascending from 0.f.  Deferred
// (round 3): the 18 Linear layers of the three blocks write their split partial sums (and those of their bias column sums) into
// regions of their own and ONE launch at the end of the backward pass adds them all up - 36 launches of 5-6 us fewer per
// training step.  The other weight gradients reduce at once, a table of one job (reduce_now).
constexpr int WG_SPLITS = 16;   // row splits of a weight-gradient product (buffers and the reduction's register array are sized for it)
constexpr int RED_JOBS_MAX = 48;
struct RedJobs {
    int n;
    const float* src[RED_JOBS_MAX];
    float* dst[RED_JOBS_MAX];
    int nz[RED_JOBS_MAX], O[RED_JOBS_MAX], C[RED_JOBS_MAX];
    int ldo[RED_JOBS_MAX];
    int bend[RED_JOBS_MAX];   // exclusive end of the job's range of workgroups
    bool push(const float* src_, float* dst_, int nz_, int O_, int C_, int64_t ldo_) {
        if (n >= RED_JOBS_MAX) return false;
        const int j = n++;
        src[j] = src_;
        dst[j] = dst_;
        nz[j] = nz_;
        O[j] = O_;
        C[j] = C_;
        ldo[j] = (int)ldo_;
        int64_t blocks = ((int64_t)O_ * C_ + 1023) / 1024;       // four outputs per thread
        if (blocks > 256) blocks = 256;
        if (blocks < 1) blocks = 1;
        bend[j] = (j ? bend[j - 1] : 0) + (int)blocks;
        return true;
    }
};
__global__ void __launch_bounds__(256) reduce_jobs_kernel(RedJobs J) {
    int j = 0;
    while (j + 1 < J.n && (int)blockIdx.x >= J.bend[j]) ++j;
    const int b0 = j ? J.bend[j - 1] : 0, nb = J.bend[j] - b0;
    const float* __restrict__ partial = J.src[j];
    float* __restrict__ out = J.dst[j];
    const int nz = J.nz[j], C = J.C[j];
    const int64_t n = (int64_t)J.O[j] * C, ldo = J.ldo[j];
    if (nz <= WG_SPLITS + 1 && ((n | C | ldo) & 3) == 0 && (((uintptr_t)partial | (uintptr_t)out) & 15) == 0) {
        // four outputs per thread and every split's load in flight before the first addition (same z-ascending order of the sums)
        for (int64_t i = ((int64_t)((int)blockIdx.x - b0) * 256 + threadIdx.x) * 4; i < n; i += (int64_t)nb * 1024) {
            f32x4 v[WG_SPLITS + 1];
#pragma unroll
            for (int z = 0; z < WG_SPLITS + 1; ++z)
                if (z < nz) v[z] = *(const f32x4*)(partial + (int64_t)z * n + i);
            f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int z = 0; z < WG_SPLITS + 1; ++z)
                if (z < nz) s4 += v[z];
            *(f32x4*)(out + (i / C) * ldo + (i % C)) = s4;
        }
        return;
    }
    for (int64_t i = (int64_t)((int)blockIdx.x - b0) * 256 + threadIdx.x; i < n; i += (int64_t)nb * 256) {
        float s = 0.f;
        for (int z = 0; z < nz; ++z) s += partial[(int64_t)z * n + i];
        out[(i / C) * ldo + (i % C)] = s;
    }
}
static void reduce_jobs(hipStream_t st, const RedJobs& J) {
    if (J.n) hipLaunchKernelGGL(reduce_jobs_kernel, dim3((unsigned)J.bend[J.n - 1]), dim3(256), 0, st, J);
}
// one reduction now (nz <= WG_SPLITS on every path: the split row count is ceil(M / chunk) with chunk >= M / WG_SPLITS, so the
// kernel takes its vector path for aligned widths)
static void reduce_now(hipStream_t st, const float* src, float* dst, int nz, int O, int C, int64_t ldo) {
    RedJobs J{};
    J.push(src, dst, nz, O, C, ldo);
    reduce_jobs(st, J);
}
struct WgDefer {
    RedJobs jobs;
    float* pool;
    size_t used, cap;   // floats
    float* take(size_t n) {
        n = (n + 63) & ~(size_t)63;
        if (used + n > cap) return nullptr;
        float* p = pool + used;
        used += n;
        return p;
    }
};
static void flush_deferred(hipStream_t st, WgDefer& df) {
    reduce_jobs(st, df.jobs);
    df.jobs.n = 0;
    df.used = 0;
}

// out[o*ldo + coff + c] = sum_m dY[m][o] * X[m][c]   (split-K batches on the matrix pipe + one reduction)
static int wgrad(ddsp_ctx* ctx, hipStream_t st, const float* dY, int64_t ldy, int O, const float* X, int64_t ldx, int C,
                 int64_t M, float* partial, float* out, int64_t ldo, int coff) {
    int64_t chunk = (M + WG_SPLITS - 1) / WG_SPLITS;
    chunk = (chunk + 31) & ~(int64_t)31;
    const int nfull = (int)(M / chunk);
    const int64_t tail = M - (int64_t)nfull * chunk;
    ddsp_prof_begin(ctx, st, PF_U2C_BWD);
    if (nfull > 0) {
        gemm::Args g = gemm::make(dY, ldy, X, ldx, O, C, (int)chunk);
        g.sA_hi = chunk * ldy;
        g.sB_hi = chunk * ldx;
        gemm::EpiStore e{partial, C, nullptr, 1, (int64_t)O * C, 0};
        gemm::launch_tile<64, 64, false, false, gemm::A_PLAIN>(st, g, nfull, e);
    }
    if (tail > 0) {
        gemm::Args g = gemm::make(dY + (int64_t)nfull * chunk * ldy, ldy, X + (int64_t)nfull * chunk * ldx, ldx, O, C, (int)tail);
        gemm::EpiStore e{partial + (int64_t)nfull * O * C, C, nullptr, 1, 0, 0};
        gemm::launch_tile<64, 64, false, false, gemm::A_PLAIN>(st, g, 1, e);
    }
    reduce_now(st, partial, out + coff, nfull + (tail > 0 ? 1 : 0), O, C, ldo);
    ddsp_prof_end(ctx, st, 2.0 * M * O * (double)C, 4.0 * M * (O + C));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// the launch pair of column sums of one shape (partial holds jb.n x CS_CHUNKS x cols); reduce_multi_kernel adds the chunks in
// the order of reduce_partials_kernel with nz = CS_CHUNKS
static void colsum_jobs(hipStream_t st, const ColsumJobs& jb, int64_t ld, int64_t rows, int cols, float* partial) {
    hipLaunchKernelGGL(colsum_multi_kernel, dim3((cols + 255) / 256, CS_CHUNKS, jb.n), dim3(256), 0, st, jb, ld, rows, cols, partial);
    hipLaunchKernelGGL(reduce_multi_kernel, dim3((cols + 63) / 64, jb.n), dim3(256), 0, st, partial, jb, cols);
}

// out[c] = sum_r X[r][c] * w(r)
static int colsum(ddsp_ctx* ctx, hipStream_t st, const float* X, int64_t ld, int64_t rows, int cols, const float* wsrc,
                  int wmode, float* partial, float* out) {
    if (cols % 4 == 0 && ld % 4 == 0 && ((uintptr_t)X % 16) == 0 && ((uintptr_t)partial % 16) == 0) {
        ColsumJobs jb{};
        jb.n = 1;
        jb.X[0] = X;
        jb.wsrc[0] = wsrc;
        jb.wmode[0] = wmode;
        jb.out[0] = out;
        colsum_jobs(st, jb, ld, rows, cols, partial);
    } else {
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((cols + 63) / 64, CS_CHUNKS), dim3(256), 0, st, X, ld, rows, cols, wsrc,
                           wmode, partial);
        hipLaunchKernelGGL(reduce_partials_kernel, dim3((cols + 63) / 64), dim3(256), 0, st, partial, CS_CHUNKS, (int64_t)cols, out);
    }
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// several column sums of one shape in one pass (cols % 4 == 0, 16-byte aligned rows; cpart holds 4 x CS_CHUNKS x cols)
static int colsum_multi(ddsp_ctx* ctx, hipStream_t st, const ColsumJobs& jb, int64_t ld, int64_t rows, int cols, float* partial) {
    bool vec = cols % 4 == 0 && ld % 4 == 0 && ((uintptr_t)partial % 16) == 0 && (size_t)jb.n * cols <= 2048;
    for (int i = 0; i < jb.n; ++i) vec = vec && ((uintptr_t)jb.X[i] % 16) == 0;
    if (!vec) {
        for (int i = 0; i < jb.n; ++i)
            if (int rc = colsum(ctx, st, jb.X[i], ld, rows, cols, jb.wsrc[i], jb.wmode[i], partial, jb.out[i])) return rc;
        return DDSP_OK;
    }
    colsum_jobs(st, jb, ld, rows, cols, partial);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
static int colsum_pair(ddsp_ctx* ctx, hipStream_t st, const float* X0, const float* X1, int64_t ld, int64_t rows, int cols,
                       float* partial, float* out0, float* out1) {
    ColsumJobs jb{};
    jb.n = 2;
    jb.X[0] = X0;
    jb.X[1] = X1;
    jb.out[0] = out0;
    jb.out[1] = out1;
    return colsum_multi(ctx, st, jb, ld, rows, cols, partial);
}

// Weight and bias gradient of one Linear (taps = 1) or Conv1d k=3 (taps = 3, X = the layer's input, out = the packed
// (O, 3*C) matrix) from the same dY.  With split-bf16 products (the context's default arithmetic) one launch of the
// transposing bf16 kernel (wgrad_bf16.h) produces the split partials of both and two small kernels add them; with
// ddsp_ctx_set_math(FP32) the round-1 path runs: fp32-MFMA split-K batches, shifted copies of X per tap, a separate column sum.
static int layer_grads(ddsp_ctx* ctx, hipStream_t st, const float* dY, int64_t ldy, int O, const float* X, int64_t ldx, int C,
                       int taps, int Fr, int64_t M, float* wpart, float* cpart, float* xs, float* w_out, int64_t ldo,
                       float* b_out, int tap_shift = 0, WgDefer* defer = nullptr) {   // tap_shift: 0 centred taps, -1 causal taps (taps == 3 only)
    int rc;
    const bool split = ctx->math == DDSP_MATH_SPLIT_BF16 && (taps == 1 || C % 128 == 0);
    if (!split) {
        if (taps == 1) {
            if ((rc = wgrad(ctx, st, dY, ldy, O, X, ldx, C, M, wpart, w_out, ldo, 0))) return rc;
        } else {
            for (int tap = 0; tap < taps; ++tap) {
                hipLaunchKernelGGL(shift_rows_kernel, dim3(grid_for(M * (C / 4))), dim3(256), 0, st, X, M, Fr, C, tap - 1 + tap_shift, xs);
                if ((rc = wgrad(ctx, st, dY, ldy, O, xs, C, C, M, wpart, w_out, ldo, tap * C))) return rc;
            }
        }
        if (b_out) return colsum(ctx, st, dY, ldy, M, O, nullptr, 0, cpart, b_out);
        return DDSP_OK;
    }
    wgrad::Args g;
    g.dY = dY;
    g.ldy = ldy;
    g.O = O;
    g.X = X;
    g.ldx = ldx;
    g.C = C;
    g.taps = taps;
    g.tap_shift = taps == 3 ? tap_shift : 0;
    g.Fr = Fr;
    g.M = M;
    g.chunk = wgrad::chunk_for(M, WG_SPLITS);
    const int nz = wgrad::splits_for(M, g.chunk), N = taps * C;
    // deferred: partial sums into regions of the caller's pool, added up by ONE launch at the end of the backward pass
    float* dpart = nullptr;
    float* dbias = nullptr;
    if (defer && defer->jobs.n + 2 <= RED_JOBS_MAX) {
        const size_t u0 = defer->used;
        dpart = defer->take((size_t)nz * O * N);
        dbias = b_out ? defer->take((size_t)nz * O) : nullptr;
        if (!dpart || (b_out && !dbias)) {
            defer->used = u0;
            dpart = dbias = nullptr;
        }
    }
    g.partial = dpart ? dpart : wpart;
    g.bias_partial = b_out ? (dpart ? dbias : cpart) : nullptr;
    ddsp_prof_begin(ctx, st, PF_U2C_BWD);
    // 64x64 tiles: with 16 splits every layer of the network gives 512-1280 workgroups; the larger tiles stage less per
    // product but leave CUs idle at these sizes (r02, training step B=32: 8.30 ms against 8.45 / 8.45 / 8.59 with 128x64 /
    // 64x128 / 128x128)
    wgrad::launch<1, 1>(st, g);
    if (dpart) {
        defer->jobs.push(dpart, w_out, nz, O, N, ldo);
        if (b_out) defer->jobs.push(dbias, b_out, nz, 1, O, O);
    } else {
        reduce_now(st, wpart, w_out, nz, O, N, ldo);
        if (b_out) hipLaunchKernelGGL(reduce_partials_kernel, dim3((O + 63) / 64), dim3(256), 0, st, cpart, nz, (int64_t)O, b_out);
    }
    ddsp_prof_end(ctx, st, 2.0 * M * O * (double)N, 4.0 * M * (O + C));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// dX[m][c] = sum_o dY[m][o] * W[o][c]   (W stored (O, C) like nn.Linear.weight), optionally accumulated into dX
// WT: the weight transposed to (C, O) in the pre-split operand layout (transpose_split_kernel), or null.  With it the
// product runs on the LDS-DMA kernel in split-bf16 arithmetic (dY split in the loop, W read split); without it on the
// register-staged fp32 kernel, which can read W as stored.
static void dgrad(hipStream_t st, const float* dY, int64_t ldy, const float* W, int O, int C, int64_t M, float* dX,
                  bool accumulate, const float* WT = nullptr) {
    if (WT) {
        gemm::Args g = gemm::make(dY, ldy, WT, O, (int)M, C, O);
        g.math = DDSP_MATH_SPLIT_BF16;
        g.B_split = WT;
        if (accumulate) {
            EpiAccumulate e{dX, C};
            gemm::launch<true, true, gemm::A_PLAIN>(st, g, 1, e);
        } else {
            gemm::EpiStore e{dX, C, nullptr, 1, 0, 0};
            gemm::launch<true, true, gemm::A_PLAIN>(st, g, 1, e);
        }
        return;
    }
    gemm::Args g = gemm::make(dY, ldy, W, C, (int)M, C, O);
    if (accumulate) {
        EpiAccumulate e{dX, C};
        gemm::launch<true, false, gemm::A_PLAIN>(st, g, 1, e);
    } else {
        gemm::EpiStore e{dX, C, nullptr, 1, 0, 0};
        gemm::launch<true, false, gemm::A_PLAIN>(st, g, 1, e);
    }
}

// Transposed, pre-split copies of the weights the input gradients multiply by: dst[c][o] (pitch O) in the (8 hi | 8 lo)
// group layout of gemm::Args::B_split.  One launch for all matrices of the network (blockIdx.y = matrix); a thread owns
// one (column c, group of 8 rows o) record, like the staging of wgrad_bf16.h.
constexpr int TS_MAX = 20;
struct TsArgs {
    const float* src[TS_MAX];
    float* dst[TS_MAX];
    int O[TS_MAX], C[TS_MAX];
};
__global__ void __launch_bounds__(256) transpose_split_kernel(TsArgs t) {
    const int mi = blockIdx.y;
    const float* __restrict__ src = t.src[mi];
    float* __restrict__ dst = t.dst[mi];
    const int O = t.O[mi], C = t.C[mi];
    const int tiles_c = C / 64, tiles = tiles_c * (O / 32);
    const int c_in = threadIdx.x & 63, og = threadIdx.x >> 6;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int c = (tile % tiles_c) * 64 + c_in, o = (tile / tiles_c) * 32 + og * 8;
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = src[(int64_t)(o + j) * C + c];
        ddsp_u32x4 hi, lo;
        ddsp_split8(x, hi, lo);
        ddsp_u32x4* p = reinterpret_cast<ddsp_u32x4*>(dst + (int64_t)c * O + o);
        p[0] = hi;
        p[1] = lo;
    }
}

// the backward pass; `keep` = the activation region a ddsp_unit2ctrl_fwd_keep call filled (then nothing is recomputed), or
// null: the forward is re-run here with its activations in the scratch arena
// Ragged batch (in.n_frames): d_ctrl is 0 on every row's padding frames, and the pass keeps the gradient of EVERY activation
// exactly 0 there.  The row-wise adjoints do so by themselves (a zero gradient row times a finite kept activation), so do the
// sums over frames of a weight gradient, of d_ctx / d_ks and of the causal scans (they add zeros).  What needs the counts are
// the places where the forward read the padding as 0 or summed over a row's own frames: the depthwise convolution (its input
// gradient is 0 there, its weight gradient reads 0 there), d_k and d_v of the attention (the context's gradient reaches every
// frame), the GroupNorm statistics and d_t1 (conv2's adjoint spills one frame past the row; t2 itself was written as 0 there).
static int u2c_backward(ddsp_ctx* ctx, hipStream_t st, const ddsp_u2c_weights& w, const ddsp_u2c_weights& gr, const U2CInputs& in,
                        int64_t B, int64_t Fr, const float* d_ctrl, float* ctrl_out, void* keep, size_t keep_bytes) {
    int rc;
#define G(p) const_cast<float*>(gr.p)
    const int64_t M = B * Fr, M8 = M * H;
    const int NO = w.n_out;

    // ---- arena: kept forward activations + backward temporaries ----
    U2CBufs bf;
    float *ctrl = nullptr, *dX, *dA, *dB512, *dC512, *dV512, *dG1, *dQF, *dKF, *dcx, *dks, *dD, *coefq, *coefk, *gx, *wpart, *cpart,
        *dWh, *pk, *xs, *dwpart, *gbst, *w2t, *wts, *wpool, *ptp, *dcxt;
    // partial sums of the 18 Linear layers of the blocks, reduced by one launch at the end (WgDefer): 17 splits at most
    const size_t wpool_floats = (size_t)(WG_SPLITS + 1) * 3 * ((size_t)2 * D * INNER + (size_t)2 * INNER * D + (size_t)3 * INNER * D + 2 * D + 2 * INNER + 3 * INNER + 1024);
    auto plan_bwd = [&](Arena& a) {
        if (!keep) {
            plan_forward(a, bf, w, B, Fr, true);
            ctrl = a.get((size_t)M * NO);
        }
        dX = a.get((size_t)M * D);          // gradient on the residual stream
        dA = a.get((size_t)M * D);          // second stream-sized temporary
        dB512 = a.get((size_t)M * INNER);   // d_dwo / d_pre / d_attn->d_num / d_q
        dC512 = a.get((size_t)M * INNER);   // d_glu / d_k
        dV512 = a.get((size_t)M * INNER);   // d_v
        dG1 = a.get((size_t)M * 2 * INNER);
        dQF = a.get((size_t)M8 * LDF);
        dKF = a.get((size_t)M8 * LDF);
        dcx = a.get((size_t)B * H * NF * DH);
        dks = a.get((size_t)B * H * LDF);
        dD = a.get((size_t)M8);
        coefq = a.get((size_t)M8);
        coefk = a.get((size_t)M8);
        gx = a.get((size_t)M * D);
        const size_t omax = (size_t)(NO > 2 * INNER ? NO : 2 * INNER);
        wpart = a.get((size_t)(WG_SPLITS + 1) * omax * (size_t)(w.n_unit > INNER ? w.n_unit : INNER));
        cpart = a.get((size_t)CS_CHUNKS * (omax > 2048 ? omax : 2048));
        dWh = a.get((size_t)NO * D);
        pk = a.get((size_t)D * 3 * (w.n_unit > D ? w.n_unit : D));
        xs = a.get((size_t)M * (w.n_unit > D ? w.n_unit : D));
        dwpart = a.get((size_t)B * ((Fr + DW_RUN - 1) / DW_RUN) * INNER * DWK);
        gbst = a.get((size_t)B * 4 * 2);
        w2t = a.get((size_t)D * 3 * D);
        wts = a.get((size_t)NO * D + 3 * ((size_t)2 * D * INNER + (size_t)2 * INNER * D + (size_t)3 * INNER * D));
        wpool = a.get(wpool_floats);
        ptp = a.get((size_t)3 * FB_PT_VEC * 4);   // prepared projections of attn_feat_bwd_kernel
        dcxt = a.get((size_t)B * H * FB_PT_VEC * 4);   // d_ctx^T of every (utterance, head) in the same layout
    };
    if (keep) {
        Arena k{ctx, false, 0, 0, (char*)keep, keep_bytes};
        plan_forward(k, bf, w, B, Fr, true);
        DDSP_REQUIRE(ctx, !k.rc, "ddsp_unit2ctrl_bwd_kept: the activation region is smaller than ddsp_unit2ctrl_keep_bytes says");
    }
    Arena dry{ctx, true, 0, 0};
    plan_bwd(dry);
    rc = ddsp_scratch_reserve_bytes(ctx, dry.total + 4096);
    if (rc) return rc;
    ddsp_scratch_reset(ctx);
    Arena a{ctx, false, 0, 0};
    plan_bwd(a);
    if (a.rc) return a.rc;

    if (!keep) {
        rc = u2c_forward(ctx, st, w, in, bf, ctrl);
        if (rc) return rc;
        if (ctrl_out) DDSP_HIP(ctx, hipMemcpyAsync(ctrl_out, ctrl, (size_t)M * NO * sizeof(float), hipMemcpyDeviceToDevice, st));
    }

    const unsigned rows_g = (unsigned)ceil_div64(M, 4), rows8_g = (unsigned)ceil_div64(M8, 4);
    // ---- transposed split copies of the weights for the input-gradient products (split-bf16 arithmetic only) ----
    const float *wt_head = nullptr, *wt_pw2[3] = {}, *wt_pw1[3] = {}, *wt_out[3] = {}, *wt_qkv[3][3] = {};
    if (ctx->math == DDSP_MATH_SPLIT_BF16) {
        TsArgs ts;
        int n = 0;
        float* next = wts;
        auto add = [&](const float* src, int O, int C) -> const float* {
            if (O % 32 != 0 || C % 64 != 0 || O < 256) return nullptr;   // (gemm::launch sends K >= 256 to the DMA kernel at every M)
            ts.src[n] = src;
            ts.dst[n] = next;
            ts.O[n] = O;
            ts.C[n] = C;
            ++n;
            next += (size_t)O * C;
            return next - (size_t)O * C;
        };
        wt_head = add(bf.wh, NO, D);
        for (int l = 0; l < 3; ++l) {
            wt_pw2[l] = add(w.layer[l].cm_pw2_w, D, INNER);
            wt_pw1[l] = add(w.layer[l].cm_pw1_w, 2 * INNER, D);
            wt_out[l] = add(w.layer[l].out_w, D, INNER);
            wt_qkv[l][0] = add(w.layer[l].q_w, INNER, D);
            wt_qkv[l][1] = add(w.layer[l].k_w, INNER, D);
            wt_qkv[l][2] = add(w.layer[l].v_w, INNER, D);
        }
        static_assert(TS_MAX >= 19, "table too small");
        hipLaunchKernelGGL(transpose_split_kernel, dim3(64, n), dim3(256), 0, st, ts);
    }
    // split-bf16, non-causal: the feature-map adjoints in attn_feat_bwd_kernel; fp32 and causal: the five-launch chain
    const bool feat_fused = ctx->math != DDSP_MATH_FP32 && !w.causal;
    if (feat_fused)
        for (int l = 0; l < 3; ++l) feat_proj_prep(st, w.layer[l].proj, 1, ptp + (size_t)l * FB_PT_VEC * 4);
    WgDefer df{};
    df.pool = wpool;
    df.cap = wpool_floats;
    WgDefer* const dfp = &df;
    // ---- head: ctrl = LN(x) W^T + b, W = g v/|v| ----
    if ((rc = layer_grads(ctx, st, d_ctrl, NO, NO, bf.y_final, D, D, 1, (int)Fr, M, wpart, cpart, xs, dWh, D, G(head_b)))) return rc;
    hipLaunchKernelGGL(weight_norm_bwd_kernel, dim3((NO + 3) / 4), dim3(256), 0, st, w.head_g, w.head_v, dWh, NO, D,
                       G(head_g), G(head_v));
    dgrad(st, d_ctrl, NO, bf.wh, NO, D, M, dA, false, wt_head);
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(rows_g), dim3(256), 0, st, bf.l[2].x_out, w.final_ln_w, dA, nullptr, M, dX, gx);
    if ((rc = colsum_pair(ctx, st, gx, dA, D, M, D, cpart, G(final_ln_w), G(final_ln_b)))) return rc;

    for (int l = 2; l >= 0; --l) {
        const ddsp_u2c_layer& L = w.layer[l];
        const ddsp_u2c_layer& GL = gr.layer[l];
        LayerBufs& b = bf.l[l];
#define GLP(p) const_cast<float*>(GL.p)
        // ===== conv module: x_out = x_mid + pw2(silu(dw(glu(pw1(LN(x_mid)))))) =====
        if ((rc = layer_grads(ctx, st, dX, D, D, b.dwo, INNER, INNER, 1, (int)Fr, M, wpart, cpart, xs, GLP(cm_pw2_w), INNER,
                              GLP(cm_pw2_b), 0, dfp))) return rc;
        dgrad(st, dX, D, L.cm_pw2_w, D, INNER, M, dB512, false, wt_pw2[l]);                                  // d_dwo
        hipLaunchKernelGGL(silu_bwd_kernel, dim3(grid_for(M * INNER)), dim3(256), 0, st, b.pre, dB512, M * INNER, dB512);  // d_pre
        {
            const int runs = (int)((Fr + DW_RUN - 1) / DW_RUN);
            hipLaunchKernelGGL(dwconv_wgrad_run_kernel, dim3(INNER / 256, (unsigned)(B * runs)), dim3(256), 0, st, dB512, b.glu, (int)B,
                               (int)Fr, dwpart, w.causal ? DWK - 1 : DWK / 2, in.n_frames);
            hipLaunchKernelGGL(dw_wgrad_reduce_kernel, dim3(INNER / 64, DWK), dim3(256), 0, st, dwpart, (int)B * runs, GLP(cm_dw_w));
        }
        if ((rc = colsum(ctx, st, dB512, INNER, M, INNER, nullptr, 0, cpart, GLP(cm_dw_b)))) return rc;
        hipLaunchKernelGGL((dwconv_kernel<false, true>), dim3(INNER / 256, (unsigned)(B * ((Fr + DW_RUN - 1) / DW_RUN))),
                           dim3(256), 0, st, dB512, L.cm_dw_w, nullptr, (int)B, (int)Fr, dC512, nullptr, DWK, 1, w.causal ? 0 : DWK / 2, 0);   // d_glu (adjoint taps: left' = DWK - 1 - left)
        if (in.n_frames) zero_padding_frames(st, dC512, in.n_frames, B, Fr, INNER);
        hipLaunchKernelGGL(glu_bwd_kernel, dim3(grid_for(M * INNER)), dim3(256), 0, st, b.g1, dC512, M, dG1);
        if ((rc = layer_grads(ctx, st, dG1, 2 * INNER, 2 * INNER, b.y2, D, D, 1, (int)Fr, M, wpart, cpart, xs, GLP(cm_pw1_w), D,
                              GLP(cm_pw1_b), 0, dfp))) return rc;
        dgrad(st, dG1, 2 * INNER, L.cm_pw1_w, 2 * INNER, D, M, dA, false, wt_pw1[l]);                         // d_y2
        hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(rows_g), dim3(256), 0, st, b.x_mid, L.cm_ln_w, dA, dX, M, dX, gx);
        if ((rc = colsum_pair(ctx, st, gx, dA, D, M, D, cpart, GLP(cm_ln_w), GLP(cm_ln_b)))) return rc;
        // dX now holds d x_mid

        // ===== attention: x_mid = x_in + to_out(attn) =====
        if ((rc = layer_grads(ctx, st, dX, D, D, b.attn, INNER, INNER, 1, (int)Fr, M, wpart, cpart, xs, GLP(out_w), INNER,
                              GLP(out_b), 0, dfp))) return rc;
        dgrad(st, dX, D, L.out_w, D, INNER, M, dB512, false, wt_out[l]);                                       // d_attn
        // the two K = 64 adjoint products of the attention (both operands K-contiguous, one problem per (utterance, head)): on the
        // LDS-DMA kernel in the context's arithmetic (round 3; the register-staged fp32 kernel took 51 us each at B = 32)
        auto attn_k64 = [&](hipStream_t s_, gemm::Args g, int batch, const EpiRowOuter& e) {
            if (ctx->math != DDSP_MATH_FP32 && gemm::dma_ok(g)) {
                g.math = DDSP_MATH_SPLIT_BF16;
                gemm::dma_go<64, 64, EpiRowOuter, 3, 4>(s_, g, batch, e);
            } else
                gemm::launch_tile<64, 64, true, true, gemm::A_PLAIN>(s_, g, batch, e);
        };
        if (w.causal) {
            // causal attention: three sequential scans per (utterance, head) (dD / coefq hold 1/den and d den between them)
            hipLaunchKernelGGL(causal_attn_bwd_q_kernel, dim3((unsigned)(B * H)), dim3(320), 0, st, b.qf, b.kf, b.v, dB512, b.attn,
                               (int)Fr, dQF, dD, coefq);
            hipLaunchKernelGGL(causal_attn_bwd_k_kernel, dim3((unsigned)(B * H)), dim3(320), 0, st, b.qf, b.v, dB512, dD, coefq,
                               (int)Fr, dKF);
            hipLaunchKernelGGL(causal_attn_bwd_v_kernel, dim3((unsigned)(B * H)), dim3(256), 0, st, b.qf, b.kf, dB512, dD, (int)Fr,
                               dV512);
        } else {
            hipLaunchKernelGGL(attn_out_bwd_kernel, dim3(rows8_g), dim3(256), 0, st, dB512, b.attn, b.dinv, M8, dD);  // d_num, d_D
            if (feat_fused) {   // d_ctx = q'^T d_num and d_ks = q'^T d_D, then d_q (in place of d_num), d_k and d_v: attn_feat_bwd_kernel
                if ((rc = attn_feat_bwd(ctx, st, b, L.proj, ptp + (size_t)l * FB_PT_VEC * 4, dB512, dD, dcx, dks, dcxt, dC512, dV512, B, Fr)))
                    return rc;
            } else {
                {   // d_q' = d_num ctx^T + d_D ks^T
                    gemm::Args g = gemm::make(dB512, INNER, b.cx, DH, (int)Fr, NF, DH);
                    g.zdiv = H;
                    g.sA_hi = (int64_t)Fr * INNER;
                    g.sA_lo = DH;
                    g.sB_hi = (int64_t)H * NF * DH;
                    g.sB_lo = (int64_t)NF * DH;
                    EpiRowOuter e{dQF, dD, b.ks, (int)Fr};
                    attn_k64(st, g, (int)(B * H), e);
                }
                {   // d_ctx = q'^T d_num, d_ks = q'^T d_D
                    gemm::Args g = gemm::make(b.qf, (int64_t)H * LDF, dB512, INNER, NF, DH, (int)Fr);
                    g.zdiv = H;
                    g.sA_hi = (int64_t)Fr * H * LDF;
                    g.sA_lo = LDF;
                    g.sB_hi = (int64_t)Fr * INNER;
                    g.sB_lo = DH;
                    gemm::EpiStore e{dcx, DH, nullptr, 1, (int64_t)NF * DH, 0};
                    gemm::launch_tile<64, 64, false, false, gemm::A_PLAIN>(st, g, (int)(B * H), e);
                    hipLaunchKernelGGL(weighted_key_sum_kernel, dim3((unsigned)(B * H)), dim3(KS_T * 8), 0, st, b.qf, dD, (int)Fr, dks);
                }
                {   // d_k' = v d_ctx^T + d_ks^T
                    gemm::Args g = gemm::make(b.v, INNER, dcx, DH, (int)Fr, NF, DH);
                    g.zdiv = H;
                    g.sA_hi = (int64_t)Fr * INNER;
                    g.sA_lo = DH;
                    g.sB_hi = (int64_t)H * NF * DH;
                    g.sB_lo = (int64_t)NF * DH;
                    EpiRowOuter e{dKF, nullptr, dks, (int)Fr};
                    attn_k64(st, g, (int)(B * H), e);
                }
                {   // d_v = k' d_ctx
                    gemm::Args g = gemm::make(b.kf, (int64_t)H * LDF, dcx, DH, (int)Fr, DH, NF);
                    g.zdiv = H;
                    g.sA_hi = (int64_t)Fr * H * LDF;
                    g.sA_lo = LDF;
                    g.sB_hi = (int64_t)H * NF * DH;
                    g.sB_lo = (int64_t)NF * DH;
                    EpiAttnOut e{dV512, nullptr, (int)Fr};
                    gemm::launch_tile<64, 64, true, false, gemm::A_PLAIN>(st, g, (int)(B * H), e);
                }
            }
        }
        if (!feat_fused) {   // d_q = d_raw_q P + coef_q q   (rows = (frame, head), 64 columns == the (M, 512) layout of q)
            hipLaunchKernelGGL(feature_map_bwd_kernel<true>, dim3(rows8_g), dim3(256), 0, st, b.qf, dQF, M8, coefq);
            hipLaunchKernelGGL(feature_map_bwd_kernel<false>, dim3(rows8_g), dim3(256), 0, st, b.kf, dKF, M8, coefk);
            gemm::Args g = gemm::make(dQF, LDF, L.proj, DH, (int)M8, DH, NF);
            EpiAxpyRow e{dB512, coefq, b.q, DH};
            gemm::launch<true, false, gemm::A_PLAIN>(st, g, 1, e);
            g.A = dKF;
            EpiAxpyRow e2{dC512, coefk, b.k, DH};
            gemm::launch<true, false, gemm::A_PLAIN>(st, g, 1, e2);
        }
        if (in.n_frames) {   // the context's gradient reaches the padding frames, whose k' and v the forward left out of the sums
            zero_padding_frames(st, dC512, in.n_frames, B, Fr, INNER);
            zero_padding_frames(st, dV512, in.n_frames, B, Fr, INNER);
        }
        DDSP_LAUNCH_CHECK(ctx);
        const float* dqkv[3] = {dB512, dC512, dV512};
        const float* pw[3] = {L.q_w, L.k_w, L.v_w};
        float* gw[3] = {GLP(q_w), GLP(k_w), GLP(v_w)};
        float* gb[3] = {GLP(q_b), GLP(k_b), GLP(v_b)};
        for (int i = 0; i < 3; ++i) {
            if ((rc = layer_grads(ctx, st, dqkv[i], INNER, INNER, b.y, D, D, 1, (int)Fr, M, wpart, cpart, xs, gw[i], D, gb[i], 0, dfp))) return rc;
            dgrad(st, dqkv[i], INNER, pw[i], INNER, D, M, dA, i > 0, wt_qkv[l][i]);                               // d_y (summed)
        }
        hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(rows_g), dim3(256), 0, st, b.x_in, L.norm_w, dA, dX, M, dX, gx);
        if ((rc = colsum_pair(ctx, st, gx, dA, D, M, D, cpart, GLP(norm_w), GLP(norm_b)))) return rc;
        // dX now holds d x_in of this layer
#undef GLP
    }

    // ---- side embeddings (x0 = conv2 + Lin(lf0) + Lin(phase/pi) + Lin(vol) + spk) ----
    {
        ColsumJobs jb{};
        jb.n = 4;
        const float* ws[4] = {in.f0, in.phase, in.volume, nullptr};
        const int wm[4] = {2, 3, 1, 0};
        float* outs[4] = {G(f0_w), G(phase_w), G(volume_w), G(f0_b)};
        for (int i = 0; i < 4; ++i) {
            jb.X[i] = dX;
            jb.wsrc[i] = ws[i];
            jb.wmode[i] = wm[i];
            jb.out[i] = outs[i];
        }
        if ((rc = colsum_multi(ctx, st, jb, D, M, D, cpart))) return rc;
    }
    DDSP_HIP(ctx, hipMemcpyAsync(G(phase_b), G(f0_b), D * sizeof(float), hipMemcpyDeviceToDevice, st));
    DDSP_HIP(ctx, hipMemcpyAsync(G(volume_b), G(f0_b), D * sizeof(float), hipMemcpyDeviceToDevice, st));
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;
    // (dA is free between the last LayerNorm adjoint and the conv2 input gradient: it holds the per-utterance sums)
    hipLaunchKernelGGL(utterance_sum_kernel, dim3((unsigned)B), dim3(1024), 0, st, dX, (int)Fr, in.mix.n > 0 ? nullptr : in.spk_id,
                       in.n_spk_id, w.n_spk, dA, dev_err);
    hipLaunchKernelGGL(spk_table_grad_kernel, dim3((unsigned)w.n_spk), dim3(D), 0, st, dA, B, in.spk_id, in.n_spk_id, in.mix,
                       G(spk_table));
    // ---- prenet conv2: weight gradient over the three taps, input gradient as the flipped conv ----
    if ((rc = layer_grads(ctx, st, dX, D, D, bf.t2, D, D, 3, (int)Fr, M, wpart, cpart, xs, pk, 3 * D, G(prenet_conv2_b),
                          w.causal ? -1 : 0))) return rc;
    hipLaunchKernelGGL(unpack_conv3_kernel, dim3(grid_for((int64_t)D * D * 3)), dim3(256), 0, st, pk, D, D, G(prenet_conv2_w));
    hipLaunchKernelGGL(pack_conv3_transposed_kernel, dim3(grid_for((int64_t)D * D * 3)), dim3(256), 0, st, w.prenet_conv2_w, D, D, w2t);
    {
        gemm::Args g = gemm::make(dX, D, w2t, 3 * D, (int)M, D, 3 * D);
        g.Fr = (int)Fr;
        g.Cin = D;
        g.tap_shift = w.causal ? 1 : 0;   // the adjoint of taps (-2, -1, 0) reads frames (0, +1, +2) of dX
        if (int rc = ddsp_zero_page(ctx, &g.zeros)) return rc;
        gemm::EpiStore e{dA, D, nullptr, 1, 0, 0};
        gemm::launch<true, true, gemm::A_CONV3>(st, g, 1, e);                                      // d_t2
    }
    // ---- GroupNorm + LeakyReLU ----
    hipLaunchKernelGGL(groupnorm_bwd_stats_kernel, dim3(4, (unsigned)B), dim3(256), 0, st, bf.t1, bf.t2, dA, bf.gst,
                       w.prenet_gn_w, (int)Fr, gbst, in.n_frames);
    hipLaunchKernelGGL(groupnorm_bwd_apply_kernel, dim3(grid_for(M * D)), dim3(256), 0, st, bf.t1, bf.t2, dA, bf.gst, gbst,
                       w.prenet_gn_w, M, (int)Fr, dX, gx, dA, in.n_frames);                        // dX = d_t1, dA = d_gn
    if ((rc = colsum_pair(ctx, st, gx, dA, D, M, D, cpart, G(prenet_gn_w), G(prenet_gn_b)))) return rc;
    // ---- prenet conv1 (the units carry no gradient) ----
    if ((rc = layer_grads(ctx, st, dX, D, D, in.units, w.n_unit, w.n_unit, 3, (int)Fr, M, wpart, cpart, xs, pk, 3 * w.n_unit,
                          G(prenet_conv1_b), w.causal ? -1 : 0))) return rc;
    hipLaunchKernelGGL(unpack_conv3_kernel, dim3(grid_for((int64_t)D * w.n_unit * 3)), dim3(256), 0, st, pk, D, w.n_unit,
                       G(prenet_conv1_w));
    // the deferred partial sums of the blocks' Linear layers, one launch
    PROF(PF_U2C_BWD, 0, 4.0 * df.used, flush_deferred(st, df));
    DDSP_LAUNCH_CHECK(ctx);
#undef G
    return DDSP_OK;
}

}  // namespace

// both entry points take the counts of a ragged batch (n_frames null: every row has Fr frames)
extern "C" int ddsp_unit2ctrl_bwd(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* wp, const float* units,
                                  const float* f0_frames, const float* phase_frames, const float* volume,
                                  const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host,
                                  const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, const int32_t* n_frames,
                                  const float* d_ctrl, const ddsp_u2c_weights* grads_host, float* ctrl_out) {
    U2CInputs in;
    int rc = check_inputs(ctx, wp, units, f0_frames, phase_frames, volume, spk_id, n_spk_id, mix_ids_host, mix_w_host,
                          n_mix, B, Fr, in);
    if (rc) return rc;
    in.n_frames = (const int*)n_frames;
    DDSP_REQUIRE(ctx, d_ctrl && grads_host, "ddsp_unit2ctrl_bwd: null argument");
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    if (B == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    return u2c_backward(ctx, (hipStream_t)stream, *wp, *grads_host, in, B, Fr, d_ctrl, ctrl_out, nullptr, 0);
}

extern "C" int ddsp_unit2ctrl_bwd_kept(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* wp, const float* units,
                                       const float* f0_frames, const float* phase_frames, const float* volume,
                                       const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host,
                                       const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, const int32_t* n_frames,
                                       void* keep, int64_t keep_bytes, const float* d_ctrl,
                                       const ddsp_u2c_weights* grads_host) {
    U2CInputs in;
    int rc = check_inputs(ctx, wp, units, f0_frames, phase_frames, volume, spk_id, n_spk_id, mix_ids_host, mix_w_host,
                          n_mix, B, Fr, in);
    if (rc) return rc;
    in.n_frames = (const int*)n_frames;
    DDSP_REQUIRE(ctx, d_ctrl && grads_host && keep && ((uintptr_t)keep % 256) == 0, "ddsp_unit2ctrl_bwd_kept: null argument or keep not 256-byte aligned");
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    if (B == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    return u2c_backward(ctx, (hipStream_t)stream, *wp, *grads_host, in, B, Fr, d_ctrl, nullptr, keep, (size_t)keep_bytes);
}
