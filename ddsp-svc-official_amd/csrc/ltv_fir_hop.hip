// a7 at hop 128 and 256: the frame-varying FIR of ltv_fir.hip for the smaller block sizes, forward and adjoint.
//
// The arithmetic statement is the one in the header of ltv_fir.hip with `hop` a template parameter:
//
//   out[u] = sum_m sum_k  ir[min(m,Fr-1)][k] * xw_m[u + n/2 - k],   xw_m[t] = x[t] * tri(t - hop*(m-1))
//
// tri the periodic Bartlett window of length 2*hop, m = 0..Fr (frame Fr reuses filter Fr-1), cropped to T = Fr*hop,
// and the same MFMA mapping (columns of 16 samples, 16x16 output tiles, Toeplitz-block products of fir_tile.h on
// v_mfma_f32_16x16x4_f32).  The filter lengths are the same as at 512 (even n, 32..2046), so a filter spans up to
// n/hop = 16 hops here and the frames that reach a block do not fit the LDS at once.  The staging therefore differs
// from the 512 kernel's:
//   * a block owns 8 output tiles (2048 samples, whatever the hop); the frames whose support can reach them,
//     floor((C0 - q_hi)/HOPC) .. floor((C0 + 127 - q_lo)/HOPC) + 1 with C0 the block's first column - a range that
//     follows n/hop -, are staged in batches of `nfb` frames (as many as the LDS budget holds), one wavefront per
//     frame, and each batch is multiplied into the register accumulators before the next one replaces it;
//   * a frame image is 2*HOPC columns (+16 pad columns either side) transposed to [r][col] with row stride 80
//     (= 16 mod 32) and the 2*(r>>1) column skew of the 512 kernel: ds_read_b32 banks are (addr/4) mod 32 per half
//     wave; the two rows r, r+1 a half wave reads sit 16 banks apart, rows r+2, r+3 two banks further on, so the
//     B-operand fetch (lanes along col) is conflict-free.  The fill is 2-way conflicted on writes, once per frame;
//   * tiles are not aligned to hops (at hop 128 a tile is two hops), which only the column arithmetic sees; a
//     trailing partial tile (Fr*hop not a multiple of 256) masks its stores by column.
// Every loop bound around the MFMA loops derives from blockIdx and readfirstlane(wave): they stay in SGPRs.
//
// Products: fp32 matrix pipe only.  There is no split-bf16 form for these hops: they use the fp32 kernels whatever
// `ddsp_ctx_set_math` says.  The kernels are untuned (about half the issued MACs at hop 128 multiply zero pad, and
// nothing overlaps the staging with the products).
//
// The generated noise is `noise_u` of fir_tile.h on (seed, b*T + t), the function the 512 kernels use.
#include "fir_tile.h"

namespace {

constexpr int IRPAD = 32;
constexpr int PADC = 16;
constexpr int RS = 80;          // row stride of a transposed frame image (floats): 2*HOPC + 2*PADC + 14 of skew <= 78
constexpr int XS = 16 * RS;     // floats per frame image
constexpr int NWF = 8;          // forward: wavefronts (output tiles) per block
constexpr int NWB = 4;          // input adjoint: wavefronts (output tiles) per block
constexpr size_t LDS_BUDGET = 112 * 1024;

struct FirHopArgs {
    const float* audio;  // (B,T) or null
    int excitation;      // DDSP_EXC_*
    uint64_t seed;
    const float* ir;     // (B,Fr,n)
    const float* add_in; // (B,T) or null
    float* out;          // (B,T) or null: filtered signal
    float* out_sum;      // (B,T) or null: filtered signal + add_in
    int Fr, n;
    int q_lo, q_hi;      // column-shift range of the filter
    int nfb;             // frames staged per batch
    int irs;             // floats per staged filter row (n + 2*IRPAD, rounded)
};

// One wavefront stages frame m (0 <= m <= Fr) of batch row b: filter row at `fd`, windowed transposed input at `xd`.
// LDS accesses of one wave are ordered, so the zero fill needs no barrier before the scatter.
template <int HOP>
__device__ __forceinline__ void fir_hop_stage(const FirHopArgs& g, int b, int m, float* __restrict__ fd,
                                              float* __restrict__ xd, int lane) {
    constexpr int KP = 2 * HOP / 256;   // float4 passes of 64 lanes over the 2*HOP samples of a frame
    const int64_t T = (int64_t)g.Fr * HOP;
    for (int i = lane; i < XS / 4; i += 64) ((f32x4*)xd)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
        const int mi = m < g.Fr ? m : g.Fr - 1;
        const float2* src = (const float2*)(g.ir + ((int64_t)b * g.Fr + mi) * g.n);
        float2* dst = (float2*)fd;
        const int per_row = g.irs / 2, half_n = g.n / 2;
        for (int base = 0; base < per_row; base += 64 * 8) {
            float2 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int k2 = base + 64 * k + lane - IRPAD / 2;
                v[k] = float2{0.f, 0.f};
                if (k2 >= 0 && k2 < half_n) v[k] = src[k2];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = base + 64 * k + lane;
                if (i < per_row) dst[i] = v[k];
            }
        }
    }
    const int64_t tb = (int64_t)HOP * (m - 1);
    f32x4 x[KP];
    bool ok[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int64_t t = tb + 4 * (lane + 64 * k);
        ok[k] = t >= 0 && t < T;
        x[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (ok[k]) {
            if (g.excitation == DDSP_EXC_GENERATE) {
#pragma unroll
                for (int e = 0; e < 4; ++e) x[k][e] = noise_u(g.seed, (uint64_t)b * T + t + e);
            } else {
                x[k] = *(const f32x4*)(g.audio + (int64_t)b * T + t);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (!ok[k]) continue;
        const int z = 4 * (lane + 64 * k);
        if (g.excitation == DDSP_EXC_UNIT_NOISE) {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[k][e] = __fadd_rn(__fmul_rn(x[k][e], 2.0f), -1.0f);
        }
        const int r0 = z & 15, col = z >> 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int zz = z + e, r = r0 + e;
            const float w = (zz < HOP) ? (float)zz * (1.0f / HOP) : (float)(2 * HOP - zz) * (1.0f / HOP);
            xd[r * RS + PADC + col + 2 * (r >> 1)] = x[k][e] * w;
        }
    }
}

template <int HOP>
__global__ void __launch_bounds__(64 * NWF) ltv_fir_hop_kernel(FirHopArgs g) {
    constexpr int HOPC = HOP / 16;
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: the MFMA loop bounds stay in SGPRs
    const int b = blockIdx.y;
    const int C0 = blockIdx.x * (16 * NWF);   // first output column of the block
    const int ncols = g.Fr * HOPC;            // columns of the signal
    const int64_t T = (int64_t)g.Fr * HOP;
    const int c = g.n / 2;

    // frames whose 2*HOPC-column support [HOPC*(m-1), HOPC*(m+1)) meets the input columns the block touches,
    // [C0 - q_hi, C0 + 16*NWF - 1 - q_lo], clipped to the frames there are
    const int lo_col = C0 - g.q_hi;
    const int m_first = lo_col > 0 ? lo_col / HOPC : 0;
    int m_last = (C0 + 16 * NWF - 1 - g.q_lo) / HOPC + 1;
    if (m_last > g.Fr) m_last = g.Fr;

    float* fs = lds;                           // [nfb][g.irs]
    float* xs = lds + (size_t)g.nfb * g.irs;   // [nfb][XS]

    const int J0 = C0 + 16 * wave;             // first output column of this wavefront's tile
    const bool active = J0 < ncols;
    const int li = lane & 15, lk = lane >> 4;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // lane-constant operand offsets, as in ltv_fir_kernel: k-step s uses image row r = 4s + lk
    const int a_base = IRPAD + c + li - lk;
    const int b_base = lk * RS + PADC + 2 * (lk >> 1) + li;
    constexpr int BSTEP = 4 * RS + 4;

    for (int mb = m_first; mb <= m_last; mb += g.nfb) {
        const int nf = (m_last - mb + 1 < g.nfb) ? m_last - mb + 1 : g.nfb;
        if (mb != m_first) __syncthreads();    // the previous batch has been multiplied
        for (int f = wave; f < nf; f += NWF)
            fir_hop_stage<HOP>(g, b, mb + f, fs + (size_t)f * g.irs, xs + (size_t)f * XS, lane);
        __syncthreads();
        if (active) {
            for (int f = 0; f < nf; ++f) {
                const int cbase = HOPC * (mb + f - 1);   // absolute column of the frame image's column 0
                int qa = J0 - (cbase + 2 * HOPC) + 1;
                int qb = J0 + 15 - cbase;
                if (qa < g.q_lo) qa = g.q_lo;
                if (qb > g.q_hi) qb = g.q_hi;
                toeplitz_accumulate<-1, -1>(fs + (size_t)f * g.irs + a_base, xs + (size_t)f * XS + (J0 - cbase) + b_base,
                                            BSTEP, qa, qb, acc);
            }
        }
    }
    if (!active || J0 + li >= ncols) return;
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
    // C/D map of the 16x16 MFMA: col = lane & 15, row = 4*(lane >> 4) + reg
    const int64_t u = (int64_t)b * T + 16 * (int64_t)(J0 + li) + 4 * lk;
    if (g.out) *(f32x4*)(g.out + u) = o;
    if (g.out_sum) {
        const f32x4 ad = *(const f32x4*)(g.add_in + u);
        *(f32x4*)(g.out_sum + u) = ad + o;
    }
}

// ---- backward: the two adjoints of ltv_fir.hip (its comment block "backward" states them) --------------------------

// (1) input gradient.  A block owns NWB tiles = SPB segments and stages the SPB + 1 reversed filters of frames
// s0 .. s0 + SPB and one raw image of d_y.  A tile of SPT segments (two at hop 128) runs one product pass per frame
// s .. s + SPT; a lane keeps, of each pass, the frame's window weight at its own sample - zero where the frame does not
// cover the lane's segment.
struct FirHopBwdInArgs {
    const float* dy;  // (B,T)
    const float* ir;  // (B,Fr,n)
    float* dx;        // (B,T)
    int Fr, n, q_lo, q_hi, irs, rsb, col_off;  // col_off = q_hi (image column 0 = absolute column C0 - q_hi)
};

template <int HOP>
__global__ void __launch_bounds__(64 * NWB) ltv_fir_hop_bwd_input_kernel(FirHopBwdInArgs g) {
    constexpr int HOPC = HOP / 16, SPB = 16 * NWB / HOPC, SPT = 16 / HOPC;
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, s0 = blockIdx.x * SPB;
    const int C0 = HOPC * s0;
    const int ncols = g.Fr * HOPC;
    const int64_t T = (int64_t)g.Fr * HOP;
    const int cp = g.n / 2 - 1;
    float* fs = lds;                               // [SPB+1][g.irs]  reversed filters
    float* img = lds + (size_t)(SPB + 1) * g.irs;  // [16][g.rsb]     raw d_y, transposed + skewed
    for (int f = 0; f <= SPB; ++f) {
        const int m = s0 + f;
        const bool live = m <= g.Fr;
        const int mi = m < g.Fr ? m : g.Fr - 1;
        const float* src = g.ir + ((int64_t)b * g.Fr + (live ? mi : 0)) * g.n;
        float* dst = fs + (size_t)f * g.irs;
        for (int i = tid; i < g.irs; i += 64 * NWB) {
            const int k = i - IRPAD;
            dst[i] = (live && k >= 0 && k < g.n) ? src[g.n - 1 - k] : 0.f;
        }
    }
    const int ncol = g.rsb - 16;                   // columns the image covers (a multiple of 32)
    const int64_t t_base = 16 * ((int64_t)C0 - g.col_off);
    for (int z = 4 * tid; z < 16 * ncol; z += 4 * 64 * NWB) {
        const int64_t t = t_base + z;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < T) v = *(const f32x4*)(g.dy + (int64_t)b * T + t);
        const int r0 = z & 15, col = z >> 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) img[(r0 + e) * g.rsb + col + 2 * ((r0 + e) >> 1)] = v[e];
    }
    __syncthreads();
    const int J0 = C0 + 16 * wave;
    if (J0 >= ncols) return;
    const int li = lane & 15, lk = lane >> 4;
    const int a_base = IRPAD + cp + li - lk;
    const int b_base = lk * g.rsb + 2 * (lk >> 1) + li + (J0 - C0 + g.col_off);
    const int bstep = 4 * g.rsb + 4;
    const int sfirst = wave * SPT;                 // the tile's first segment, relative to s0
    const int sl = sfirst + li / HOPC;             // this lane's segment
    const int j0 = 16 * (li % HOPC) + 4 * lk;      // position of this lane's first sample in its segment
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p <= SPT; ++p) {
        const int f = sfirst + p;
        f32x4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        toeplitz_accumulate<-1, -1>(fs + (size_t)f * g.irs + a_base, img + b_base, bstep, g.q_lo, g.q_hi, acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float j = (float)(j0 + e) * (1.0f / HOP);
            const float w = (f == sl) ? 1.0f - j : ((f == sl + 1) ? j : 0.0f);
            o[e] = fmaf(w, (acc[0][e] + acc[1][e]) + (acc[2][e] + acc[3][e]), o[e]);
        }
    }
    if (J0 + li < ncols) *(f32x4*)(g.dx + (int64_t)b * T + 16 * (int64_t)(J0 + li) + 4 * lk) = o;
}

// (2) filter gradient: ltv_fir_bwd_filter_kernel with the frame length a template parameter.  One workgroup per
// (utterance, frame); "taps" = the windowed input frame (2*hop values), "signal" = d_y around it, outputs = the n taps.
struct FirHopBwdIrArgs {
    const float* audio;  // forward input (B,T) or null
    int excitation;
    uint64_t seed;
    const float* dy;     // (B,T)
    float* dir;          // (B,Fr,n)
    int Fr, n, rsf, tiles;
};

template <int HOP>
__global__ void __launch_bounds__(256) ltv_fir_hop_bwd_filter_kernel(FirHopBwdIrArgs g) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, m0 = blockIdx.x;       // frame m0 < Fr; frame Fr (same filter) is folded into Fr-1
    const int64_t T = (int64_t)g.Fr * HOP;
    const int c = g.n / 2;
    constexpr int HROW = 2 * HOP + 2 * IRPAD;        // windowed frame with 32 zeros either side
    float* hrow = lds;
    float* img = lds + HROW;                         // [16][g.rsf]
    const int li = lane & 15, lk = lane >> 4;
    const int bstep = 4 * g.rsf + 4;
    const int n_pass = (m0 == g.Fr - 1) ? 2 : 1;
    f32x4 out[4];                                    // this wave's tiles: wave, wave+4, ... (n <= 2046: at most 2)
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int pass = 0; pass < n_pass; ++pass) {
        const int m = m0 + pass;
        const int64_t tb = (int64_t)HOP * (m - 1);
        __syncthreads();
        for (int i = tid; i < HROW; i += 256) {
            const int z = i - IRPAD;
            float v = 0.f;
            const int64_t t = tb + z;
            if (z >= 0 && z < 2 * HOP && t >= 0 && t < T) {
                float x;
                if (g.excitation == DDSP_EXC_GENERATE) {
                    x = noise_u(g.seed, (uint64_t)b * T + t);
                } else {
                    x = g.audio[(int64_t)b * T + t];
                    if (g.excitation == DDSP_EXC_UNIT_NOISE) x = __fadd_rn(__fmul_rn(x, 2.0f), -1.0f);
                }
                const float w = (z < HOP) ? (float)z * (1.0f / HOP) : (float)(2 * HOP - z) * (1.0f / HOP);
                v = x * w;
            }
            hrow[i] = v;
        }
        const int ncol = g.rsf - 16;
        for (int z = 4 * tid; z < 16 * ncol; z += 4 * 256) {
            const int64_t t = tb - c + z;                 // c = n/2 may be odd -> element-wise bounds and loads
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t + e >= 0 && t + e < T) v[e] = g.dy[(int64_t)b * T + t + e];
            const int r0 = z & 15, col = z >> 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) img[(r0 + e) * g.rsf + col + 2 * ((r0 + e) >> 1)] = v[e];
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int tile = wave + 4 * it;
            if (tile < g.tiles) {
                const int J = 16 * tile;
                f32x4 acc[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
                const float* ap = hrow + IRPAD + lk - li;
                const float* bp = img + lk * g.rsf + 2 * (lk >> 1) + li + J;
                toeplitz_accumulate<1, 1>(ap, bp, bstep, 0, 2 * HOP / 16, acc);
#pragma unroll
                for (int e = 0; e < 4; ++e) out[it][e] += (acc[0][e] + acc[1][e]) + (acc[2][e] + acc[3][e]);
            }
        }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int tile = wave + 4 * it;
        if (tile < g.tiles) {
            const int k0 = 16 * (16 * tile + li) + 4 * lk;
            float* dst = g.dir + ((int64_t)b * g.Fr + m0) * g.n;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (k0 + e < g.n) dst[k0 + e] = out[it][e];
        }
    }
}

template <int HOP>
int fir_hop_forward(ddsp_ctx* ctx, hipStream_t st, FirHopArgs g, int64_t B) {
    constexpr int HOPC = HOP / 16;
    const int c = g.n / 2;
    g.q_lo = -((c + 15) / 16);
    g.q_hi = (c + 14) / 16;
    g.irs = (g.n + 2 * IRPAD + 3) & ~3;
    // most frames a block can need (kernel: m_first .. m_last), and how many of them the LDS budget holds at once
    const int max_frames = (16 * NWF + g.q_hi - g.q_lo) / HOPC + 3;
    const size_t per_frame = (size_t)(g.irs + XS) * sizeof(float);
    int nfb = (int)(LDS_BUDGET / per_frame);
    if (nfb > max_frames) nfb = max_frames;
    g.nfb = nfb;                                   // >= 8: per_frame <= 13.3 KiB at n = 2046
    const size_t lds_bytes = (size_t)nfb * per_frame;
    DDSP_ONCE_PER_DEVICE(ctx, DDSP_HIP(ctx, hipFuncSetAttribute((const void*)ltv_fir_hop_kernel<HOP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)));
    const int64_t ncols = (int64_t)g.Fr * HOPC;
    dim3 grid((unsigned)ceil_div64(ncols, 16 * NWF), (unsigned)B);
    hipLaunchKernelGGL((ltv_fir_hop_kernel<HOP>), grid, dim3(64 * NWF), lds_bytes, st, g);
    return DDSP_OK;
}

template <int HOP>
int fir_hop_backward(ddsp_ctx* ctx, hipStream_t st, const float* audio, int excitation, uint64_t noise_seed,
                     const float* ir, const float* d_out, int64_t B, int64_t Fr, int n, float* d_audio, float* d_ir) {
    constexpr int HOPC = HOP / 16;
    DDSP_ONCE_PER_DEVICE(ctx, DDSP_HIP(ctx, hipFuncSetAttribute((const void*)ltv_fir_hop_bwd_input_kernel<HOP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); DDSP_HIP(ctx, hipFuncSetAttribute((const void*)ltv_fir_hop_bwd_filter_kernel<HOP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)));
    const double Ts = (double)Fr * HOP;
    if (d_audio) {
        FirHopBwdInArgs g;
        g.dy = d_out;
        g.ir = ir;
        g.dx = d_audio;
        g.Fr = (int)Fr;
        g.n = n;
        const int cp = n / 2 - 1;
        g.q_lo = -((cp + 15) / 16);
        g.q_hi = (cp + 14) / 16;
        g.irs = (n + 2 * IRPAD + 3) & ~3;
        g.col_off = g.q_hi;
        // image columns: [C0 - q_hi, C0 + 16*NWB - 1 - q_lo] (+ up to 14 of skew), row stride = 16 (mod 32)
        const int width = 16 * NWB + g.q_hi - g.q_lo;
        const int ncol = (width + 31) & ~31;
        g.rsb = ncol + 16;
        constexpr int SPB = 16 * NWB / HOPC;
        const size_t lds_bytes = ((size_t)(SPB + 1) * g.irs + 16 * (size_t)g.rsb) * sizeof(float);
        DDSP_REQUIRE(ctx, lds_bytes <= 160 * 1024, "ddsp_ltv_fir_bwd: filter too long for the LDS staging");
        ddsp_prof_begin(ctx, st, PF_LTV_FIR_BWD);
        hipLaunchKernelGGL((ltv_fir_hop_bwd_input_kernel<HOP>), dim3((unsigned)ceil_div64(Fr * HOPC, 16 * NWB), (unsigned)B),
                           dim3(64 * NWB), lds_bytes, st, g);
        ddsp_prof_end(ctx, st, (double)B * Ts * n * 4.0, 4.0 * B * (2.0 * Ts + (double)Fr * n));
    }
    if (d_ir) {
        FirHopBwdIrArgs g;
        g.audio = audio;
        g.excitation = excitation;
        g.seed = noise_seed;
        g.dy = d_out;
        g.dir = d_ir;
        g.Fr = (int)Fr;
        g.n = n;
        g.tiles = (n + 255) / 256;
        // signal positions used: [0, 2*hop - 1 + n) -> columns, + skew, row stride = 16 (mod 32)
        const int ncol = ((2 * HOP + n + 15) / 16 + 16 + 31) & ~31;
        g.rsf = ncol + 16;
        const size_t lds_bytes = ((size_t)(2 * HOP + 2 * IRPAD) + 16 * (size_t)g.rsf) * sizeof(float);
        ddsp_prof_begin(ctx, st, PF_LTV_FIR_BWD);
        hipLaunchKernelGGL((ltv_fir_hop_bwd_filter_kernel<HOP>), dim3((unsigned)Fr, (unsigned)B), dim3(256), lds_bytes, st, g);
        ddsp_prof_end(ctx, st, (double)B * Ts * n * 4.0, 4.0 * B * (2.0 * Ts + (double)Fr * n));
    }
    return DDSP_OK;
}

}  // namespace

int ddsp_ltv_fir_hop(ddsp_ctx* ctx, hipStream_t st, const float* audio, int excitation, uint64_t noise_seed,
                     const float* ir, int64_t B, int64_t Fr, int hop, int n, const float* add_in, float* out,
                     float* out_sum) {
    FirHopArgs g;
    g.audio = audio;
    g.excitation = excitation;
    g.seed = noise_seed;
    g.ir = ir;
    g.add_in = add_in;
    g.out = out;
    g.out_sum = out_sum;
    g.Fr = (int)Fr;
    g.n = n;
    DDSP_REQUIRE(ctx, Fr * (int64_t)(hop / 16) < (1ll << 31) - 256, "ddsp_ltv_fir: signal too long");
    DDSP_ENTER_DEVICE(ctx);
    const double Tsig = (double)Fr * hop, nbat = (double)B;
    ddsp_prof_begin(ctx, st, PF_LTV_FIR);
    const int rc = hop == 128 ? fir_hop_forward<128>(ctx, st, g, B) : fir_hop_forward<256>(ctx, st, g, B);
    if (rc != DDSP_OK) return rc;
    ddsp_prof_end(ctx, st, nbat * Tsig * n * 2.0 * 2.0,
                  4.0 * nbat * (Tsig * ((audio ? 1 : 0) + (out ? 1 : 0) + (out_sum ? 2 : 0)) + (double)Fr * n));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

int ddsp_ltv_fir_hop_bwd(ddsp_ctx* ctx, hipStream_t st, const float* audio, int excitation, uint64_t noise_seed,
                         const float* ir, const float* d_out, int64_t B, int64_t Fr, int hop, int n, float* d_audio,
                         float* d_ir) {
    DDSP_ENTER_DEVICE(ctx);
    const int rc = hop == 128 ? fir_hop_backward<128>(ctx, st, audio, excitation, noise_seed, ir, d_out, B, Fr, n, d_audio, d_ir)
                              : fir_hop_backward<256>(ctx, st, audio, excitation, noise_seed, ir, d_out, B, Fr, n, d_audio, d_ir);
    if (rc != DDSP_OK) return rc;
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
