// The autocorrelation f0 extractor (Boersma 1993: "Accurate short-term analysis of the fundamental frequency and the
// harmonics-to-noise ratio of a sampled sound") with the parameters of the reference's `'parselmouth'` call
// (ddsp/vocoder.py:55-69): Hanning window of 3 periods, voicing threshold 0.6, silence threshold 0.03, octave cost 0.01,
// octave-jump cost 0.35, voiced/unvoiced cost 0.14.
//
//   stats_kernel  one workgroup per row: mean and max |x - mean| (fp64 sums in a fixed order: a row of a batch is the row alone)
//   frame_kernel  one workgroup per (frame, row): the windowed frame in the LDS, its autocorrelation by a packed real FFT of
//                 nfft points (nfft / 2 complex points, in place: decimation in frequency forward, the power spectrum on the
//                 bit-reversed bins, decimation in time back), normalised by the window's own autocorrelation; the peak scan
//                 and the candidate list on wave 0 (one sinc term per lane, one candidate per lane), the Brent refinement with
//                 8 lanes per candidate.  fp32 up to the normalised autocorrelation, fp64 from the interpolation on.
//   path_kernel   one wave per row, candidates across lanes: the Viterbi recursion with frame-sequential back-pointers, one
//                 backtrack through LDS-staged blocks, then the padding, the interpolation over unvoiced frames and the clamp.
#include "tables.h"

namespace {

constexpr int FT = 256;            // threads of the frame workgroup
constexpr int MAX_C = 32;          // candidates per frame, the unvoiced one included (8 lanes each in the refinement)
constexpr int MAX_NFFT = 8192;
constexpr int BT = 64;             // frames per backtracking block
constexpr double kPi = 3.14159265358979323846264338327950288;
constexpr double kVoicing = 0.6, kSilence = 0.03, kOctave = 0.01, kOctaveJump = 0.35, kVuv = 0.14;

struct Geo {
    int W, half, nfft, log2m, imax, lag_min, lag_max, period, half_period, C;
    int hw_ld, win_ld;             // table: hw[hw_ld] | window[win_ld] | twiddles exp(-2 pi i k / nfft), k < nfft / 2
    double dx, dt, three_periods, hop, f0_min, f0_max;
    int sr;
};

bool make_geo(int sr, double hop, double f0_min, double f0_max, Geo& g) {
    if (!(sr > 0 && hop > 0.0 && f0_min > 0.0 && f0_max > f0_min && hop < 1e9 && f0_max < 1e9)) return false;
    g.sr = sr;
    g.hop = hop;
    g.f0_min = f0_min;
    g.f0_max = f0_max;
    g.dx = 1.0 / sr;
    g.dt = hop / sr;
    g.three_periods = 3.0 / f0_min;
    const double w0 = floor(3.0 / f0_min / g.dx);
    if (!(w0 >= 66.0 && w0 < 1e6)) return false;
    g.half = (int)w0 / 2 - 1;
    g.W = 2 * g.half;
    g.nfft = 1;
    while ((double)g.nfft < 1.5 * g.W) g.nfft *= 2;
    if (g.nfft > MAX_NFFT) return false;
    g.log2m = 0;
    while ((2 << g.log2m) < g.nfft) ++g.log2m;
    g.imax = g.W / 2;
    const int lm = (int)floor(sr / f0_max);
    g.lag_min = lm > 2 ? lm : 2;
    g.lag_max = g.W / 3 + 2 < g.W ? g.W / 3 + 2 : g.W;
    g.period = (int)floor(sr / f0_min);
    g.half_period = g.period / 2 + 1;
    const int c = (int)floor(f0_max / f0_min);
    g.C = c > 15 ? c : 15;
    g.hw_ld = ddsp_pad4(g.imax + 1);
    g.win_ld = ddsp_pad4(g.W);
    return g.C <= MAX_C && g.lag_min + 1 < g.imax;
}

// frames of a row of N samples (<= 0: shorter than one window); the same fp64 expression as ddsp_f0_ac_frames
__host__ __device__ inline int64_t row_frames(int64_t N, double dx, double dt, double three_periods) {
    return (int64_t)floor(((double)N * dx - three_periods) / dt) + 1;
}

// ---- the per-geometry table (kind TAB_F0_AC of the context's table cache, made on the first call of a geometry) ---------
__global__ void __launch_bounds__(256) table_kernel(float* __restrict__ tab, int W, int imax, int nfft, int hw_ld, int win_ld) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    auto h = [&](int j) { return 0.5 - 0.5 * cospi(2.0 * (double)(j + 1) / (double)(W + 1)); };
    if ((int)blockIdx.x <= imax) {
        const int l = blockIdx.x;
        double num = 0.0, nrm = 0.0;
        for (int j = tid; j < W; j += 256) {
            const double a = h(j);
            nrm += a * a;
            if (j + l < W) num += a * h(j + l);
        }
        red[0][tid] = num;
        red[1][tid] = nrm;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                red[0][tid] += red[0][tid + s];
                red[1][tid] += red[1][tid + s];
            }
            __syncthreads();
        }
        if (tid == 0) tab[l] = (float)(red[0][0] / red[1][0]);
        return;
    }
    const int e = ((int)blockIdx.x - imax - 1) * 256 + tid;
    if (e < W) tab[hw_ld + e] = (float)h(e);
    if (e < nfft / 2) {
        tab[hw_ld + win_ld + 2 * e] = (float)cospi(2.0 * (double)e / (double)nfft);
        tab[hw_ld + win_ld + 2 * e + 1] = (float)(-sinpi(2.0 * (double)e / (double)nfft));
    }
}

// ---- row statistics --------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t row_samples(const int32_t* __restrict__ n_samples, int b, int64_t T) {
    if (!n_samples) return T;
    const int64_t n = n_samples[b];
    return n < 0 ? 0 : (n > T ? T : n);
}

__global__ void __launch_bounds__(256) stats_kernel(const float* __restrict__ audio, int64_t T, const int32_t* __restrict__ n_samples,
                                                    float* __restrict__ stats) {
    __shared__ double red[256];
    __shared__ float mean_s;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t N = row_samples(n_samples, b, T);
    const float* x = audio + (int64_t)b * T;
    double s = 0.0;
    for (int64_t i = tid; i < N; i += 256) s += (double)x[i];
    red[tid] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) red[tid] += red[tid + k];
        __syncthreads();
    }
    if (tid == 0) mean_s = N > 0 ? (float)(red[0] / (double)N) : 0.f;
    __syncthreads();
    const float mean = mean_s;
    float pk = 0.f;
    for (int64_t i = tid; i < N; i += 256) pk = fmaxf(pk, fabsf(x[i] - mean));
    __syncthreads();
    red[tid] = (double)pk;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) red[tid] = fmax(red[tid], red[tid + k]);
        __syncthreads();
    }
    if (tid == 0) {
        stats[2 * b] = mean;
        stats[2 * b + 1] = (float)red[0];
    }
}

// ---- the frame -------------------------------------------------------------------------------------------------------
struct c32 {
    float x, y;
};

// Hann-windowed sinc interpolation of the even sequence r[|k|], |k| <= imax, at x with `depth` terms on each side, the terms
// dealt to the G neighbouring lanes of a group (sub = lane within the group); every lane of the group returns the same sum
template <int G>
__device__ __forceinline__ double sinc_interp(const float* __restrict__ r, int imax, double x, int depth, int sub) {
    if (!(x >= 0.0 && x <= (double)imax)) return 0.0;
    const double fl = floor(x);
    const int m = (int)fl;
    if (x == fl) return (double)r[m];
    int D = depth < m + imax + 1 ? depth : m + imax + 1;
    D = D < imax - m ? D : imax - m;
    const int L = m + 1 - D, R = m + D;
    const double dl = x - (double)L + 1.0, dr = (double)R - x + 1.0;
    double acc = 0.0;
    for (int k = L + sub; k <= R; k += G) {
        const bool left = k <= m;
        const double u = left ? x - (double)k : (double)k - x;
        const int ak = k < 0 ? -k : k;
        acc += (double)r[ak] * (sinpi(u) / (kPi * u)) * (0.5 + 0.5 * cospi(u / (left ? dl : dr)));
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    return acc;
}

__device__ __forceinline__ int bitrev(int k, int bits) { return (int)(__brev((unsigned)k) >> (32 - bits)); }

struct FrameOut {
    double* cand;      // (B, nF_max, C, 2): frequency, strength; slot 0 the unvoiced candidate
    int32_t* ncand;    // (B, nF_max)
    float* lpeak;      // (B, nF_max)
};

__global__ void __launch_bounds__(FT) frame_kernel(const float* __restrict__ audio, int64_t T, const int32_t* __restrict__ n_samples,
                                                   const float* __restrict__ stats, const float* __restrict__ tab, Geo g,
                                                   int64_t nF_max, FrameOut out) {
    extern __shared__ float buf[];          // nfft floats: the frame, its spectrum (nfft / 2 complex), then r[0..imax]
    __shared__ float red[FT];
    __shared__ unsigned peak_bits[(MAX_NFFT / 3 + 64) / 32];
    __shared__ double cand_f[MAX_C], cand_s[MAX_C];
    __shared__ int cand_l[MAX_C], n_cand_s;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t i = blockIdx.x;
    const int64_t N = row_samples(n_samples, b, T);
    const int64_t nF = row_frames(N, g.dx, g.dt, g.three_periods);
    if (i >= nF || i >= nF_max) return;
    const float* x = audio + (int64_t)b * T;
    const float mean = stats[2 * b], gpeak = stats[2 * b + 1];
    const int64_t slot = (int64_t)b * nF_max + i;
    double* co = out.cand + slot * g.C * 2;
    for (int c = tid; c < 2 * g.C; c += FT) co[c] = 0.0;
    if (!(gpeak > 0.f)) {
        if (tid == 0) {
            out.ncand[slot] = 1;
            out.lpeak[slot] = 0.f;
        }
        return;
    }
    const double t = 0.5 * (double)N * g.dx - 0.5 * (double)nF * g.dt + 0.5 * g.dt + (double)i * g.dt;
    const int64_t left = (int64_t)floor(t / g.dx - 0.5), right = left + 1;
    const int64_t start = right - g.half;
    const int W = g.W, nfft = g.nfft, M = nfft / 2, imax = g.imax;
    const float* hw = tab;
    const float* win = tab + g.hw_ld;
    const c32* tw = (const c32*)(tab + g.hw_ld + g.win_ld);
    for (int j = tid; j < W; j += FT) {
        const int64_t idx = start + j;
        buf[j] = (idx >= 0 && idx < N) ? x[idx] - mean : 0.f;
    }
    for (int j = W + tid; j < nfft; j += FT) buf[j] = 0.f;
    for (int w = tid; w < (int)(sizeof(peak_bits) / sizeof(unsigned)); w += FT) peak_bits[w] = 0u;
    __syncthreads();
    // local mean over [right - period, left + period], local peak over [left - half_period, right + half_period]
    auto clampj = [&](int64_t v) { return (int)(v < 0 ? 0 : (v > W ? W : v)); };
    const int m0 = clampj(right - g.period - start), m1 = clampj(left + g.period + 1 - start);
    float s = 0.f;
    for (int j = m0 + tid; j < m1; j += FT) s += buf[j];
    red[tid] = s;
    __syncthreads();
    for (int k = FT / 2; k > 0; k >>= 1) {
        if (tid < k) red[tid] += red[tid + k];
        __syncthreads();
    }
    const float lmean = m1 > m0 ? red[0] / (float)(m1 - m0) : 0.f;
    __syncthreads();
    const int64_t p_lo = left - g.half_period < 0 ? 0 : left - g.half_period;
    const int64_t p_hi = right + g.half_period > N - 1 ? N - 1 : right + g.half_period;
    const int p0 = clampj(p_lo - start), p1 = clampj(p_hi + 1 - start);
    float pk = 0.f;
    for (int j = p0 + tid; j < p1; j += FT) pk = fmaxf(pk, fabsf(buf[j] - lmean));
    red[tid] = pk;
    __syncthreads();
    for (int k = FT / 2; k > 0; k >>= 1) {
        if (tid < k) red[tid] = fmaxf(red[tid], red[tid + k]);
        __syncthreads();
    }
    const float lpeak = red[0];
    if (!(lpeak > 0.f)) {
        if (tid == 0) {
            out.ncand[slot] = 1;
            out.lpeak[slot] = 0.f;
        }
        return;
    }
    for (int j = tid; j < W; j += FT) buf[j] = (buf[j] - lmean) * win[j];
    __syncthreads();

    // packed real FFT: z[n] = f[2n] + i f[2n+1], M = nfft / 2 points, natural order in, bit-reversed out
    c32* z = (c32*)buf;
    for (int sp = M / 2; sp >= 1; sp >>= 1) {
        const int tstep = M / sp;
        for (int q = tid; q < M / 2; q += FT) {
            const int pos = q & (sp - 1);
            const int i0 = ((q - pos) << 1) + pos, i1 = i0 + sp;
            const c32 a = z[i0], bb = z[i1], w = tw[pos * tstep];
            const c32 d = {a.x - bb.x, a.y - bb.y};
            z[i0] = {a.x + bb.x, a.y + bb.y};
            z[i1] = {d.x * w.x - d.y * w.y, d.x * w.y + d.y * w.x};
        }
        __syncthreads();
    }
    // power spectrum P_k = |X_k|^2 of the real frame from the packed bins k and M - k, re-packed for the inverse:
    // Z'_k = (P_k + P_{M-k}) + i (P_k - P_{M-k}) conj(w_k), w_k = exp(-2 pi i k / nfft)
    for (int k = tid; k <= M / 2; k += FT) {
        if (k == 0) {
            const c32 z0 = z[0];
            const float x0 = z0.x + z0.y, xm = z0.x - z0.y;
            const float P0 = x0 * x0, PM = xm * xm;
            z[0] = {P0 + PM, P0 - PM};
            continue;
        }
        const int pk_ = bitrev(k, g.log2m), pm_ = bitrev(M - k, g.log2m);
        const c32 zk = z[pk_], zm = z[pm_], w = tw[k];
        const c32 E = {0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};
        const c32 O = {0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x)};
        const c32 Tt = {O.x * w.x - O.y * w.y, O.x * w.y + O.y * w.x};
        const float ax = E.x + Tt.x, ay = E.y + Tt.y, bx = E.x - Tt.x, by = E.y - Tt.y;
        const float Pk = ax * ax + ay * ay, Pm = bx * bx + by * by;
        const float S = Pk + Pm, D = Pk - Pm;
        z[pk_] = {S + D * w.y, D * w.x};
        if (pm_ != pk_) z[pm_] = {S - D * w.y, D * w.x};
    }
    __syncthreads();
    // inverse, bit-reversed in, natural out; unnormalised (the scale cancels in a[l] / a[0])
    for (int sp = 1; sp < M; sp <<= 1) {
        const int tstep = M / sp;
        for (int q = tid; q < M / 2; q += FT) {
            const int pos = q & (sp - 1);
            const int i0 = ((q - pos) << 1) + pos, i1 = i0 + sp;
            const c32 a = z[i0], bb = z[i1], w = tw[pos * tstep];
            const c32 d = {bb.x * w.x + bb.y * w.y, bb.y * w.x - bb.x * w.y};   // bb * conj(w)
            z[i0] = {a.x + d.x, a.y + d.y};
            z[i1] = {a.x - d.x, a.y - d.y};
        }
        __syncthreads();
    }
    const float a0 = buf[0];
    __syncthreads();
    if (!(a0 > 0.f)) {
        if (tid == 0) {
            out.ncand[slot] = 1;
            out.lpeak[slot] = lpeak;
        }
        return;
    }
    for (int l = tid; l <= imax; l += FT) buf[l] = buf[l] / (a0 * hw[l]);
    __syncthreads();
    const float* r = buf;
    // peaks
    const int l_end = g.lag_max < imax ? g.lag_max : imax;
    for (int l = g.lag_min + tid; l < l_end; l += FT) {
        const float rl = r[l];
        if (rl > (float)(0.5 * kVoicing) && rl > r[l - 1] && rl >= r[l + 1]) atomicOr(&peak_bits[l >> 5], 1u << (l & 31));
    }
    __syncthreads();
    // the candidate list on wave 0: lane c holds candidate c; the peaks are visited in lag order
    if (tid < 64) {
        const int lane = tid;
        double cf = 0.0, cs = 0.0;
        int cl = 0, n = 1;
        for (int wi = g.lag_min >> 5; wi <= (l_end - 1) >> 5; ++wi) {
            unsigned bits = peak_bits[wi];
            while (bits) {
                const int l = (wi << 5) + __ffs(bits) - 1;
                bits &= bits - 1;
                const double rm = (double)r[l - 1], r0 = (double)r[l], rp = (double)r[l + 1];
                const double den = 2.0 * r0 - rm - rp;
                if (!(den > 0.0 && isfinite(den))) continue;
                const double tau = (double)l + 0.5 * (rp - rm) / den;
                const double fq = (double)g.sr / tau;
                double st = sinc_interp<64>(r, imax, tau, 30, lane);
                if (st > 1.0) st = 1.0 / st;
                if (!(fq < g.f0_max && isfinite(st))) continue;
                int place;
                if (n < g.C) {
                    place = n++;
                } else {
                    // the weakest of the list: lowest local strength, the lower slot on ties
                    double v = (lane >= 1 && lane < g.C) ? cs - kOctave * log2(g.f0_min / cf) : INFINITY;
                    int at = lane;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const double ov = __shfl_xor(v, o, 64);
                        const int oa = __shfl_xor(at, o, 64);
                        if (ov < v || (ov == v && oa < at)) {
                            v = ov;
                            at = oa;
                        }
                    }
                    place = (v < 2.0 && st - kOctave * log2(g.f0_min / fq) > v) ? at : -1;
                }
                if (lane == place) {
                    cf = fq;
                    cs = st;
                    cl = l;
                }
            }
        }
        if (lane < MAX_C) {
            cand_f[lane] = cf;
            cand_s[lane] = cs;
            cand_l[lane] = cl;
        }
        if (lane == 0) n_cand_s = n;
    }
    __syncthreads();
    // refinement: 8 lanes per candidate maximise the depth-70 interpolant on [l - 1, l + 1] (Brent: golden section and
    // parabolic steps, on the negated function)
    {
        const int n = n_cand_s, c = 1 + (tid >> 3), sub = tid & 7;
        const bool mine = c < n;
        const int l = mine ? cand_l[c] : g.lag_min + 1;
        const double golden = 1.0 - 0.6180339887498948482045868343656381177203;
        const double sqrt_eps = 1.4901161193847656e-08, tol = 1e-10;
        double a = (double)l - 1.0, bnd = (double)l + 1.0;
        double v = a + golden * (bnd - a);
        double fv = mine ? -sinc_interp<8>(r, imax, v, 70, sub) : 0.0;
        double xq = v, w = v, fx = fv, fw = fv;
        bool done = !mine;
        for (int it = 0; it < 60; ++it) {
            const double rng = bnd - a, mid = 0.5 * (a + bnd);
            const double tol_act = sqrt_eps * fabs(xq) + tol / 3.0;
            if (fabs(xq - mid) + 0.5 * rng <= 2.0 * tol_act) done = true;
            if (__all(done)) break;
            double step = golden * (xq < mid ? bnd - xq : a - xq);
            if (fabs(xq - w) >= tol_act) {
                double tt = (xq - w) * (fx - fv);
                double q = (xq - v) * (fx - fw);
                double p = (xq - v) * q - (xq - w) * tt;
                q = 2.0 * (q - tt);
                if (q > 0.0)
                    p = -p;
                else
                    q = -q;
                if (fabs(p) < fabs(step * q) && p > q * (a - xq + 2.0 * tol_act) && p < q * (bnd - xq - 2.0 * tol_act)) step = p / q;
            }
            if (fabs(step) < tol_act) step = step > 0.0 ? tol_act : -tol_act;
            const double tn = xq + step;
            const double ft = -sinc_interp<8>(r, imax, done ? xq : tn, 70, sub);
            if (done) continue;
            if (ft <= fx) {
                if (tn < xq)
                    bnd = xq;
                else
                    a = xq;
                v = w;
                w = xq;
                xq = tn;
                fv = fw;
                fw = fx;
                fx = ft;
            } else {
                if (tn < xq)
                    a = tn;
                else
                    bnd = tn;
                if (ft <= fw || w == xq) {
                    v = w;
                    w = tn;
                    fv = fw;
                    fw = ft;
                } else if (ft <= fv || v == xq || v == w) {
                    v = tn;
                    fv = ft;
                }
            }
        }
        if (mine && sub == 0) {
            double st = -fx;
            if (st > 1.0) st = 1.0 / st;
            co[2 * c] = (double)g.sr / xq;
            co[2 * c + 1] = st;
        }
        if (tid == 0) {
            out.ncand[slot] = n;
            out.lpeak[slot] = lpeak;
        }
    }
}

// ---- the path and the placement ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) path_kernel(int64_t T, const int32_t* __restrict__ n_samples, const float* __restrict__ stats,
                                                  Geo g, int64_t nF_max, FrameOut in, uint8_t* __restrict__ bp,
                                                  float* __restrict__ raw, int64_t n_frames, int64_t start_frame, int uv_interp,
                                                  float* __restrict__ out, int32_t* __restrict__ choice) {
    __shared__ uint8_t bp_s[BT * MAX_C];
    __shared__ int choice_s[BT], carry;
    __shared__ int64_t first_v[64], last_v[64];
    const int lane = threadIdx.x, b = blockIdx.x, C = g.C;
    const int64_t N = row_samples(n_samples, b, T);
    int64_t nF = row_frames(N, g.dx, g.dt, g.three_periods);
    nF = nF < 0 ? 0 : (nF > nF_max ? nF_max : nF);
    const float gpeak = stats[2 * b + 1];
    const double* cand = in.cand + (int64_t)b * nF_max * C * 2;
    const int32_t* ncand = in.ncand + (int64_t)b * nF_max;
    const float* lpk = in.lpeak + (int64_t)b * nF_max;
    uint8_t* bpr = bp + (int64_t)b * nF_max * C;
    float* rw = raw + (int64_t)b * nF_max;
    const double corr = 0.01 / g.dt, oj = kOctaveJump * corr, vu = kVuv * corr, lfmax = log2(g.f0_max);
    const bool in_c = lane < C;
    double delta = -INFINITY, lf = 0.0;
    bool voiced = false;
    double f_n = 0.0, s_n = 0.0;
    int nc_n = 1;
    float lp_n = 0.f;
    if (nF > 0) {
        if (in_c) {
            f_n = cand[2 * lane];
            s_n = cand[2 * lane + 1];
        }
        nc_n = ncand[0];
        lp_n = lpk[0];
    }
    for (int64_t i = 0; i < nF; ++i) {
        const double f = f_n, s = s_n;
        const int nc = nc_n;
        const float lp = lp_n;
        if (i + 1 < nF) {
            if (in_c) {
                f_n = cand[((i + 1) * C + lane) * 2];
                s_n = cand[((i + 1) * C + lane) * 2 + 1];
            }
            nc_n = ncand[i + 1];
            lp_n = lpk[i + 1];
        }
        const bool valid = lane < nc && in_c, v_now = valid && f > 0.0;
        const double lf_now = v_now ? log2(f) : 0.0;
        const double inten = gpeak > 0.f ? fmin(1.0, (double)lp / (double)gpeak) : 0.0;
        const double unv = kVoicing + fmax(0.0, 2.0 - inten / (kSilence / (1.0 + kVoicing)));
        const double score = v_now ? s - kOctave * (lfmax - lf_now) : unv;
        if (i == 0) {
            delta = valid ? score : -INFINITY;
        } else {
            double best = -INFINITY;
            int arg = 0;
            for (int k = 0; k < C; ++k) {
                const double dk = __shfl(delta, k, 64), lfk = __shfl(lf, k, 64);
                const bool vk = __shfl((int)voiced, k, 64) != 0;
                const double cost = (vk && v_now) ? oj * fabs(lfk - lf_now) : ((vk || v_now) ? vu : 0.0);
                const double tot = dk - cost;
                if (tot > best) {
                    best = tot;
                    arg = k;
                }
            }
            delta = valid ? best + score : -INFINITY;
            if (in_c) bpr[i * C + lane] = (uint8_t)arg;
        }
        lf = lf_now;
        voiced = v_now;
    }
    // the end of the best path: the highest delta, the lower candidate on ties
    int cur = lane;
    {
        double v = delta;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o, 64);
            const int oa = __shfl_xor(cur, o, 64);
            if (ov > v || (ov == v && oa < cur)) {
                v = ov;
                cur = oa;
            }
        }
    }
    __syncthreads();   // the back-pointers written above are read below by other lanes of this (single-wave) workgroup
    for (int64_t hi = nF; hi > 0; hi -= BT) {
        const int64_t lo = hi > BT ? hi - BT : 0;
        const int cnt = (int)(hi - lo);
        for (int e = lane; e < cnt * C; e += 64) bp_s[e] = bpr[lo * C + e];
        __syncthreads();
        if (lane == 0) {
            int c = cur;
            for (int j = cnt - 1; j >= 0; --j) {
                choice_s[j] = c;
                if (lo + j > 0) c = bp_s[j * C + c];
            }
            carry = c;
        }
        __syncthreads();
        cur = carry;
        for (int j = lane; j < cnt; j += 64) {
            const int c = choice_s[j];
            rw[lo + j] = (float)cand[((lo + j) * C + c) * 2];
            if (choice) choice[(int64_t)b * nF_max + lo + j] = c;
        }
        __syncthreads();
    }
    if (choice)
        for (int64_t j = nF + lane; j < nF_max; j += 64) choice[(int64_t)b * nF_max + j] = 0;
    // placement: `pad` zeros, the nF frames, zeros to the row's own frame count; 0 after it
    float* o = out + (int64_t)b * n_frames;
    int64_t n_out = n_frames;
    if (n_samples) {
        n_out = (int64_t)floor((double)N / g.hop) + 1;
        n_out = n_out < 0 ? 0 : (n_out > n_frames ? n_frames : n_out);
    }
    const int64_t body = (int64_t)floor((double)N / g.hop) - nF + 1;
    const int64_t pad = start_frame + (body >= 0 ? body / 2 : -((-body + 1) / 2));
    for (int64_t n = lane; n < n_frames; n += 64) {
        const int64_t k = n - pad;
        o[n] = (n < n_out && k >= 0 && k < nF) ? rw[k] : 0.f;
    }
    if (!uv_interp) return;
    __syncthreads();
    const int64_t chunk = (n_out + 63) / 64, c0 = lane * chunk < n_out ? lane * chunk : n_out;
    const int64_t c1 = c0 + chunk < n_out ? c0 + chunk : n_out;
    int64_t fv = n_out, lv = -1;
    for (int64_t k = c0; k < c1; ++k)
        if (o[k] != 0.f) {
            if (fv == n_out) fv = k;
            lv = k;
        }
    first_v[lane] = fv;
    last_v[lane] = lv;
    __syncthreads();
    int64_t prev = -1, next = n_out, any = n_out;
    for (int u = 0; u < 64; ++u) {
        if (u < lane) prev = last_v[u] > prev ? last_v[u] : prev;
        if (u > lane) next = first_v[u] < next ? first_v[u] : next;
        any = first_v[u] < any ? first_v[u] : any;
    }
    if (any < n_out) {
        // numpy.interp over the zero frames: runs [k, e) of zeros between voiced neighbours xl < k and xr >= e
        int64_t k = c0;
        while (k < c1) {
            if (o[k] != 0.f) {
                prev = k;
                ++k;
                continue;
            }
            int64_t e = k;
            while (e < c1 && o[e] == 0.f) ++e;
            const int64_t xr = e < c1 ? e : next, xl = prev;
            for (int64_t q = k; q < e; ++q) {
                double v;
                if (xl < 0) {
                    v = (double)o[xr];
                } else if (xr >= n_out) {
                    v = (double)o[xl];
                } else {
                    const double yl = (double)o[xl], yr = (double)o[xr];
                    const double slope = (yr - yl) / ((double)xr - (double)xl);
                    v = slope * ((double)q - (double)xl) + yl;
                }
                o[q] = (float)v;
            }
            k = e;
        }
    }
    __syncthreads();
    for (int64_t k = c0; k < c1; ++k)
        if (o[k] < (float)g.f0_min) o[k] = (float)g.f0_min;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int get_table(ddsp_ctx* ctx, hipStream_t st, const Geo& g, float** out) {
    for (int i = 0; i < ctx->n_tables; ++i) {
        ddsp_table& t = ctx->tables[i];
        if (t.kind == TAB_F0_AC && t.n0 == g.W && t.n1 == g.nfft) {
            *out = t.dev;
            return DDSP_OK;
        }
    }
    if (ctx->n_tables >= 64) return ddsp_fail(ctx, DDSP_ERR_OOM, "table cache full", "");
    const size_t elems = (size_t)g.hw_ld + g.win_ld + g.nfft;
    float* dev = nullptr;
    hipError_t e = hipMalloc((void**)&dev, elems * sizeof(float));
    if (e != hipSuccess) return ddsp_fail(ctx, DDSP_ERR_OOM, "table hipMalloc", hipGetErrorString(e));
    const int rest = g.W > g.nfft / 2 ? g.W : g.nfft / 2;
    hipLaunchKernelGGL(table_kernel, dim3((unsigned)(g.imax + 1 + (rest + 255) / 256)), dim3(256), 0, st, dev, g.W, g.imax, g.nfft,
                       g.hw_ld, g.win_ld);
    DDSP_LAUNCH_CHECK(ctx);
    ddsp_table& t = ctx->tables[ctx->n_tables++];
    t.kind = TAB_F0_AC;
    t.n0 = g.W;
    t.n1 = g.nfft;
    t.dev = dev;
    t.bytes = elems * sizeof(float);
    *out = dev;
    return DDSP_OK;
}

}  // namespace

extern "C" int64_t ddsp_f0_ac_frames(int64_t T, int sr, double hop, double f0_min) {
    if (T < 0 || sr < 1 || !(hop > 0.0) || !(f0_min > 0.0)) return -1;
    const int64_t n = row_frames(T, 1.0 / sr, hop / sr, 3.0 / f0_min);
    return n < 0 ? 0 : n;
}

// n_samples == nullptr: every row holds T samples; with counts start_frame is 0
extern "C" int ddsp_f0_ac(ddsp_ctx* ctx, void* stream, const float* audio, int64_t B, int64_t T, const int32_t* n_samples, int sr,
                          double hop, double f0_min, double f0_max, int64_t n_frames, int64_t start_frame, int uv_interp, float* out,
                          int32_t* choice) {
    DDSP_REQUIRE(ctx, ctx && (!n_samples || start_frame == 0), "ddsp_f0_ac: start_frame must be 0 with n_samples (a ragged batch)");
    DDSP_REQUIRE(ctx, ctx && audio && out, "ddsp_f0_ac: null argument");
    Geo g;
    DDSP_REQUIRE(ctx, make_geo(sr, hop, f0_min, f0_max, g),
                 "ddsp_f0_ac: needs sr, hop > 0, 0 < f0_min < f0_max <= 32 * f0_min and a window of 64 samples to an FFT of 8192");
    const int64_t nF_max = row_frames(T, g.dx, g.dt, g.three_periods);
    DDSP_REQUIRE(ctx, B >= 1 && B < 65536 && T >= 1 && T < ((int64_t)1 << 31), "ddsp_f0_ac: bad shape");
    DDSP_REQUIRE(ctx, nF_max >= 1, "ddsp_f0_ac: the audio is shorter than one analysis window (3 / f0_min seconds)");
    DDSP_REQUIRE(ctx, nF_max < ((int64_t)1 << 31) / (2 * MAX_C) / B, "ddsp_f0_ac: too many frames");
    DDSP_REQUIRE(ctx, n_frames >= 1 && start_frame >= 0 && start_frame <= n_frames, "ddsp_f0_ac: bad frame counts");
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    float* tab = nullptr;
    int rc = get_table(ctx, st, g, &tab);
    if (rc) return rc;
    const size_t rows = (size_t)B * nF_max;
    const size_t sz[6] = {align256((size_t)B * 2 * 4), align256(rows * g.C * 2 * 8), align256(rows * 4), align256(rows * 4),
                          align256(rows * g.C), align256(rows * 4)};
    size_t total = 0;
    for (size_t s : sz) total += s;
    if ((rc = ddsp_scratch_reserve_bytes(ctx, total + 4096))) return rc;
    ddsp_scratch_reset(ctx);
    char* arena = nullptr;
    if ((rc = ddsp_scratch_get(ctx, total, (void**)&arena))) return rc;
    float* stats = (float*)arena;
    FrameOut fo;
    fo.cand = (double*)(arena + sz[0]);
    fo.ncand = (int32_t*)(arena + sz[0] + sz[1]);
    fo.lpeak = (float*)(arena + sz[0] + sz[1] + sz[2]);
    uint8_t* bp = (uint8_t*)(arena + sz[0] + sz[1] + sz[2] + sz[3]);
    float* raw = (float*)(arena + sz[0] + sz[1] + sz[2] + sz[3] + sz[4]);
    hipLaunchKernelGGL(stats_kernel, dim3((unsigned)B), dim3(256), 0, st, audio, T, n_samples, stats);
    hipLaunchKernelGGL(frame_kernel, dim3((unsigned)nF_max, (unsigned)B), dim3(FT), (size_t)g.nfft * sizeof(float), st, audio, T,
                       n_samples, stats, tab, g, nF_max, fo);
    hipLaunchKernelGGL(path_kernel, dim3((unsigned)B), dim3(64), 0, st, T, n_samples, stats, g, nF_max, fo, bp, raw, n_frames,
                       start_frame, uv_interp ? 1 : 0, out, choice);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
