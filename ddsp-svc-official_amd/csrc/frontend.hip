// SURVEY 8(f) rank 2 - the two device-side steps immediately BEFORE the synthesis path that need no pretrained model:
//   * frame-wise RMS volume (`Volume_Extractor.extract`, ddsp/vocoder.py:116-137): reflect-pad by (hop//2, (hop+1)//2),
//     mean of squares over non-overlapping blocks [int(n*hop), int((n+1)*hop)), square root; int(T//hop) + 1 frames - for
//     an integral hop and for the fractional one a device at another rate than the model's gives (main.py:72,109);
//   * nearest-frame alignment of encoder units to the synthesiser's frame rate (`Units_Encoder.encode`,
//     ddsp/vocoder.py:201-211): frame i takes unit row min(rint(fp32(ratio) * i), Lu - 1), rint = half to even.
// Both are HBM-bound streaming kernels: 4 B read per sample / 8 B per copied feature.
#include "common.h"

#include <algorithm>

namespace {

// one wavefront per (utterance, frame).  Block n is padded[int(n*h) : min(int((n+1)*h), Tp)] of the signal reflect-padded
// by pad_l in front (Tp = padded length), bounds in fp64 like the reference's Python floats; its mean divides by the
// block's own length.  An integral hop gives start n*hop and length hop exactly, so both entry points share this kernel.
// Ragged batch (n_samples != nullptr, integral hop): row b is its first n_samples[b] samples - it reflects at its own end,
// has n_samples[b] / hop + 1 frames and 0 in the frames after them; what follows its samples is never read.
__global__ void __launch_bounds__(256) volume_kernel(const float* __restrict__ audio, int64_t T, double hop, int64_t pad_l,
                                                     int64_t Tp, int64_t n_frames, int64_t total, float* __restrict__ vol,
                                                     const int32_t* __restrict__ n_samples) {
    const int lane = threadIdx.x & 63;
    const int64_t fidx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fidx >= total) return;
    const int64_t b = fidx / n_frames, n = fidx - b * n_frames;
    const float* x = audio + b * T;
    if (n_samples) {
        const int64_t pad = Tp - T, nb = n_samples[b];
        T = nb < 1 ? 1 : (nb < T ? nb : T);
        Tp = T + pad;
        if (n >= T / (int64_t)hop + 1) {
            if (lane == 0) vol[fidx] = 0.f;
            return;
        }
    }
    const int64_t start = (int64_t)((double)n * hop);
    int64_t end = (int64_t)((double)(n + 1) * hop);
    end = end < Tp ? end : Tp;                        // numpy truncates the slice at the padded length
    const int64_t len = end - start;
    const int64_t first = start - pad_l;              // index of the block's first sample in the UNpadded signal
    double s = 0.0;                                   // (numpy sums the fp32 squares pairwise; fp64 is at least as close)
    for (int64_t j = lane; j < len; j += 64) {
        int64_t i = first + j;
        if (i < 0) i = -i;                            // numpy 'reflect': edge sample not repeated
        if (i >= T) i = 2 * (T - 1) - i;
        if (n_samples) i = i < 0 ? 0 : (i < T ? i : T - 1);   // (a count below the caller's bound: stay inside the row)
        const float v = x[i];
        s += (double)(v * v);                         // the square is rounded to fp32 first, like `audio ** 2`
    }
    s = wave_sum_d(s);
    if (lane == 0) vol[fidx] = sqrtf((float)(s / (double)len));
}

// one wavefront per output row (utterance, frame).  Ragged batch (n_units != nullptr): row b has n_out[b] frames of its own,
// gathered from its own n_units[b] unit rows (the source index stops at n_units[b] - 1), and zeros after them.
__global__ void __launch_bounds__(256) align_units_kernel(const float* __restrict__ units, int64_t Lu, int64_t C,
                                                          int64_t n_frames, float ratio, int64_t total,
                                                          float* __restrict__ out, const int32_t* __restrict__ n_units,
                                                          const int32_t* __restrict__ n_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total) return;
    const int64_t b = row / n_frames, i = row - b * n_frames;
    float* d = out + row * C;
    const bool vec = (C & 3) == 0 && (((uintptr_t)units | (uintptr_t)out) & 15) == 0;
    int64_t last = Lu - 1;
    if (n_units) {
        if (i >= (int64_t)n_out[b]) {
            if (vec) {
                for (int64_t c = 4 * lane; c < C; c += 256) *(f32x4*)(d + c) = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
                for (int64_t c = lane; c < C; c += 64) d[c] = 0.f;
            }
            return;
        }
        const int64_t lb = (int64_t)n_units[b] - 1;
        last = lb < last ? lb : last;
    }
    int64_t src = (int64_t)rintf(__fmul_rn(ratio, (float)i));     // torch.round of an fp32 product: half to even
    src = src < last ? src : last;
    src = src < 0 ? 0 : src;
    const float* s = units + (b * Lu + src) * C;
    if (vec) {
        for (int64_t c = 4 * lane; c < C; c += 256) *(f32x4*)(d + c) = *(const f32x4*)(s + c);
    } else {
        for (int64_t c = lane; c < C; c += 64) d[c] = s[c];
    }
}

// f0 track re-timed for the enhancer (enhancer.py:56-62): out[i] = numpy.interp(i * step_dst, knots j * step_num / div,
// fl32(f0[j] * scale)) with the end values held outside the knots; one thread per output frame, fp64 like numpy.  Ragged batch
// (ns != nullptr): blockIdx.y is the row, with ns[b] <= n_src knots and nd[b] <= n_dst targets of its own - the ends are held
// at the row's own first and last frame, what follows them in f0 is not read, and the outputs from nd[b] on are 0.  Keyed batch
// (key != nullptr, a ragged one): the row's (div, scale) are entry key[b] of two device tables of n_keys entries, the key clamped
// into them.
__global__ void __launch_bounds__(256) retime_f0_kernel(const float* __restrict__ f0, int64_t n_src, double step_num, double div,
                                                        float scale, double step_dst, int64_t n_dst, float* __restrict__ out,
                                                        const int32_t* __restrict__ ns, const int32_t* __restrict__ nd,
                                                        const int32_t* __restrict__ key, const double* __restrict__ div_tab,
                                                        const float* __restrict__ scale_tab, int n_keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_dst) return;
    if (ns) {
        const int64_t b = blockIdx.y;
        if (key) {
            int k = key[b];
            k = k < 0 ? 0 : (k >= n_keys ? n_keys - 1 : k);
            div = div_tab[k];
            scale = scale_tab[k];
        }
        f0 += b * n_src;
        out += b * n_dst;
        if (i >= (int64_t)nd[b]) {
            out[i] = 0.f;
            return;
        }
        const int64_t nb = ns[b];
        n_src = nb < 1 ? 1 : (nb < n_src ? nb : n_src);
    }
    auto knot = [&](int64_t j) { return (step_num * (double)j) / div; };              // (hop / sr) * arange(n) / real_factor
    auto val = [&](int64_t j) { return (double)__fmul_rn(f0[j], scale); };            // the fp32 in-place `f0_np *= real_factor`
    const double x = step_dst * (double)i;
    double y;
    if (n_src == 1 || x <= knot(0)) {
        y = val(0);
    } else if (x >= knot(n_src - 1)) {
        y = val(n_src - 1);
    } else {
        int64_t j = (int64_t)(x * div / step_num);
        j = j < 0 ? 0 : (j > n_src - 2 ? n_src - 2 : j);
        while (j > 0 && knot(j) > x) --j;
        while (j < n_src - 2 && knot(j + 1) <= x) ++j;
        const double slope = (val(j + 1) - val(j)) / (knot(j + 1) - knot(j));
        y = slope * (x - knot(j)) + val(j);
    }
    out[i] = (float)y;
}

}  // namespace

// ddsp_retime_f0 and its keyed form: ns == nd == nullptr is one track (B = 1, every knot and target)
static int retime_f0_go(ddsp_ctx* ctx, void* stream, const float* f0, int64_t B, int64_t n_src, const int32_t* ns, double step_num,
                        double div, float scale, double step_dst, int64_t n_dst, const int32_t* nd, float* out,
                        const int32_t* key = nullptr, const double* div_tab = nullptr, const float* scale_tab = nullptr,
                        int n_keys = 0) {
    DDSP_REQUIRE(ctx, ctx && f0 && out, "ddsp_retime_f0: null argument");
    DDSP_REQUIRE(ctx, B >= 1 && B <= 65535 && n_src >= 1 && n_dst >= 0 && step_num > 0 && div > 0 && step_dst > 0,
                 "ddsp_retime_f0: bad shape or step");
    if (n_dst == 0) return DDSP_OK;
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    hipLaunchKernelGGL(retime_f0_kernel, dim3((unsigned)ceil_div64(n_dst, 256), (unsigned)B), dim3(256), 0, st, f0, n_src, step_num, div,
                       scale, step_dst, n_dst, out, ns, nd, key, div_tab, scale_tab, n_keys);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_retime_f0(ddsp_ctx* ctx, void* stream, const float* f0, int64_t B, int64_t n_src, const int32_t* n_src_rows,
                              double step_num, double div, float scale, double step_dst, int64_t n_dst, const int32_t* n_dst_rows,
                              float* out) {
    DDSP_REQUIRE(ctx, ctx && !n_src_rows == !n_dst_rows, "ddsp_retime_f0: n_src_rows and n_dst_rows are given together or not at all");
    // (the kernel finds a row by its counts: without them there is one track)
    DDSP_REQUIRE(ctx, n_src_rows ? n_dst >= 1 : B == 1, "ddsp_retime_f0: a batch needs n_dst >= 1 and its counts, one track B = 1");
    return retime_f0_go(ctx, stream, f0, B, n_src, n_src_rows, step_num, div, scale, step_dst, n_dst, n_dst_rows, out);
}

extern "C" int ddsp_retime_f0_keyed(ddsp_ctx* ctx, void* stream, const float* f0, int64_t B, int64_t n_src, const int32_t* n_src_rows,
                                    double step_num, const int32_t* key, int n_keys, const double* div_by_key,
                                    const float* scale_by_key, double step_dst, int64_t n_dst, const int32_t* n_dst_rows, float* out) {
    DDSP_REQUIRE(ctx, ctx && n_src_rows && n_dst_rows && key && div_by_key && scale_by_key, "ddsp_retime_f0_keyed: null argument");
    DDSP_REQUIRE(ctx, n_dst >= 1 && n_keys >= 1, "ddsp_retime_f0_keyed: bad shape or table");
    // (the tables live on the device: their entries are the caller's to keep positive, as `div` is checked in the other forms)
    return retime_f0_go(ctx, stream, f0, B, n_src, n_src_rows, step_num, 1.0, 1.f, step_dst, n_dst, n_dst_rows, out, key, div_by_key,
                        scale_by_key, n_keys);
}

// The enhancer's key of every row, decided on the device (enhancer.py:34-38 without its read-back): one wave per row takes
// the highest f0 of the frames from `cut` on, forms q = fl32(f0max / 760) and returns the first k with q <= thr[k], thr[k]
// being the largest fp32 value <= 2^(k/12) (a host table) - the comparison form of ceil(12 log2 q) <= k, which needs no
// device log2.  request[b] >= 0 is a fixed key instead; both are clamped to max_key.
namespace {
__global__ void __launch_bounds__(64) enhancer_keys_kernel(const float* __restrict__ f0, int64_t Fr, int64_t cut, int max_key,
                                                           const int32_t* __restrict__ request, const float* __restrict__ thr,
                                                           int32_t* __restrict__ key) {
    const int64_t b = blockIdx.x;
    const int want = request[b];
    if (want >= 0) {
        if (threadIdx.x == 0) key[b] = want > max_key ? max_key : want;
        return;
    }
    float m = -INFINITY;
    for (int64_t i = cut + threadIdx.x; i < Fr; i += 64) m = fmaxf(m, f0[b * Fr + i]);
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (threadIdx.x != 0) return;
    int k = 0;
    if (m > 0.f) {
        const float q = __fdiv_rn(m, 760.f);
        while (k < max_key && !(q <= thr[k])) ++k;
    }
    key[b] = k;
}
}  // namespace

extern "C" int ddsp_enhancer_keys(ddsp_ctx* ctx, void* stream, const float* f0, int64_t S, int64_t Fr, int64_t cut_frames, int max_key,
                                  const int32_t* request, const float* thresholds, int32_t* key) {
    DDSP_REQUIRE(ctx, ctx && f0 && request && thresholds && key, "ddsp_enhancer_keys: null argument");
    DDSP_REQUIRE(ctx, S >= 1 && S <= (1 << 20) && Fr >= 1 && cut_frames >= 0 && cut_frames < Fr && max_key >= 0 && max_key <= 12,
                 "ddsp_enhancer_keys: bad shape, cut or max_key (0..12; thresholds holds max_key + 1 values)");
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    hipLaunchKernelGGL(enhancer_keys_kernel, dim3((unsigned)S), dim3(64), 0, st, f0, Fr, cut_frames, max_key, request, thresholds, key);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// The conversion leg of validation (solver.py:46-54) without its host round trip: per row the target speaker follows from the
// source id - (src + 1) % n_spk, and 0 becomes 1 - and the f0 is mapped between the two speakers' log-f0 statistics,
// out = exp(lfo[tgt] * ln(f0) / lfo[src]) in fp32 in the reference's order of operations.  f0 == 0 (unvoiced) gives exactly 0
// (there: exp(-inf)), frames at or after a row's count are written as 0 and not read.  A source id outside [1, n_spk] is not
// used as an index: the row comes out as zeros with target 0 and the context's device error word is set.
namespace {
__global__ void __launch_bounds__(256) vc_f0_map_kernel(const float* __restrict__ f0, const int64_t* __restrict__ src,
                                                        const float* __restrict__ lfo, int n_spk, int64_t Fr,
                                                        const int32_t* __restrict__ n_frames, float* __restrict__ out,
                                                        int64_t* __restrict__ tgt, int* __restrict__ err) {
    const int64_t b = blockIdx.y;
    const int64_t s = src[b];
    const bool ok = s >= 1 && s <= n_spk;
    int64_t t = ok ? (s + 1) % n_spk : 0;
    if (ok && t == 0) t = 1;                       // 1 <= t <= max(1, n_spk - 1)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        tgt[b] = t;
        if (!ok) __hip_atomic_store(err, DDSP_DEV_ERR_SPK_ID, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    int64_t nb = n_frames ? (int64_t)n_frames[b] : Fr;
    nb = !ok ? 0 : nb < 0 ? 0 : nb > Fr ? Fr : nb;
    const float ls = ok ? lfo[s - 1] : 1.f, lt = ok ? lfo[t - 1] : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < Fr; i += (int64_t)gridDim.x * 256) {
        float v = 0.f;
        if (i < nb) {
            const float f = f0[b * Fr + i];
            if (f > 0.f) v = expf(__fdiv_rn(lt * logf(f), ls));
        }
        out[b * Fr + i] = v;
    }
}
}  // namespace

extern "C" int ddsp_vc_f0_map(ddsp_ctx* ctx, void* stream, const float* f0, const int64_t* src_spk, const float* lfo, int n_spk,
                              int64_t B, int64_t Fr, const int32_t* n_frames, float* f0_out, int64_t* tgt_spk) {
    DDSP_REQUIRE(ctx, ctx && f0 && src_spk && lfo && f0_out && tgt_spk, "ddsp_vc_f0_map: null argument");
    DDSP_REQUIRE(ctx, B >= 1 && B <= 65535 && Fr >= 1 && n_spk >= 1, "ddsp_vc_f0_map: bad shape");
    int rc;
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;
    const unsigned gx = (unsigned)std::min<int64_t>(ceil_div64(Fr, 256), 64);
    hipLaunchKernelGGL(vc_f0_map_kernel, dim3(gx, (unsigned)B), dim3(256), 0, st, f0, src_spk, lfo, n_spk, Fr, n_frames, f0_out,
                       tgt_spk, dev_err);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// Python's float floor division `a // b` (CPython float_floor_div: fmod, exact quotient of the remainder-free part, floor,
// round-half correction), so that frame counts and pads equal the reference's `int(T // h)` / `int(h // 2)` bit for bit
static double py_floordiv(double a, double b) {
    double mod = fmod(a, b);
    double div = (a - mod) / b;
    if (mod != 0.0 && ((b < 0) != (mod < 0))) div -= 1.0;
    if (div == 0.0) return copysign(0.0, a / b);
    double fl = floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return fl;
}

static int volume_launch(ddsp_ctx* ctx, hipStream_t st, const float* audio, int64_t B, int64_t T, double hop, int64_t n_frames,
                         int64_t pad_l, int64_t pad_r, float* volume, const int32_t* n_samples) {
    DDSP_ENTER_DEVICE(ctx);
    const int64_t total = B * n_frames;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(volume_kernel, dim3((unsigned)ceil_div64(total, 4)), dim3(256), 0, st, audio, T, hop, pad_l,
                       T + pad_l + pad_r, n_frames, total, volume, n_samples);
    ddsp_prof_end(ctx, st, 2.0 * B * T, 4.0 * (B * (double)T + total));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// n_samples == nullptr is the rectangular batch
extern "C" int ddsp_volume_extract(ddsp_ctx* ctx, void* stream, const float* audio, int64_t B, int64_t T, const int32_t* n_samples,
                                   int hop, float* volume) {
    DDSP_REQUIRE(ctx, ctx && audio && volume, "ddsp_volume_extract: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && hop >= 1 && hop <= (1 << 20), "ddsp_volume_extract: bad shape");
    // numpy's reflect padding needs the pad (at most (hop+1)/2) to be smaller than the signal
    DDSP_REQUIRE(ctx, T > (hop + 1) / 2, "ddsp_volume_extract: signal shorter than the reflect padding");
    if (B == 0) return DDSP_OK;
    return volume_launch(ctx, (hipStream_t)stream, audio, B, T, (double)hop, T / hop + 1, hop / 2, (hop + 1) / 2, volume, n_samples);
}

extern "C" int ddsp_volume_extract_frac(ddsp_ctx* ctx, void* stream, const float* audio, int64_t B, int64_t T, double hop_size,
                                        float* volume) {
    DDSP_REQUIRE(ctx, ctx && audio && volume, "ddsp_volume_extract_frac: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && T >= 0 && hop_size >= 1.0 && hop_size <= (double)(1 << 20),
                 "ddsp_volume_extract_frac: bad shape or hop");       // (also refuses a NaN hop)
    const int64_t pad_l = (int64_t)py_floordiv(hop_size, 2.0), pad_r = (int64_t)py_floordiv(hop_size + 1.0, 2.0);
    DDSP_REQUIRE(ctx, T > pad_r, "ddsp_volume_extract_frac: signal shorter than the reflect padding");
    if (B == 0) return DDSP_OK;
    const int64_t n_frames = (int64_t)py_floordiv((double)T, hop_size) + 1;
    return volume_launch(ctx, (hipStream_t)stream, audio, B, T, hop_size, n_frames, pad_l, pad_r, volume, nullptr);
}

// n_units == n_out == nullptr is the rectangular batch
extern "C" int ddsp_align_units(ddsp_ctx* ctx, void* stream, const float* units, int64_t B, int64_t Lu, int64_t C,
                                int64_t n_frames, float ratio, const int32_t* n_units, const int32_t* n_out, float* out) {
    DDSP_REQUIRE(ctx, ctx && units && out, "ddsp_align_units: null argument");
    DDSP_REQUIRE(ctx, !n_units == !n_out, "ddsp_align_units: n_units and n_out are given together or not at all");
    DDSP_REQUIRE(ctx, B >= 0 && Lu >= 1 && C >= 1 && n_frames >= 0 && ratio >= 0.f && ratio == ratio,
                 "ddsp_align_units: bad shape or ratio");
    if (B == 0 || n_frames == 0) return DDSP_OK;
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    const int64_t total = B * n_frames;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(align_units_kernel, dim3((unsigned)ceil_div64(total, 4)), dim3(256), 0, st, units, Lu, C, n_frames,
                       ratio, total, out, n_units, n_out);
    ddsp_prof_end(ctx, st, 0.0, 8.0 * total * (double)C);
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
