// The silence slicer (reference: `slicer.py`, `Slicer.slice`): frame RMS as librosa.feature.rms documents it, then the
// reference's tagging state machine and chunk assembly, for a solo row or a ragged batch (B, T) with per-row sample counts in
// a device array that is never read back.
//
// Frame RMS.  Frame i of a row of n samples covers [i * hop - win / 2, +win); a sample outside [0, n) is 0 ('constant') or
// the sample numpy's 'reflect' rule names - a SELECT by a bounds test, so the padding of a ragged row (t >= n) is never read.
// A workgroup owns a tile of consecutive frames, stages the squares of the tile's span ((frames - 1) * hop + win samples) in
// the LDS once - 16-byte loads from the first 16-byte boundary at or below the span's start wherever the four samples lie
// inside the row, the scalar select at the row's start and tail - and sums every frame of the tile from there in fp64
// (fp32 products): a frame overlaps up to four hops, so each sample is read from memory once per tile, not once per frame.
// A window that does not fit the staging area (win > 12280 samples) is summed straight from memory, one frame per wave.
//
// Tagging.  One wave per row.  64 frames per step: a ballot of `rms < threshold`, run starts and ends from the mask with
// wave-uniform bit operations, the serial decisions per silent run (not per frame), every argmin over a range as a wave
// reduction that returns the lowest index among equal minima (numpy's), and the chunks written as the tags appear.
//
// Capacity of the chunk table (the binding derives it): a tag is appended when a silent run ends (or at the end of the row),
// and needs that run to hold min_interval frames - or the leading rule, which needs the run to start at frame 0 and so fires
// once.  Runs are disjoint, so a row of F frames has K <= F / min_interval + 1 tags, and K tags make at most 2 K + 1 chunks:
// one voiced chunk in front of every tag, the K silence chunks, one voiced chunk behind the last.
#include "common.h"

namespace {

constexpr int RMS_THREADS = 256;
constexpr int RMS_LDS_FLOATS = 12288;   // 48 KiB of the CU's 160: three workgroups per CU
constexpr int RMS_MAX_TILE = 64;        // frames per tile at small hops (enough workgroups for a short file)

struct RmsArgs {
    const float* x;
    const int32_t* n_samples;   // (B,) or null: T for every row
    int64_t T;
    int win, hop, pad_mode;
    int F_max, tile;
    float* rms;
};

__host__ __device__ __forceinline__ int slicer_frames(int64_t n, int win, int hop) {
    return (int)(1 + (n + 2 * (win / 2) - win) / hop);
}

__device__ __forceinline__ int row_samples(const int32_t* __restrict__ n_samples, int64_t b, int64_t T) {
    if (!n_samples) return (int)T;
    const int n = n_samples[b];
    return n < 1 ? 1 : (n > T ? (int)T : n);
}

// sample j of the padded view of row[0, n): the row's own sample inside, else the pad rule - an index outside [0, n) is
// never formed
__device__ __forceinline__ float padded_sample(const float* __restrict__ row, int64_t j, int n, int pad_mode) {
    if (j >= 0 && j < n) return row[j];
    if (pad_mode == DDSP_SLICER_PAD_CONSTANT) return 0.f;
    if (n == 1) return row[0];
    const int64_t p = 2 * ((int64_t)n - 1);
    int64_t m = j % p;
    if (m < 0) m += p;
    return row[m < n ? m : p - m];
}

// grid (tiles, B).  STAGED: the tile's squares go through the LDS; else one frame per wave straight from memory
template <bool STAGED>
__global__ void __launch_bounds__(RMS_THREADS) slicer_rms_kernel(RmsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sq[];
    const int64_t b = blockIdx.y;
    const int n = row_samples(a.n_samples, b, a.T);
    const int F = slicer_frames(n, a.win, a.hop);
    const int f0 = blockIdx.x * a.tile;
    const int nf = min(a.tile, a.F_max - f0);        // frames of this tile in the output
    const int nfv = min(nf, F - f0);                 // ... that the row has (<= 0: the tile lies behind the row's frames)
    const float* __restrict__ row = a.x + b * a.T;
    float* __restrict__ out = a.rms + b * a.F_max + f0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (nfv <= 0) {
        for (int f = tid; f < nf; f += RMS_THREADS) out[f] = 0.f;
        return;
    }
    const int64_t g0 = (int64_t)f0 * a.hop - a.win / 2;   // the row sample the tile's span starts at (may be negative)
    int off = 0;
    if constexpr (STAGED) {
        // sq[k] = square of padded sample ga + k, ga = g0 moved down to a 16-byte boundary of the address
        off = (int)((((int64_t)((uintptr_t)row >> 2)) + g0) & 3);
        const int64_t ga = g0 - off;
        const int span = off + (nfv - 1) * a.hop + a.win;
        for (int k = 4 * tid; k < span; k += 4 * RMS_THREADS) {
            const int64_t s = ga + k;
            f32x4 v;
            if (s >= 0 && s + 3 < n) {
                v = *(const f32x4*)(row + s);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = padded_sample(row, s + e, n, a.pad_mode);
            }
            *(f32x4*)(sq + k) = v * v;
        }
        __syncthreads();
    }
    for (int f = wave; f < nf; f += RMS_THREADS / 64) {
        if (f >= nfv) {
            if (lane == 0) out[f] = 0.f;
            continue;
        }
        double acc = 0.0;
        if constexpr (STAGED) {
            const float* s = sq + off + f * a.hop;
            for (int k = lane; k < a.win; k += 64) acc += (double)s[k];
        } else {
            const int64_t s = g0 + (int64_t)f * a.hop;
            for (int k = lane; k < a.win; k += 64) {
                const float v = padded_sample(row, s + k, n, a.pad_mode);
                acc += (double)(v * v);
            }
        }
        acc = wave_sum_d(acc);
        if (lane == 0) out[f] = (float)sqrt(acc / (double)a.win);
    }
}

struct TagArgs {
    const float* rms;           // (B, F_max)
    const int32_t* n_samples;
    int64_t T;
    int win, hop, F_max;
    double threshold;
    int min_length, min_interval, max_sil_kept;
    int32_t* table;             // (B, capacity, 3)
    int32_t* count;             // (B,)
    int capacity;
    int* err;
};

// lowest index of the minimum of r[lo, hi) (hi > lo), the same in every lane; a NaN counts as the smallest value (numpy's
// argmin returns the first NaN)
__device__ __forceinline__ int wave_argmin(const float* __restrict__ r, int lo, int hi, int lane) {
    constexpr int NONE = 0x7fffffff;
    float best = 0.f;
    int bi = NONE;
    for (int j = lo + lane; j < hi; j += 64) {
        float v = r[j];
        v = (v != v) ? -1.f : v;
        if (bi == NONE || v < best) {
            best = v;
            bi = j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != NONE && (bi == NONE || ob < best || (ob == best && oi < bi))) {
            best = ob;
            bi = oi;
        }
    }
    return bi == NONE ? lo : bi;
}

// The chunk table of one row, written as the tags appear (every value is the same in all lanes; lane 0 stores)
struct ChunkWriter {
    int32_t* table;
    int capacity, hop, n, lane;
    int count = 0, tags = 0, last_end = 0;
    bool overflow = false;

    __device__ __forceinline__ void chunk(int64_t start, int64_t end, int silence) {
        if (count >= capacity) {
            overflow = true;
            return;
        }
        if (lane == 0) {
            table[3 * count] = (int32_t)start;
            table[3 * count + 1] = (int32_t)end;
            table[3 * count + 2] = silence;
        }
        ++count;
    }
    __device__ __forceinline__ int64_t clipped(int frame) const {
        const int64_t s = (int64_t)frame * hop;
        return s < n ? s : n;
    }
    // the tag (a, b) in frames: the voiced chunk in front of it (none in front of a first tag that starts at 0), then its own
    __device__ __forceinline__ void tag(int a, int b) {
        if (tags == 0) {
            if (a != 0) chunk(0, clipped(a), 0);
        } else {
            chunk((int64_t)last_end * hop, clipped(a), 0);
        }
        chunk((int64_t)a * hop, clipped(b), 1);
        last_end = b;
        ++tags;
    }
    __device__ __forceinline__ void close() {
        if (tags == 0) chunk(0, n, 0);
        else if ((int64_t)last_end * hop < n) chunk((int64_t)last_end * hop, n, 0);
    }
};

// grid (B), one wave per row
__global__ void __launch_bounds__(64) slicer_tag_kernel(TagArgs a) {
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const int n = row_samples(a.n_samples, b, a.T);
    const int F = slicer_frames(n, a.win, a.hop);
    const float* __restrict__ r = a.rms + b * a.F_max;
    const int M = a.max_sil_kept, MI = a.min_interval, ML = a.min_length;
    ChunkWriter w{a.table + b * (int64_t)a.capacity * 3, a.capacity, a.hop, n, lane};

    if (n > ML) {   // (a sample count against a frame count: the reference's early return, `slicer.py:32`)
        int start = -1, clip = 0;   // the open silent run's first frame (-1: none) and the reference's clip_start
        float cur = lane < F ? r[lane] : 0.f;
        for (int base = 0; base < F; base += 64) {
            const float nxt = base + 64 + lane < F ? r[base + 64 + lane] : 0.f;   // (the next step's load, issued early)
            const int nv = min(64, F - base);
            const uint64_t valid = nv == 64 ? ~0ull : (1ull << nv) - 1;
            const uint64_t silent = __ballot((double)cur < a.threshold) & valid;
            const uint64_t voiced = ~silent & valid;
            int p = 0;
            while (p < 64) {
                const uint64_t m = (start < 0 ? silent : voiced) & (~0ull << p);
                if (!m) break;
                const int bit = __builtin_ctzll(m);
                p = bit + 1;
                if (start < 0) {     // a silent run opens
                    start = base + bit;
                    continue;
                }
                const int i = base + bit;   // the voiced frame that ends the run [start, i)
                const bool leading = start == 0 && i > M;
                const bool middle = i - start >= MI && i - clip >= ML;
                if (leading || middle) {
                    if (i - start <= M) {
                        const int pos = wave_argmin(r, start, i + 1, lane);
                        w.tag(start == 0 ? 0 : pos, pos);
                        clip = pos;
                    } else if (i - start <= 2 * M) {
                        const int pos = wave_argmin(r, i - M, min(start + M + 1, F), lane);
                        const int pos_l = wave_argmin(r, start, min(start + M + 1, F), lane);
                        const int pos_r = wave_argmin(r, i - M, i + 1, lane);
                        if (start == 0) {
                            w.tag(0, pos_r);
                            clip = pos_r;
                        } else {
                            w.tag(min(pos_l, pos), max(pos_r, pos));
                            clip = max(pos_r, pos);
                        }
                    } else {
                        const int pos_l = wave_argmin(r, start, min(start + M + 1, F), lane);
                        const int pos_r = wave_argmin(r, i - M, i + 1, lane);
                        w.tag(start == 0 ? 0 : pos_l, pos_r);
                        clip = pos_r;
                    }
                }
                start = -1;
            }
            cur = nxt;
        }
        if (start >= 0 && F - start >= MI) {   // trailing silence
            const int end = min(F, start + M);
            w.tag(wave_argmin(r, start, min(end + 1, F), lane), F + 1);
        }
    }
    w.close();
    for (int k = 3 * w.count + lane; k < 3 * a.capacity; k += 64) w.table[k] = 0;
    if (lane == 0) {
        a.count[b] = w.count;
        if (w.overflow) __hip_atomic_store(a.err, DDSP_DEV_ERR_SLICER, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

extern "C" int64_t ddsp_slicer_frames(int64_t n, int64_t win, int64_t hop) {
    if (n < 0 || win < 1 || hop < 1 || n + 2 * (win / 2) < win) return -1;
    return 1 + (n + 2 * (win / 2) - win) / hop;
}

// n_samples == nullptr: every row holds T samples
extern "C" int ddsp_slicer(ddsp_ctx* ctx, void* stream, const float* audio, int64_t B, int64_t T, const int32_t* n_samples,
                           int64_t win, int64_t hop, double threshold, int64_t min_length, int64_t min_interval,
                           int64_t max_sil_kept, int pad_mode, float* rms, int32_t* table, int32_t* count, int64_t capacity) {
    DDSP_REQUIRE(ctx, ctx && audio && rms && table && count, "ddsp_slicer: null argument");
    DDSP_REQUIRE(ctx, B >= 0 && B <= 65535 && T >= 1 && win >= 1 && hop >= 1 && T + 4 * hop + win < (1ll << 31),
                 "ddsp_slicer: bad shape");
    DDSP_REQUIRE(ctx, min_length >= 0 && min_interval >= 1 && max_sil_kept >= 0 && min_length < (1ll << 30) &&
                          min_interval < (1ll << 30) && max_sil_kept < (1ll << 30) && threshold == threshold,
                 "ddsp_slicer: bad min_length, min_interval, max_sil_kept (frames) or threshold");
    DDSP_REQUIRE(ctx, pad_mode == DDSP_SLICER_PAD_CONSTANT || pad_mode == DDSP_SLICER_PAD_REFLECT, "ddsp_slicer: bad pad_mode");
    const int64_t F_max = ddsp_slicer_frames(T, win, hop);
    DDSP_REQUIRE(ctx, F_max >= 1 && F_max < (1ll << 30), "ddsp_slicer: bad frame count");
    DDSP_REQUIRE(ctx, capacity >= 1 && capacity * 3 < (1ll << 31), "ddsp_slicer: bad capacity");
    int rc;
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    if (B == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;
    hipStream_t st = (hipStream_t)stream;

    RmsArgs ra;
    ra.x = audio;
    ra.n_samples = n_samples;
    ra.T = T;
    ra.win = (int)win;
    ra.hop = (int)hop;
    ra.pad_mode = pad_mode;
    ra.F_max = (int)F_max;
    ra.rms = rms;
    // the staging area holds up to 3 samples of alignment, the span and the rest of its last group of four
    const bool staged = win + 8 <= RMS_LDS_FLOATS;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    if (staged) {
        int64_t tile = (RMS_LDS_FLOATS - 8 - win) / hop + 1;
        if (tile > RMS_MAX_TILE) tile = RMS_MAX_TILE;
        ra.tile = (int)tile;
        const size_t lds = (size_t)((3 + (tile - 1) * hop + win + 3) / 4 * 4) * sizeof(float);
        hipLaunchKernelGGL(slicer_rms_kernel<true>, dim3((unsigned)ceil_div64(F_max, tile), (unsigned)B), dim3(RMS_THREADS),
                           lds, st, ra);
    } else {
        ra.tile = RMS_THREADS / 64;
        hipLaunchKernelGGL(slicer_rms_kernel<false>, dim3((unsigned)ceil_div64(F_max, ra.tile), (unsigned)B),
                           dim3(RMS_THREADS), 0, st, ra);
    }
    ddsp_prof_end(ctx, st, 0.0, (double)B * ((double)T + (double)F_max) * 4.0);
    DDSP_LAUNCH_CHECK(ctx);

    TagArgs ta;
    ta.rms = rms;
    ta.n_samples = n_samples;
    ta.T = T;
    ta.win = (int)win;
    ta.hop = (int)hop;
    ta.F_max = (int)F_max;
    ta.threshold = threshold;
    ta.min_length = (int)min_length;
    ta.min_interval = (int)min_interval;
    // (a max_sil_kept beyond the frame count decides as the frame count does: every comparison is against a frame distance)
    ta.max_sil_kept = (int)(max_sil_kept < F_max ? max_sil_kept : F_max);
    ta.table = table;
    ta.count = count;
    ta.capacity = (int)capacity;
    ta.err = dev_err;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(slicer_tag_kernel, dim3((unsigned)B), dim3(64), 0, st, ta);
    ddsp_prof_end(ctx, st, 0.0, (double)B * ((double)F_max * 4.0 + (double)capacity * 12.0));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
