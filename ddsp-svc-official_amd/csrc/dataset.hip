// Device-resident training dataset: one launch assembles a training batch from packed arenas (reference: B calls of
// AudioDataset.__getitem__ / get_data, `data_loaders.py:88-146`, plus the DataLoader's five torch.stack collations).
//
// Row b of the batch is the triple (file, start_frame, unit_idx): injected by the caller, or drawn here from a device
// permutation, a cursor and a seed - every workgroup recomputes its own row's draw (a few hashes and one fp64 division), so
// there is no second launch and nothing is read back.  The row copies len_b frames of the file from start_frame on and
// writes exact zeros behind them.  Everything is a SELECT: padding is written once, a cell outside the file's range is never
// read, and a triple that points outside its file sets the context's device error word and leaves a row of zeros.
#include "common.h"

namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct GatherArgs {
    ddsp_dataset_view ds;
    const int32_t* triples;   // (B, 3) or null: drawn
    const int32_t* perm;
    int64_t cursor;
    uint64_t seed;
    const int32_t* len_rows;  // (B,) or null: crop_frames for every row
    int crop_frames;
    double waveform_sec, frame_sec;
    int Fr_out;
    int va, vu;               // elements per item of the audio / units copy: 1 (scalar), 4 or 8
    float* audio;
    float* units;
    float* f0;
    float* volume;
    int64_t* spk_id;
    int32_t* draws;
    int* err;
};

// dst[e] = e < n_copy ? (float)src[e] : 0 for the items i of this thread; V elements per item.  n_copy and n_out are
// multiples of V and src + e, dst + e are V-element aligned (the launcher chose V so)
template <typename T, int V>
__device__ __forceinline__ void copy_item(const T* __restrict__ src, float* __restrict__ dst, int64_t e, int64_t n_copy) {
    if constexpr (V == 1) {
        dst[e] = e < n_copy ? (float)src[e] : 0.f;
    } else if constexpr (V == 4) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (e < n_copy) {
            if constexpr (sizeof(T) == 4) v = *(const f32x4*)(src + e);
            else v = __builtin_convertvector(*(const f16x4*)(src + e), f32x4);
        }
        *(f32x4*)(dst + e) = v;
    } else {
        static_assert(sizeof(T) == 2, "8 elements per item: the fp16 arenas' 16-byte load");
        typedef float f32x8 __attribute__((ext_vector_type(8)));
        f32x8 v = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (e < n_copy) v = __builtin_convertvector(*(const f16x8*)(src + e), f32x8);
        *(f32x4*)(dst + e) = f32x4{v[0], v[1], v[2], v[3]};
        *(f32x4*)(dst + e + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
}

template <typename T>
__device__ __forceinline__ void copy_any(int V, const T* __restrict__ src, float* __restrict__ dst, int64_t e, int64_t n_copy) {
    if (V == 4) copy_item<T, 4>(src, dst, e, n_copy);
    else if (V == 1) copy_item<T, 1>(src, dst, e, n_copy);
    else if constexpr (sizeof(T) == 2) copy_item<T, 8>(src, dst, e, n_copy);
}

// grid (gx, B): the gx workgroups of a row share its items - audio, units, f0, volume laid end to end - grid-strided
template <typename T>
__global__ void __launch_bounds__(256) dataset_gather_kernel(GatherArgs a) {
    const int64_t b = blockIdx.y;
    const ddsp_dataset_view& ds = a.ds;
    const int hop = ds.hop, C = ds.n_unit, Fr = a.Fr_out;

    // ---- the row's triple (uniform over the workgroup) ----
    int file, start, uidx;
    if (a.triples) {
        file = a.triples[3 * b];
        start = a.triples[3 * b + 1];
        uidx = a.triples[3 * b + 2];
    } else {
        const uint64_t k = (uint64_t)(a.cursor + b);
        const int p = a.perm[a.cursor + b];
        file = (p >= 0 && p < ds.n_files) ? ds.next_valid[p] : -1;
        uidx = (int)(((uint64_t)ddsp_hash32(a.seed, 2 * k + 1) * (uint64_t)(ds.n_aunit + 1)) >> 32);
        start = 0;
        if (file >= 0 && file < ds.n_files) {
            // random.uniform(0, duration - waveform_sec - 0.1) / frame_resolution, `data_loaders.py:128-129`, in fp64
            const double u = (double)ddsp_hash32(a.seed, 2 * k) * (1.0 / 4294967296.0);
            const double span = ds.duration[file] - a.waveform_sec - 0.1;
            start = (int)((u * span) / a.frame_sec);
        }
    }
    const bool file_ok = file >= 0 && file < ds.n_files;
    int len = a.len_rows ? a.len_rows[b] : a.crop_frames;
    bool ok = file_ok && uidx >= 0 && uidx <= ds.n_aunit && start >= 0 && len >= 0 && len <= Fr;
    if (ok)
        ok = (int64_t)start + len <= (int64_t)ds.frames[file] && ((int64_t)start + len) * hop <= ds.audio_len[file] &&
             ds.audio_off[file] % a.va == 0;   // (the packing's alignment, which the vector path relies on)
    if (!ok) len = 0;

    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (!ok) __hip_atomic_store(a.err, DDSP_DEV_ERR_DATASET, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        a.draws[3 * b] = file;
        a.draws[3 * b + 1] = start;
        a.draws[3 * b + 2] = uidx;
        a.spk_id[b] = ok ? ds.spk_id[file] : 0;
    }

    // sources: formed only for a checked triple (len == 0 otherwise: nothing is read through them)
    const int64_t a_src = ok ? ds.audio_off[file] + (int64_t)start * hop : 0;
    const int64_t f_src = ok ? ds.frame_off[file] + start : 0;
    const T* audio_src = (const T*)ds.audio + a_src;
    const T* units_src = (const T*)ds.units + ((int64_t)(ok ? uidx : 0) * ds.total_frames + f_src) * C;
    const float* f0_src = ds.f0 + f_src;
    const float* vol_src = ds.volume + f_src;

    float* audio_dst = a.audio + b * (int64_t)Fr * hop;
    float* units_dst = a.units + b * (int64_t)Fr * C;
    float* f0_dst = a.f0 + b * (int64_t)Fr;
    float* vol_dst = a.volume + b * (int64_t)Fr;

    const int64_t nA = (int64_t)Fr * hop / a.va, nU = (int64_t)Fr * C / a.vu;
    const int64_t total = nA + nU + 2 * (int64_t)Fr;
    const int64_t copyA = (int64_t)len * hop, copyU = (int64_t)len * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        if (i < nA) {
            copy_any<T>(a.va, audio_src, audio_dst, i * a.va, copyA);
        } else if (i < nA + nU) {
            copy_any<T>(a.vu, units_src, units_dst, (i - nA) * a.vu, copyU);
        } else if (i < nA + nU + Fr) {
            copy_item<float, 1>(f0_src, f0_dst, i - nA - nU, len);
        } else {
            copy_item<float, 1>(vol_src, vol_dst, i - nA - nU - Fr, len);
        }
    }
}

}  // namespace

extern "C" int ddsp_dataset_gather(ddsp_ctx* ctx, void* stream, const ddsp_dataset_view* ds, const int32_t* triples,
                                   const int32_t* perm, int64_t n_perm, int64_t cursor, uint64_t seed, const int32_t* len_rows,
                                   int64_t crop_frames, double waveform_sec, int64_t B, int64_t Fr_out, float* audio,
                                   float* units, float* f0, float* volume, int64_t* spk_id, int32_t* draws) {
    DDSP_REQUIRE(ctx, ctx && ds && audio && units && f0 && volume && spk_id && draws, "ddsp_dataset_gather: null argument");
    DDSP_REQUIRE(ctx, ds->audio && ds->units && ds->f0 && ds->volume && ds->audio_off && ds->audio_len && ds->frame_off &&
                          ds->frames && ds->spk_id && ds->duration && ds->next_valid,
                 "ddsp_dataset_gather: null pointer in the dataset view");
    DDSP_REQUIRE(ctx, ds->n_files >= 1 && ds->n_files < (1ll << 31) && ds->total_frames >= 1 && ds->n_aunit >= 0 &&
                          ds->n_unit >= 1 && ds->hop >= 1 && ds->sample_rate >= 1 && (ds->fp16 == 0 || ds->fp16 == 1),
                 "ddsp_dataset_gather: bad dataset view");
    DDSP_REQUIRE(ctx, B >= 0 && B <= 65535 && Fr_out >= 1 && Fr_out * (int64_t)ds->hop < (1ll << 31) &&
                          Fr_out * (int64_t)ds->n_unit < (1ll << 31),
                 "ddsp_dataset_gather: bad shape");
    DDSP_REQUIRE(ctx, (triples != nullptr) != (perm != nullptr), "ddsp_dataset_gather: pass injected triples or a permutation to draw from, not both");
    if (perm) {
        DDSP_REQUIRE(ctx, !len_rows, "ddsp_dataset_gather: a drawn batch is a cropped one (len_rows goes with injected triples)");
        DDSP_REQUIRE(ctx, cursor >= 0 && n_perm >= 0 && cursor + B <= n_perm, "ddsp_dataset_gather: cursor + B passes the permutation's end");
        DDSP_REQUIRE(ctx, waveform_sec >= 0.0, "ddsp_dataset_gather: bad waveform_sec");
    }
    if (!len_rows) DDSP_REQUIRE(ctx, crop_frames >= 0 && crop_frames <= Fr_out, "ddsp_dataset_gather: crop_frames outside [0, Fr_out]");
    int rc;
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    if (B == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;

    GatherArgs a;
    a.ds = *ds;
    a.triples = triples;
    a.perm = perm;
    a.cursor = cursor;
    a.seed = seed;
    a.len_rows = len_rows;
    a.crop_frames = (int)crop_frames;
    a.waveform_sec = waveform_sec;
    a.frame_sec = (double)ds->hop / (double)ds->sample_rate;
    a.Fr_out = (int)Fr_out;
    a.audio = audio;
    a.units = units;
    a.f0 = f0;
    a.volume = volume;
    a.spk_id = spk_id;
    a.draws = draws;
    a.err = dev_err;
    // 16-byte accesses where base, start and width allow: every file's audio offset is a multiple of 8 elements and every
    // units arena starts on 16 bytes (the packing pads them), so the widths decide - else the scalar path
    const bool aligned = (((uintptr_t)ds->audio | (uintptr_t)ds->units | (uintptr_t)audio | (uintptr_t)units) % 16) == 0;
    const int hop = ds->hop, C = ds->n_unit;
    const bool arena_rows_ok = ds->fp16 ? ((ds->total_frames * (int64_t)C) % 8 == 0) : ((ds->total_frames * (int64_t)C) % 4 == 0);
    a.va = a.vu = 1;
    if (aligned) {
        if (ds->fp16) {
            if (hop % 8 == 0) a.va = 8;
            if (arena_rows_ok) a.vu = C % 8 == 0 ? 8 : (C % 4 == 0 ? 4 : 1);
        } else {
            if (hop % 4 == 0) a.va = 4;
            if (arena_rows_ok && C % 4 == 0) a.vu = 4;
        }
    }
    // a bandwidth kernel: spread every row over enough workgroups to fill the CUs (about 2048 in all, 4 items a thread)
    const int64_t items = Fr_out * hop / a.va + Fr_out * C / a.vu + 2 * Fr_out;
    int64_t gx = ceil_div64(items, 256 * 4);
    const int64_t cap = ceil_div64(2048, B);
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    if (ds->fp16)
        hipLaunchKernelGGL(dataset_gather_kernel<_Float16>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(dataset_gather_kernel<float>, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, st, a);
    const double out_elems = (double)B * Fr_out * ((double)hop + C + 2);
    ddsp_prof_end(ctx, st, 0.0, out_elems * (4.0 + (ds->fp16 ? 2.0 : 4.0)));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
