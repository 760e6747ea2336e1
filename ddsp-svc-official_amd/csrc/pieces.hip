// The rows of one ragged group of an offline conversion of SEVERAL files, formed in one launch from the padded batch of the
// files (reference: per slice `audio[int(start_frame * hop_size):int(end_frame * hop_size)]`, `f0[:, start:start + n]` shifted
// by the file's key and `volume[:, start:start + n]`, `main.py:143-159`; one slice and one file at a time there).
//
// Row r of the piece table is (file, start_frame, n_frames, start_sample, n_samples); the host forms the sample range, because
// the hop may be fractional and `main.split` snaps with Python's int().  The row copies n_samples samples of its file's audio
// and n_frames frames of its f0 - times the file's key factor, one rounded fp32 product - and volume, and writes exact zeros
// behind them.  grid (gx, R): the gx workgroups of a row share its items - groups of four consecutive outputs of wav, f0_rows
// and vol_rows laid end to end - grid-strided.  An item is stored as 16 bytes where its four outputs lie inside the row at an
// aligned address, and loaded as 16 bytes where its four sources lie inside the piece at an aligned address; elsewhere every
// element goes through a bounds SELECT (as in stitch_kernel), so no address outside a file's own row is formed.  A row whose
// range leaves its file, or whose counts exceed the output widths, is written as zeros and sets the context's error word.
// HBM-bound: 4 B read and 4 B written per element.
//
// ddsp_pieces_gather_jobs is the same launch over rows of SIX columns: the sixth names the row's JOB - one conversion of the
// file to one voice and key.  The file still names the source of audio, f0 and volume, so J jobs over one file read that file's
// features in place; the job names the key factor, key_factor (J).  A job outside [0, J) is a bad row like a file outside [0, F):
// it is tested before key_factor is indexed.
//
// ddsp_pieces_gather_keys is the six-column launch with a KEY TIMELINE per job in place of the one factor: job j owns the
// breakpoints bp_off[j] .. bp_off[j + 1] - 1 of bp_frame (file frames), bp_semi and bp_fac, and frame t of a row is its file's
// f0 times the factor at file frame start_frame + t (key_timeline.h states the rule; one rounded product per element).  A
// breakpoint range that is empty or leaves [0, P) is a bad row like a job outside [0, J): tested before any address is formed.
#include "common.h"
#include "key_timeline.h"

namespace {

struct PiecesArgs {
    const float* audio;            // (F, T_max) or null: no wav rows
    const float* f0;               // (F, Fr_max) or null: no frame rows
    const float* volume;           // (F, Fr_max)
    const float* key_factor;       // (F)
    const int32_t* n_file_samples; // (F)
    const int32_t* n_file_frames;  // (F)
    const int32_t* table;          // (R, cols)
    int64_t F, T_max, Fr_max, S_max, N_max;
    int64_t cols, J;               // cols 5: key_factor (F) by file; cols 6: key_factor (J) by the row's sixth column
    const int32_t* bp_off;         // (J + 1) or null: no key timelines (key_factor holds the factors); with it key_factor is null
    const int32_t* bp_frame;       // (P) file frames
    const float* bp_semi;          // (P)
    const float* bp_fac;           // (P)
    int64_t P;
    float* wav;                    // (R, S_max)
    float* f0_rows;                // (R, N_max)
    float* vol_rows;               // (R, N_max)
    int* err;
};

// the key timeline of a row: n breakpoints (null and 0: the row takes one factor) and the file frame of the row's frame 0
struct KeyOfRow {
    const int32_t* bt;
    const float* semi;
    const float* fac;
    int n;
    int64_t first;
};

// dst[e .. e + 3] (as far as they lie before n_out) = scale * src[.] before n_copy, 0 from there on.  src is only indexed
// below n_copy.  SCALE: the product is one rounded multiplication; without it the value is copied untouched.  With a key
// timeline (key.n > 0) the scale is every element's own: the factor at file frame key.first + e + k.
template <bool SCALE>
__device__ __forceinline__ void copy4(const float* __restrict__ src, int64_t n_copy, float* __restrict__ dst, int64_t n_out,
                                      int64_t e, float scale, const KeyOfRow& key) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (e + 3 < n_copy && (((uintptr_t)(src + e)) & 15) == 0) {
        v = *(const f32x4*)(src + e);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < n_copy) v[k] = src[e + k];
    }
    if (SCALE) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < n_copy)
                v[k] = __fmul_rn(v[k], key.n > 0 ? keytl::factor_at(key.bt, key.semi, key.fac, key.n, (double)(key.first + e + k))
                                                 : scale);
    }
    if (e + 3 < n_out && (((uintptr_t)(dst + e)) & 15) == 0) {
        *(f32x4*)(dst + e) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (e + k < n_out) dst[e + k] = v[k];
    }
}

__global__ void __launch_bounds__(256) pieces_gather_kernel(PiecesArgs a) {
    const int64_t r = blockIdx.y;
    const int32_t* __restrict__ row = a.table + a.cols * r;
    const int64_t file = row[0], sf = row[1], ss = row[3];
    const int64_t key_of = a.cols == 6 ? row[5] : file;   // whose key factor the row takes: its job's, or its file's
    int64_t nf = row[2], ns = row[4];
    bool ok = file >= 0 && file < a.F && key_of >= 0 && key_of < (a.cols == 6 ? a.J : a.F);
    if (ok) {
        // every half is held to its own columns and widths: those of a half that was not asked for mean nothing
        const int64_t file_samples = a.n_file_samples[file], file_frames = a.n_file_frames[file];
        if (a.audio)
            ok = ss >= 0 && ns >= 0 && file_samples >= 0 && file_samples <= a.T_max && ss + ns <= file_samples && ns <= a.S_max;
        if (a.f0)
            ok = ok && sf >= 0 && nf >= 0 && file_frames >= 0 && file_frames <= a.Fr_max && sf + nf <= file_frames && nf <= a.N_max;
    }
    // a row of the keys launch: its job's breakpoint range, read only for a job inside [0, J) and held to [0, P)
    int64_t bp_lo = 0, bp_hi = 0;
    if (ok && a.bp_off) {
        bp_lo = a.bp_off[key_of];
        bp_hi = a.bp_off[key_of + 1];
        ok = bp_lo >= 0 && bp_hi > bp_lo && bp_hi <= a.P;
    }
    if (!ok) {
        nf = ns = 0;
        if (blockIdx.x == 0 && threadIdx.x == 0)
            __hip_atomic_store(a.err, DDSP_DEV_ERR_PIECES, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // sources: formed only for a checked row (counts of 0 otherwise: nothing is read through them)
    const int64_t a_off = ok ? file * a.T_max + ss : 0, f_off = ok ? file * a.Fr_max + sf : 0;
    const bool timed = ok && a.f0 && a.bp_off;
    const float scale = (ok && a.f0 && !a.bp_off) ? a.key_factor[key_of] : 1.0f;
    const KeyOfRow key = {timed ? a.bp_frame + bp_lo : nullptr, timed ? a.bp_semi + bp_lo : nullptr,
                          timed ? a.bp_fac + bp_lo : nullptr, timed ? (int)(bp_hi - bp_lo) : 0, sf};
    const KeyOfRow none = {nullptr, nullptr, nullptr, 0, 0};
    const int64_t nW = a.audio ? (a.S_max + 3) / 4 : 0, nN = a.f0 ? (a.N_max + 3) / 4 : 0;
    const int64_t total = nW + (a.volume ? 2 : 1) * nN;   // (no volume: the f0 rows alone, as the enhancer takes them)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        if (i < nW) copy4<false>(a.audio + a_off, ns, a.wav + r * a.S_max, a.S_max, 4 * i, 1.0f, none);
        else if (i < nW + nN) copy4<true>(a.f0 + f_off, nf, a.f0_rows + r * a.N_max, a.N_max, 4 * (i - nW), scale, key);
        else copy4<false>(a.volume + f_off, nf, a.vol_rows + r * a.N_max, a.N_max, 4 * (i - nW - nN), 1.0f, none);
    }
}

}  // namespace

// the one body of all entries: `cols` 5 (key_factor by file, J unused) or 6 (key_factor (J) by job, or - bp_off given, key_factor
// null - the key timelines of the jobs; the four bp pointers are null on the other entries' path)
static int pieces_gather(ddsp_ctx* ctx, void* stream, const float* audio, const float* f0, const float* volume,
                         const float* key_factor, const int32_t* n_file_samples, const int32_t* n_file_frames, int64_t F,
                         int64_t T_max, int64_t Fr_max, int64_t cols, int64_t J, const int32_t* table, int64_t R, int64_t S_max,
                         int64_t N_max, float* wav, float* f0_rows, float* vol_rows, const int32_t* bp_off = nullptr,
                         const int32_t* bp_frame = nullptr, const float* bp_semi = nullptr, const float* bp_fac = nullptr,
                         int64_t P = 0) {
    DDSP_REQUIRE(ctx, ctx && n_file_samples && n_file_frames && (R == 0 || table), "ddsp_pieces_gather: null argument");
    DDSP_REQUIRE(ctx, (audio != nullptr) == (wav != nullptr), "ddsp_pieces_gather: audio and wav come together or not at all");
    DDSP_REQUIRE(ctx, (bp_off ? !key_factor : (f0 != nullptr) == (key_factor != nullptr)) && (f0 != nullptr) == (f0_rows != nullptr),
                 "ddsp_pieces_gather: f0, key_factor and f0_rows come together or not at all");
    DDSP_REQUIRE(ctx, (volume != nullptr) == (vol_rows != nullptr) && (!volume || f0),
                 "ddsp_pieces_gather: volume and vol_rows come together, and only with f0");
    DDSP_REQUIRE(ctx, audio || f0, "ddsp_pieces_gather: nothing to gather");
    DDSP_REQUIRE(ctx, F >= 1 && F < (1ll << 31) && R >= 0 && R <= 65535 && T_max >= 1 && T_max < (1ll << 31) && Fr_max >= 1 &&
                          Fr_max < (1ll << 31) && (!audio || (S_max >= 1 && S_max < (1ll << 31))) &&
                          (!f0 || (N_max >= 1 && N_max < (1ll << 31))),
                 "ddsp_pieces_gather: bad shape");
    int rc;
    if ((rc = ddsp_take_dev_error(ctx))) return rc;
    if (R == 0) return DDSP_OK;
    DDSP_ENTER_DEVICE(ctx);
    int* dev_err = nullptr;
    if ((rc = ddsp_dev_error_ptr(ctx, &dev_err))) return rc;
    PiecesArgs a;
    a.audio = audio;
    a.f0 = f0;
    a.volume = volume;
    a.key_factor = key_factor;
    a.n_file_samples = n_file_samples;
    a.n_file_frames = n_file_frames;
    a.table = table;
    a.F = F;
    a.T_max = T_max;
    a.Fr_max = Fr_max;
    a.S_max = audio ? S_max : 0;
    a.N_max = f0 ? N_max : 0;
    a.cols = cols;
    a.J = J;
    a.bp_off = bp_off;
    a.bp_frame = bp_frame;
    a.bp_semi = bp_semi;
    a.bp_fac = bp_fac;
    a.P = P;
    a.wav = wav;
    a.f0_rows = f0_rows;
    a.vol_rows = vol_rows;
    a.err = dev_err;
    // a bandwidth kernel: spread every row over enough workgroups to fill the CUs (about 2048 in all, 4 items a thread)
    const int n_tracks = volume ? 2 : 1;
    const int64_t items = ceil_div64(a.S_max, 4) + n_tracks * ceil_div64(a.N_max, 4);
    int64_t gx = ceil_div64(items, 256 * 4);
    const int64_t cap = ceil_div64(2048, R);
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    hipStream_t st = (hipStream_t)stream;
    ddsp_prof_begin(ctx, st, PF_OTHER);
    hipLaunchKernelGGL(pieces_gather_kernel, dim3((unsigned)gx, (unsigned)R), dim3(256), 0, st, a);
    ddsp_prof_end(ctx, st, 0.0, 8.0 * (double)R * ((double)a.S_max + (double)n_tracks * (double)a.N_max));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_pieces_gather(ddsp_ctx* ctx, void* stream, const float* audio, const float* f0, const float* volume,
                                  const float* key_factor, const int32_t* n_file_samples, const int32_t* n_file_frames,
                                  int64_t F, int64_t T_max, int64_t Fr_max, const int32_t* table, int64_t R, int64_t S_max,
                                  int64_t N_max, float* wav, float* f0_rows, float* vol_rows) {
    return pieces_gather(ctx, stream, audio, f0, volume, key_factor, n_file_samples, n_file_frames, F, T_max, Fr_max, 5, 0, table,
                         R, S_max, N_max, wav, f0_rows, vol_rows);
}

extern "C" int ddsp_pieces_gather_jobs(ddsp_ctx* ctx, void* stream, const float* audio, const float* f0, const float* volume,
                                       const float* key_factor, const int32_t* n_file_samples, const int32_t* n_file_frames,
                                       int64_t F, int64_t T_max, int64_t Fr_max, int64_t J, const int32_t* table, int64_t R,
                                       int64_t S_max, int64_t N_max, float* wav, float* f0_rows, float* vol_rows) {
    DDSP_REQUIRE(ctx, ctx && J >= 1 && J < (1ll << 31), "ddsp_pieces_gather_jobs: J must be in [1, 2^31)");
    return pieces_gather(ctx, stream, audio, f0, volume, key_factor, n_file_samples, n_file_frames, F, T_max, Fr_max, 6, J, table,
                         R, S_max, N_max, wav, f0_rows, vol_rows);
}

extern "C" int ddsp_pieces_gather_keys(ddsp_ctx* ctx, void* stream, const float* audio, const float* f0, const float* volume,
                                       const int32_t* bp_off, const int32_t* bp_frame, const float* bp_semi, const float* bp_fac,
                                       int64_t P, const int32_t* n_file_samples, const int32_t* n_file_frames, int64_t F,
                                       int64_t T_max, int64_t Fr_max, int64_t J, const int32_t* table, int64_t R, int64_t S_max,
                                       int64_t N_max, float* wav, float* f0_rows, float* vol_rows) {
    DDSP_REQUIRE(ctx, ctx && J >= 1 && J < (1ll << 31) && P >= 1 && P < (1ll << 31),
                 "ddsp_pieces_gather_keys: J and P must be in [1, 2^31)");
    DDSP_REQUIRE(ctx, bp_off && bp_frame && bp_semi && bp_fac, "ddsp_pieces_gather_keys: null breakpoint table");
    return pieces_gather(ctx, stream, audio, f0, volume, nullptr, n_file_samples, n_file_frames, F, T_max, Fr_max, 6, J, table, R,
                         S_max, N_max, wav, f0_rows, vol_rows, bp_off, bp_frame, bp_semi, bp_fac, P);
}
