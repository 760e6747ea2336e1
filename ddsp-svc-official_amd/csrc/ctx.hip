// Handle, scratch arena and error text for libddsp_amd.
#include "common.h"

#include <stdlib.h>

#define DDSP_ABI_VERSION 8   // (new entry points beside unchanged ones do not bump it: tests pin it - ddsp_bank_gather / ddsp_bank_scatter were added at 8); 2: ddsp_rss_loss takes the hops; 3: ddsp_conv1d / ddsp_nsf_mean emit activated (split) copies, kept-activation entry points; 4: ddsp_retime_f0; 5: ddsp_u2c_weights::version (prepared-weight cache); 6: ddsp_hubert_weights; 7: ddsp_crepe_weights; 8: one symbol per operation - the _ragged / _batch / _scaled / _dseed / _share twins are folded into the un-suffixed names, whose optional parts are NULL / 1 (INTEGRATION.md has the old-name table)

extern "C" int ddsp_abi_version(void) { return DDSP_ABI_VERSION; }

extern "C" int ddsp_ctx_create(ddsp_ctx** out, int device) {
    if (!out) return DDSP_ERR_ARG;
    ddsp_ctx* c = (ddsp_ctx*)calloc(1, sizeof(ddsp_ctx));
    if (!c) return DDSP_ERR_OOM;
    c->device = device;
    c->math = DDSP_MATH_SPLIT_BF16;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        free(c);
        return DDSP_ERR_HIP;  // no silent CPU fallback: the library is unusable without a GPU
    }
    if (device < 0 || device >= ndev) {
        free(c);
        return DDSP_ERR_ARG;
    }
    *out = c;
    return DDSP_OK;
}

extern "C" int ddsp_ctx_destroy(ddsp_ctx* ctx) {
    if (!ctx) return DDSP_OK;
    ddsp_device_guard guard;
    (void)guard.enter(ctx->device);
    (void)hipDeviceSynchronize();
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->zero_page) (void)hipFree(ctx->zero_page);
    if (ctx->u2c_slot.dev) (void)hipFree(ctx->u2c_slot.dev);
    if (ctx->hubert_slot.dev) (void)hipFree(ctx->hubert_slot.dev);
    if (ctx->crepe_slot.dev) (void)hipFree(ctx->crepe_slot.dev);
    if (ctx->dev_error_host) (void)hipHostFree(ctx->dev_error_host);
    if (ctx->prof) {
        for (int i = 0; i < ctx->prof_events_made; ++i) {
            (void)hipEventDestroy(ctx->prof[i].start);
            (void)hipEventDestroy(ctx->prof[i].stop);
        }
        free(ctx->prof);
    }
    for (int i = 0; i < ctx->n_tables; ++i)
        if (ctx->tables[i].dev) (void)hipFree(ctx->tables[i].dev);
    free(ctx);
    return DDSP_OK;
}

extern "C" int ddsp_ctx_set_math(ddsp_ctx* ctx, int math) {
    if (!ctx) return DDSP_ERR_ARG;
    // (4: split-bf16 with every operand split inside the GEMM loops, test_presplit_operands_give_the_same_bits)
    DDSP_REQUIRE(ctx, math == DDSP_MATH_FP32 || math == DDSP_MATH_SPLIT_BF16 || math == 4, "ddsp_ctx_set_math: unknown mode");
    ctx->math = math;
    return DDSP_OK;
}

extern "C" int ddsp_ctx_get_math(const ddsp_ctx* ctx) { return ctx ? ctx->math : DDSP_ERR_ARG; }

extern "C" const char* ddsp_last_error(const ddsp_ctx* ctx) { return ctx ? ctx->err : "null ctx"; }

int ddsp_scratch_reserve_bytes(ddsp_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->scratch_bytes) return DDSP_OK;
    // Growing: earlier kernels may still read the old arena, so drain the device first.
    DDSP_ENTER_DEVICE(ctx);
    DDSP_HIP(ctx, hipDeviceSynchronize());
    if (ctx->scratch) DDSP_HIP(ctx, hipFree(ctx->scratch));
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    size_t want = bytes + (bytes >> 3) + (1u << 20);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) return ddsp_fail(ctx, DDSP_ERR_OOM, "scratch hipMalloc", hipGetErrorString(e));
    ctx->scratch = (char*)p;
    ctx->scratch_bytes = want;
    return DDSP_OK;
}

int ddsp_weight_slot_take(ddsp_ctx* ctx, hipStream_t st, ddsp_weight_slot& slot, const void* w, size_t key_bytes,
                          uint64_t version, size_t bytes, ddsp_weight_slot** out, bool keep_in_capture) {
    *out = nullptr;
    if (version == 0) return DDSP_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    if (capturing && !keep_in_capture) return DDSP_OK;
    uint64_t key = 1469598103934665603ull;   // FNV-1a
    const unsigned char* p = (const unsigned char*)w;
    for (size_t i = 0; i < key_bytes; ++i) key = (key ^ p[i]) * 1099511628211ull;
    if (key == 0) key = 1;
    if (capturing) {
        // nothing is allocated, synchronised or prepared while a stream is captured: the slot is handed out only as the
        // warm-up calls left it, for exactly these weights
        if (slot.dev && slot.bytes >= bytes && slot.key == key && slot.version == version && slot.state) *out = &slot;
        return DDSP_OK;
    }
    if (slot.bytes < bytes) {
        if (slot.dev) {
            // (the stream may still read the old buffer: wait for it before it goes)
            DDSP_HIP(ctx, hipStreamSynchronize(st));
            (void)hipFree(slot.dev);
        }
        slot = ddsp_weight_slot{};
        DDSP_HIP(ctx, hipMalloc((void**)&slot.dev, bytes));
        slot.bytes = bytes;
    }
    if (slot.key != key || slot.version != version) {
        slot.key = key;
        slot.version = version;
        slot.state = 0;
    }
    *out = &slot;
    return DDSP_OK;
}

extern "C" int ddsp_ctx_reserve(ddsp_ctx* ctx, uint64_t bytes) {
    if (!ctx) return DDSP_ERR_ARG;
    return ddsp_scratch_reserve_bytes(ctx, (size_t)bytes);
}

int ddsp_scratch_reset(ddsp_ctx* ctx) {
    ctx->scratch_used = 0;
    return DDSP_OK;
}

int ddsp_scratch_get(ddsp_ctx* ctx, size_t bytes, void** out) {
    size_t off = (ctx->scratch_used + 255) & ~(size_t)255;
    if (off + bytes > ctx->scratch_bytes)
        return ddsp_fail(ctx, DDSP_ERR_OOM, "scratch arena too small", "internal sizing error");
    *out = ctx->scratch + off;
    ctx->scratch_used = off + bytes;
    return DDSP_OK;
}

// ---- HIP-event profiler ------------------------------------------------------------------------------
static const char* kFamilyName[PF_COUNT] = {
    "phase_scan", "fir_act", "fir_dft_gemm", "ltv_fir", "u2c_prep", "u2c_gemm_conv3", "u2c_gemm_linear",
    "u2c_gemm_feat", "u2c_gemm_ctx", "u2c_gemm_attnout", "u2c_rowwise", "sins_bank", "spectral_ola", "rss_loss",
    "sola", "upsample", "other", "ltv_fir_bwd", "fir_synth_bwd", "u2c_bwd", "optim"};

void ddsp_prof_begin(ddsp_ctx* ctx, hipStream_t st, int id) {
    ctx->prof_open = 0;
    if (!ctx->prof_mask || !((ctx->prof_mask >> id) & 1ull) || ctx->prof_n >= DDSP_PROF_CAP) return;
    if (!ctx->prof) ctx->prof = (ddsp_prof_rec*)calloc(DDSP_PROF_CAP, sizeof(ddsp_prof_rec));
    if (!ctx->prof) return;
    ddsp_prof_rec& r = ctx->prof[ctx->prof_n];
    if (ctx->prof_n >= ctx->prof_events_made) {
        // timing events without the system-scope fence (and its L2 write-back) a default event performs when it completes:
        // the brackets sit inside bench.py's timed region, 32 records per step
        if (hipEventCreateWithFlags(&r.start, hipEventDisableSystemFence) != hipSuccess ||
            hipEventCreateWithFlags(&r.stop, hipEventDisableSystemFence) != hipSuccess)
            return;
        ctx->prof_events_made = ctx->prof_n + 1;
    }
    r.id = id;
    if (hipEventRecord(r.start, st) != hipSuccess) return;
    ctx->prof_open = 1;
}

void ddsp_prof_end(ddsp_ctx* ctx, hipStream_t st, double flops, double bytes) {
    if (!ctx->prof_open) return;
    ddsp_prof_rec& r = ctx->prof[ctx->prof_n];
    r.flops = flops;
    r.bytes = bytes;
    if (hipEventRecord(r.stop, st) == hipSuccess) ctx->prof_n++;
    ctx->prof_open = 0;
}

extern "C" int ddsp_profile_begin(ddsp_ctx* ctx, uint64_t family_mask) {
    if (!ctx) return DDSP_ERR_ARG;
    ctx->prof_n = 0;
    ctx->prof_open = 0;
    ctx->prof_mask = family_mask;
    return DDSP_OK;
}

// change which families are bracketed WITHOUT dropping the records taken so far (0 pauses): lets a caller bracket a sample of
// its steps only - an event record costs ~2 us of stream time, 38 of them per bench step are 6 % of it
extern "C" int ddsp_profile_mask(ddsp_ctx* ctx, uint64_t family_mask) {
    if (!ctx) return DDSP_ERR_ARG;
    ctx->prof_open = 0;
    ctx->prof_mask = family_mask;
    return DDSP_OK;
}

extern "C" int ddsp_profile_end(ddsp_ctx* ctx, ddsp_prof_entry* out, int max_entries, int* n_entries) {
    if (!ctx || !out || !n_entries) return DDSP_ERR_ARG;
    ctx->prof_mask = 0;
    ddsp_prof_entry agg[PF_COUNT];
    memset(agg, 0, sizeof(agg));
    for (int i = 0; i < ctx->prof_n; ++i) {
        ddsp_prof_rec& r = ctx->prof[i];
        DDSP_HIP(ctx, hipEventSynchronize(r.stop));
        float ms = 0.f;
        DDSP_HIP(ctx, hipEventElapsedTime(&ms, r.start, r.stop));
        ddsp_prof_entry& a = agg[r.id];
        a.launches += 1;
        a.ms_total += ms;
        a.flops_total += r.flops;
        a.bytes_total += r.bytes;
    }
    int n = 0;
    for (int id = 0; id < PF_COUNT && n < max_entries; ++id) {
        if (!agg[id].launches) continue;
        agg[id].family = id;
        strncpy(agg[id].name, kFamilyName[id], sizeof(agg[id].name) - 1);
        out[n++] = agg[id];
    }
    *n_entries = n;
    ctx->prof_n = 0;
    return DDSP_OK;
}

int ddsp_dev_error_ptr(ddsp_ctx* ctx, int** out) {
    if (!ctx->dev_error_host) {
        DDSP_ENTER_DEVICE(ctx);
        int* h = nullptr;
        hipError_t e = hipHostMalloc((void**)&h, 64, hipHostMallocMapped);
        if (e != hipSuccess) return ddsp_fail(ctx, DDSP_ERR_OOM, "error flag hipHostMalloc", hipGetErrorString(e));
        *h = 0;
        int* d = nullptr;
        e = hipHostGetDevicePointer((void**)&d, h, 0);
        if (e != hipSuccess) {
            (void)hipHostFree(h);
            return ddsp_fail(ctx, DDSP_ERR_HIP, "hipHostGetDevicePointer", hipGetErrorString(e));
        }
        ctx->dev_error_host = h;
        ctx->dev_error_dev = d;
    }
    *out = ctx->dev_error_dev;
    return DDSP_OK;
}

int ddsp_take_dev_error(ddsp_ctx* ctx) {
    if (!ctx->dev_error_host) return DDSP_OK;
    const int code = __atomic_exchange_n(ctx->dev_error_host, 0, __ATOMIC_ACQ_REL);
    if (code == DDSP_DEV_ERR_SPK_ID)
        return ddsp_fail(ctx, DDSP_ERR_ARG, "spk_id out of range [1, n_spk] in an earlier ddsp_unit2ctrl call",
                         "the speaker embedding of those rows was skipped (the reference's nn.Embedding raises)");
    if (code == DDSP_DEV_ERR_DATASET)
        return ddsp_fail(ctx, DDSP_ERR_ARG, "a (file, start_frame, unit_idx) triple outside its file in an earlier ddsp_dataset_gather call",
                         "those rows were written as zeros and nothing was read for them");
    if (code == DDSP_DEV_ERR_SLICER)
        return ddsp_fail(ctx, DDSP_ERR_ARG, "a row with more chunks than the table's capacity in an earlier ddsp_slicer call",
                         "the table holds the chunks that fit");
    if (code == DDSP_DEV_ERR_GATE_ROWS)
        return ddsp_fail(ctx, DDSP_ERR_ARG, "a row whose frames lie outside [0, Fr] or its own row in an earlier ddsp_volume_gate_rows "
                         "or ddsp_volume_gate_files call", "those rows were left as they were");
    if (code == DDSP_DEV_ERR_PIECES)
        return ddsp_fail(ctx, DDSP_ERR_ARG, "a piece whose range leaves its file or exceeds the output widths in an earlier "
                         "ddsp_pieces_gather call", "those rows were written as zeros and nothing was read for them");
    if (code == DDSP_DEV_ERR_FORMANT)
        return ddsp_fail(ctx, DDSP_ERR_ARG, "a formant factor that is not finite or not > 0 in an earlier ddsp_ctrl_warp call",
                         "the segments of those rows were left as they were");
    if (code == DDSP_DEV_ERR_TUNE)
        return ddsp_fail(ctx, DDSP_ERR_ARG, "a pitch-correction setting whose a4 is not finite or not > 0, whose strength is outside "
                         "[0, 1] or whose alpha is outside (0, 1] in an earlier ddsp_f0_tune call", "the rows of that owner were left as they were");
    if (code == DDSP_DEV_ERR_RETRIEVE)
        return ddsp_fail(ctx, DDSP_ERR_ARG, "a retrieval ratio that is not finite or outside [0, 1] on a row that names an index in an "
                         "earlier ddsp_units_retrieve call", "the units of those rows were left as they were");
    if (code == DDSP_DEV_ERR_ENVELOPE)
        return ddsp_fail(ctx, DDSP_ERR_ARG, "an envelope-mix rate that is not finite or outside [0, 1], an owner or source row outside "
                         "its table, a source count < 1 or a span that leaves the tensor in an earlier ddsp_envelope_rms or "
                         "ddsp_envelope_apply call", "those rows were left as they were (their envelope is 0)");
    if (code) return ddsp_fail(ctx, DDSP_ERR_ARG, "device-side contract violation in an earlier call", "");
    return DDSP_OK;
}

extern "C" int ddsp_ctx_poll_error(ddsp_ctx* ctx) {
    if (!ctx) return DDSP_ERR_ARG;
    return ddsp_take_dev_error(ctx);
}

int ddsp_zero_page(ddsp_ctx* ctx, const float** out) {
    if (!ctx->zero_page) {
        DDSP_ENTER_DEVICE(ctx);
        float* p = nullptr;
        hipError_t e = hipMalloc((void**)&p, DDSP_ZERO_FLOATS * sizeof(float));
        if (e != hipSuccess) return ddsp_fail(ctx, DDSP_ERR_OOM, "zero page hipMalloc", hipGetErrorString(e));
        e = hipMemset(p, 0, DDSP_ZERO_FLOATS * sizeof(float));
        if (e != hipSuccess) {
            (void)hipFree(p);
            return ddsp_fail(ctx, DDSP_ERR_HIP, "zero page hipMemset", hipGetErrorString(e));
        }
        ctx->zero_page = p;
    }
    *out = ctx->zero_page;
    return DDSP_OK;
}
