/*
 * libddsp_amd - C ABI of the MI355X (gfx950) DDSP harmonic-plus-noise synthesis path.
 *
 * The reference (tarepan/DDSP-SVC-official) has no FFI layer: its callers import Python names
 * (`ddsp.vocoder.{load_model,Sins,CombSub,CombSubFast}`, `ddsp.core.upsample`, `ddsp.loss.RSSLoss`).
 * This header is the boundary a binding for that path attaches to; each entry point names the
 * reference code it replaces (paths relative to the reference root).  The Python mirror under
 * `ddsp-svc-official_amd/ddsp/` binds it with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in `_host`;
 *   - tensors are dense, row-major, fp32 unless stated; sizes are element counts;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing synchronises
 *     except scratch growth inside ddsp_ctx_reserve / the first call at a larger size;
 *   - return value: DDSP_OK or a negative DDSP_ERR_*; ddsp_last_error() gives the text;
 *   - one ddsp_ctx per stream/thread; a ctx holds scratch + constant tables, no model state.
 */
#ifndef DDSP_AMD_H
#define DDSP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDSP_OK 0
#define DDSP_ERR_ARG (-1)   /* shape / mode / null-pointer contract violated (Python: ValueError)   */
#define DDSP_ERR_HIP (-2)   /* a HIP runtime call or launch failed            (Python: RuntimeError) */
#define DDSP_ERR_OOM (-3)   /* scratch allocation failed                      (Python: RuntimeError) */

typedef struct ddsp_ctx ddsp_ctx;

/* ---- handle ------------------------------------------------------------------------------- */
int ddsp_ctx_create(ddsp_ctx** out, int device);
int ddsp_ctx_destroy(ddsp_ctx* ctx);
const char* ddsp_last_error(const ddsp_ctx* ctx);
/* Pre-size the scratch arena (bytes).  Optional; calls grow it on demand (with a device sync). */
int ddsp_ctx_reserve(ddsp_ctx* ctx, uint64_t bytes);
int ddsp_abi_version(void);
/* Device-side contract violations cannot fail the call that launched them (nothing synchronises): a kernel that meets
 * one - a speaker id outside [1, n_spk], where the reference's nn.Embedding raises - skips the access and sets a flag in
 * host-mapped memory.  The next ddsp_unit2ctrl_* call on the context, or this function (call it after synchronising the
 * stream), returns DDSP_ERR_ARG once and clears the flag. */
int ddsp_ctx_poll_error(ddsp_ctx* ctx);
/* Product arithmetic of the INFERENCE contractions that have both forms (the Linear / conv GEMMs of ddsp_unit2ctrl_fwd,
 * the inverse-DFT GEMMs of ddsp_fir_from_ctrl; ddsp_ltv_fir takes its own `math` argument):
 *   DDSP_MATH_SPLIT_BF16 (default): every fp32 product from three bf16 matrix products (hi*hi + hi*lo + lo*hi), fp32
 *                         accumulation, ~4e-6 relative error per contraction - narrower than the reference's fp32;
 *   DDSP_MATH_FP32:       fp32 matrix products (v_mfma_f32_*_f32), ~3e-7 - the reference's precision class.
 * Training: the weight-gradient and input-gradient GEMMs of ddsp_unit2ctrl_bwd / ddsp_unit2ctrl_bwd_kept FOLLOW this mode
 * too (split-bf16 by default: transposed pre-split weight copies, wgrad_bf16.h); the attention / FIR / filter-synthesis
 * adjoints, the spectral loss and every activation a backward call rebuilds use fp32 products in either mode.  A caller that
 * needs reference-class fp32 gradients sets DDSP_MATH_FP32 around the backward call as well.  The Python mirror runs the
 * training FORWARD in fp32 products (dL/dsignal amplifies a 4e-6 disagreement between forward and backward) and leaves the
 * backward on the context's mode.  GEMMs whose shape keeps them off the LDS-DMA kernel (K not a multiple of 32, unaligned
 * rows) run fp32 products in either mode. */
#define DDSP_MATH_FP32 0
#define DDSP_MATH_SPLIT_BF16 3
int ddsp_ctx_set_math(ddsp_ctx* ctx, int math);
int ddsp_ctx_get_math(const ddsp_ctx* ctx);

/* ---- a1: frame -> sample linear upsampler ------------------------------------------------- */
/* replaces ddsp/core.py:7-21 `upsample(signal(B,Fr,C), factor)`; out (B, Fr*hop, C):
 * out[t] = fma(1-a, x[t/hop], a*x[min(t/hop+1, Fr-1)]), a = (t%hop)/hop. */
int ddsp_upsample(ddsp_ctx* ctx, void* stream, const float* x, int64_t B, int64_t Fr, int64_t C, int hop,
                  float* out);

/* ---- a1-a3: f0 frames -> wrapped rotation, frame phases, combtooth ------------------------- */
#define DDSP_COMB_NONE 0
#define DDSP_COMB_SINC 1        /* ddsp/vocoder.py:539  CombSub                                   */
#define DDSP_COMB_SINC_GATED 2  /* ddsp/vocoder.py:459-460 CombSubFast: comb = 0 where f0 <= 0     */
/* replaces upsample(f0) + fo_to_rot (ddsp/core.py:31-51) + `2*pi*rot[:, ::hop]` (ddsp/vocoder.py:515-517)
 * + torch.sinc(sr*rot/(f0+1e-3)).  `precise` != 0 is the reference's infer=True (fp64 increments);
 * 0 is infer=False (fp32 increments, fp64 running sum rounded to fp32 per sample).
 * f0_frames (B,Fr); initial_phase (B,) radians or NULL; outputs (any may be NULL except phase_frames):
 * rot (B,T) cycles in [-0.5,0.5]; phase (B,T) = 2*pi*rot (Sins, ddsp/vocoder.py:392); comb (B,T);
 * f0_up (B,T) upsampled f0; phase_frames (B,Fr) radians. T = Fr*hop. */
int ddsp_phase_scan(ddsp_ctx* ctx, void* stream, const float* f0_frames, const float* initial_phase, int64_t B,
                    int64_t Fr, int hop, int sr, int precise, int comb_mode, float* rot, float* phase, float* comb,
                    float* f0_up, float* phase_frames);

/* ---- a5-a6: control frames -> linear-phase FIR frames -------------------------------------- */
#define DDSP_FIR_ALLPASS 0  /* mags = exp(j*cumsum(pi*tanh(ctrl))), no window (ddsp/vocoder.py:521,540) */
#define DDSP_FIR_DYNAMIC 1  /* mags = exp(ctrl), raised-cosine of half width 1.5*sr/(f0+1e-3) (:522,541-542; ddsp/core.py:292-303) */
#define DDSP_FIR_STATIC 2   /* mags = exp(ctrl)/128, periodic Hann (:523,546; ddsp/core.py:242-289)  */
/* replaces the ctrl activation + ddsp/core.py:306-328 `_frequency_impulse_response`.
 * ctrl: (B*Fr) rows of `n_mag` values at row stride `ctrl_ld` (so a column block of the fused control
 * matrix can be passed in place); f0_frames (B*Fr) (DYNAMIC only); ir out (B*Fr, n = 2*(n_mag-1)).
 * ddsp_ctx_set_math: DDSP_MATH_FP32 forms fp32 products and the DYNAMIC window in IEEE form (two divisions and cosf per tap, the
 * reference's order of operations); DDSP_MATH_SPLIT_BF16 forms split-bf16 products where n_mag is a multiple of 32 (all-pass: of
 * 16) and there the fast DYNAMIC window (one reciprocal per row, v_cos_f32: ~1e-6 of the weight); every other n_mag keeps fp32
 * products and the IEEE window in either mode. */
int ddsp_fir_from_ctrl(ddsp_ctx* ctx, void* stream, int mode, const float* ctrl, int64_t ctrl_ld, int n_mag,
                       const float* f0_frames, int64_t rows, int sr, float* ir);

/* Up to three filters of ONE control matrix in one call (the filters of a synthesiser's render chain).  Each problem is a
 * ddsp_fir_from_ctrl call on the columns [col, col + n_mag) of ctrl and writes the same bits into its ir.  Inference at large
 * row counts (split-bf16 products, rows >= 8192, every n_mag a multiple of 32 - all-pass: of 16 with 2*pad32(n_mag) >= 256 - and
 * 16-byte aligned column blocks): two launches, one for all activations and one grouped inverse-DFT product.  Every other case
 * runs the single calls in order. */
typedef struct ddsp_fir_problem {
    int mode;               /* DDSP_FIR_* */
    int col;                /* first column of the filter's control values */
    int n_mag;
    const float* f0_frames; /* (rows), DYNAMIC only (else NULL) */
    float* ir;              /* out (rows, 2*(n_mag-1)) */
} ddsp_fir_problem;
int ddsp_fir_from_ctrl_group(ddsp_ctx* ctx, void* stream, const float* ctrl, int64_t ctrl_ld, int64_t rows, int sr,
                             const ddsp_fir_problem* problems, int n_problems);

/* ---- a7: frame-varying FIR (50%-overlap triangular cross-fade between frame filters) -------- */
/* replaces ddsp/core.py:185-239 `_fft_convolve` (+ :147-182 crop): out[u] = sum over taps of
 * x[t]*((1-j/hop)*ir[m] + (j/hop)*ir[min(m+1,Fr-1)])[u + n/2 - t], t = m*hop + j.
 * excitation: DDSP_EXC_AUDIO      audio (B,T) is the input signal;
 *             DDSP_EXC_UNIT_NOISE audio (B,T) holds U[0,1) draws and the input is 2*u-1 (the reference's
 *                                 `torch.rand_like(x)*2-1`, ddsp/vocoder.py:545, with the draw injected);
 *             DDSP_EXC_GENERATE   audio is NULL, the input is a counter-based U[-1,1) stream keyed by
 *                                 noise_seed (perf mode: the CPU mt19937 stream cannot be reproduced on a GPU).
 * out (B,T) or NULL receives the filtered signal; out_sum (B,T) or NULL receives filtered + add_in
 * (fuses `harmonic + noise`, ddsp/vocoder.py:548); add_in and out_sum are given together.
 * math: DDSP_FIR_FP32 = products on the fp32 matrix pipe (training forward, tight-tolerance checks);
 *       DDSP_FIR_SPLIT_BF16 = every fp32 product formed from three bf16 matrix products (hi*hi + lo*hi + hi*lo,
 *       fp32 accumulation, ~4e-6 relative error; the inference path).  Filters too long for that kernel's
 *       staging fall back to the fp32 kernel.  (Values 31..58 force one block shape of the split-bf16 kernels or
 *       switch their products off - measurement aids of tools/fir_bf16_check.py, not part of the interface.)
 * Requires hop in {128, 256, 512} and n even, 32 <= n <= 2046 (the same at every hop: up to 16 hops at 128).
 * hop 128 and 256 multiply on the fp32 matrix pipe whatever `math` (or ddsp_ctx_set_math) says: no split-bf16 form is
 * built for them.  The generated stream is one function of (noise_seed, row, sample index) at every hop.
 * ddsp_ltv_fir_bwd takes the same hops. */
#define DDSP_FIR_FP32 0
#define DDSP_FIR_SPLIT_BF16 3
#define DDSP_EXC_AUDIO 0
#define DDSP_EXC_UNIT_NOISE 1
#define DDSP_EXC_GENERATE 2
int ddsp_ltv_fir(ddsp_ctx* ctx, void* stream, const float* audio, int excitation, uint64_t noise_seed,
                 const float* ir, int64_t B, int64_t Fr, int hop, int n, const float* add_in, float* out,
                 float* out_sum, int math);


/* ---- a4: unit -> control network ---------------------------------------------------------- */
/* Device pointers into the model's state dict (reference key names), fp32, dense.
 * Shapes: conv weights (Cout, Cin, k) as torch stores them; Linear weights (out, in); d = 256.
 *   prenet_conv1_w (256, n_unit, 3)  prenet_gn_* (256)  prenet_conv2_w (256, 256, 3)
 *   f0_w/phase_w/volume_w (256, 1) + biases (256)        spk_table (n_spk, 256)
 *   per layer l0..l2: norm_* (256); q/k/v_w (512, 256) + b (512); proj (266, 64); out_w (256, 512) + b (256);
 *                     cm_ln_* (256); cm_pw1_w (1024, 256, 1); cm_dw_w (512, 1, 31); cm_pw2_w (256, 512, 1)
 *   final_ln_* (256); head_g (n_out, 1); head_v (n_out, 256); head_b (n_out)                               */
typedef struct ddsp_u2c_layer {
    const float *norm_w, *norm_b, *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *proj, *out_w, *out_b;
    const float *cm_ln_w, *cm_ln_b, *cm_pw1_w, *cm_pw1_b, *cm_dw_w, *cm_dw_b, *cm_pw2_w, *cm_pw2_b;
} ddsp_u2c_layer;

typedef struct ddsp_u2c_weights {
    const float *prenet_conv1_w, *prenet_conv1_b, *prenet_gn_w, *prenet_gn_b, *prenet_conv2_w, *prenet_conv2_b;
    const float *f0_w, *f0_b, *phase_w, *phase_b, *volume_w, *volume_b, *spk_table;
    int n_spk, n_unit, n_out;
    int causal;   /* 0 = the shipped configs (`c: false`); 1 = causal convolutions + causal linear attention */
    ddsp_u2c_layer layer[3];
    const float *final_ln_w, *final_ln_b, *head_g, *head_v, *head_b;
    /* The caller's change counter of the weight VALUES, or 0.  ddsp_unit2ctrl_fwd prepares the weights for its kernels on every
     * call (weight norm of the head, re-ordered pw1 rows, bf16 hi/lo copies: two launches, ~1.5 % of a 64-clip forward).  With
     * version != 0 it keeps the prepared copies in the context and reuses them while every pointer and integer of this struct
     * AND the version are what they were - so bump it whenever a tensor's contents change.  (torch: the sum of the parameters'
     * `_version` counters does that for every write torch counts; a write through the pointer - `.data`, a foreign kernel -
     * must advance the counter itself, `torch.autograd.graph.increment_version`, as ddsp_adamw_step's caller does.)  Ignored
     * while the stream is being captured into a HIP graph (a replay must see the weights of its own time) and by the training
     * entry points. */
    uint64_t version;
} ddsp_u2c_weights;

/* replaces ddsp/unit2control.py:68-101 `Unit2Control.forward` + ddsp/pcmer.py (non-causal, c=False only).
 * units (B,Fr,n_unit); f0_frames, phase_frames, volume (B,Fr); spk_id (n_spk_id) int64, 1-based, n_spk_id in
 * {1, B} (the reference broadcasts a (1,1) id); speaker mixing (`spk_mix_dict`): n_mix > 0 host arrays
 * mix_ids_host (1-based) / mix_w_host replace spk_id (n_mix <= 16).  ctrl out (B,Fr,n_out), the fused
 * control matrix that `split_to_dict` (ddsp/unit2control.py:10-20) views.  The `weights` struct itself is a
 * HOST pointer.  n_frames: NULL, or the counts of a ragged batch (next section). */
int ddsp_unit2ctrl_fwd(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* weights_host, const float* units,
                       const float* f0_frames, const float* phase_frames, const float* volume,
                       const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host,
                       const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, const int32_t* n_frames, float* ctrl);

/* ---- ragged batches: rows of different length in one padded (B, Fr, ...) call ------------------------------------------------
 * n_frames: DEVICE array of B int32, 1 <= n_frames[b] <= Fr (the caller checks it; the kernels hold a value outside the range
 * at its nearest bound), or NULL: every row has Fr frames.  Row b comes out as if it had been computed alone with
 * Fr = n_frames[b].
 *
 * With n_frames, ddsp_unit2ctrl_fwd runs the same launches, in which every place that looks across frames stops at the row's
 * own end: the GroupNorm statistics (count included), the zero padding of the second prenet convolution,
 * the key sums and the context of the linear attention, the input of the depthwise convolution.  Its first convolution
 * reads `units` as they are: frames >= n_frames[b] must hold 0 (ddsp_ragged_frames, hold = 0).  Rows of ctrl past a row's
 * count carry no meaning.
 *
 * The DSP entry points (ddsp_phase_scan, ddsp_fir_from_ctrl, ddsp_ltv_fir, ddsp_sins_bank, ddsp_spectral_ola) take a ragged
 * batch unchanged once it is in HELD form, which the three calls below produce by selection (never by a product with a
 * mask, so NaN or infinities in the padding are not read into arithmetic):
 *   ddsp_ragged_frames  dst[b][i][:] = i < n_b ? src[b][i][:] : (hold ? src[b][n_b - 1][:] : 0); src == dst is allowed.
 *                       hold = 1 for f0 and the control matrix (the kernels interpolate towards frame min(i + 1, Fr - 1) and
 *                       reuse the last filter for frame Fr: over held frames that IS min(i + 1, n_b - 1)); hold = 0 for
 *                       units, volume and the returned frame phases.
 *   ddsp_ragged_crop    x[b][t] = 0 for t >= n_b * hop in up to three (B, Fr*hop) signals (x1, x2 may be NULL): every
 *                       sample-rate signal before it enters a filter (a filter tail then reads the zeros a row rendered
 *                       alone is padded with) and every output.  hop % 4 == 0, 16-byte aligned buffers.
 *   ddsp_ragged_noise   out (B, Fr*hop) = the unit-noise draw U[0,1) for DDSP_EXC_UNIT_NOISE: inside a row noise[b][t], or
 *                       (noise == NULL) a counter hash of (noise_seed, b, t); 0.5 past the row's end (2u - 1 = 0 exactly). */
int ddsp_ragged_frames(ddsp_ctx* ctx, void* stream, const float* src, const int32_t* n_frames, int64_t B, int64_t Fr,
                       int64_t C, int hold, float* dst);

/* ---- a speaker mix per row, as device data (inference only) -----------------------------------------------------------------
 * ddsp_unit2ctrl_fwd_rowmix is ddsp_unit2ctrl_fwd whose speaker term comes from two DEVICE tables instead of spk_id or the
 * host mix: mix_ids_dev (B, K) int32, 1-based, and mix_w_dev (B, K) fp32, 1 <= K <= 16.  Row b of the batch adds
 *   sum_k mix_w_dev[b][k] * spk_table[mix_ids_dev[b][k] - 1]      (terms in slot order k = 0 .. K-1)
 * in the embedding epilogue of the second prenet convolution.  A slot {id 1, weight 0} is padding (a row with fewer than K
 * speakers); the row {id, 1.0} is a plain speaker id.  An id outside [1, n_spk] is not used as an index: the call's device
 * error word is set (DDSP_ERR_ARG from the next call or ddsp_ctx_poll_error) and the slot adds nothing.  The tables are read
 * when the kernels run, so a captured HIP graph follows later writes to them: nothing of the mix is a kernel argument.
 * n_frames (or NULL) as ddsp_unit2ctrl_fwd takes it.  The launches and tile choices are those of ddsp_unit2ctrl_fwd. */
int ddsp_unit2ctrl_fwd_rowmix(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* weights_host, const float* units,
                              const float* f0_frames, const float* phase_frames, const float* volume,
                              const int32_t* mix_ids_dev, const float* mix_w_dev, int K, int64_t B, int64_t Fr,
                              const int32_t* n_frames, float* ctrl);
/* The same call with the weights of every FRAME: mix_w_dev is (B, Fr, K), mix_ids_dev stays (B, K).  Frame i of row b adds
 *   sum_k mix_w_dev[b][i][k] * spk_table[mix_ids_dev[b][k] - 1]   (slot order, after the f0, phase and volume terms)
 * - the reference's `spk_mix_dict` with (B, Frame, 1) tensors as values, a voice that changes inside a call.  Ids, the error
 * word, n_frames and the launches as for ddsp_unit2ctrl_fwd_rowmix; weights constant over a row's frames give its bits. */
int ddsp_unit2ctrl_fwd_framemix(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* weights_host, const float* units,
                                const float* f0_frames, const float* phase_frames, const float* volume,
                                const int32_t* mix_ids_dev, const float* mix_w_dev, int K, int64_t B, int64_t Fr,
                                const int32_t* n_frames, float* ctrl);
int ddsp_ragged_crop(ddsp_ctx* ctx, void* stream, float* x0, float* x1, float* x2, const int32_t* n_frames, int64_t B,
                     int64_t Fr, int hop);
int ddsp_ragged_noise(ddsp_ctx* ctx, void* stream, const float* noise, uint64_t noise_seed, const int32_t* n_frames,
                      int64_t B, int64_t Fr, int hop, float* out);

/* Backward of ddsp_unit2ctrl_fwd for training (reference: autograd through Unit2Control, solver.py:113).  The call
 * re-runs the forward keeping its activations in the scratch arena, then back-propagates d_ctrl (B,Fr,n_out) to
 * every parameter.  `grads_host` has the layout of ddsp_u2c_weights; each pointer receives the gradient of the
 * like-named parameter (written, not accumulated; fast_attention.projection_matrix is a buffer: `proj` is ignored).
 * ctrl_out (B,Fr,n_out) or NULL additionally receives the forward result.  Inputs carry no gradient.
 * Ragged training (all three training calls; n_frames as for ddsp_unit2ctrl_fwd, or NULL): the forward keeps or re-runs the
 * ragged forward; units of frames >= n_frames[b] must hold 0 and f0, phase and volume finite values there (ddsp_ragged_frames),
 * and d_ctrl must be 0 on those frames (ddsp_ragged_frames with hold = 0, or ddsp_ragged_frames_adjoint).  Every gradient is
 * then the sum over rows of the gradient the row gives alone at its own length. */
int ddsp_unit2ctrl_bwd(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* weights_host, const float* units,
                       const float* f0_frames, const float* phase_frames, const float* volume,
                       const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host,
                       const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, const int32_t* n_frames, const float* d_ctrl,
                       const ddsp_u2c_weights* grads_host, float* ctrl_out);

/* A training step without the second forward: ddsp_unit2ctrl_fwd_keep is ddsp_unit2ctrl_fwd in fp32 products that leaves
 * its activations (~40 KB per frame and layer) in `keep`, a caller-owned device region of ddsp_unit2ctrl_keep_bytes(w, B, Fr)
 * bytes, 256-byte aligned (the autograd node owns it between the two calls: reference `solver.py:111-113`, where PyTorch
 * keeps the activations); ddsp_unit2ctrl_bwd_kept back-propagates from them exactly like ddsp_unit2ctrl_bwd, which re-runs
 * the forward instead.  The weights must not change between the two calls. */
int64_t ddsp_unit2ctrl_keep_bytes(const ddsp_u2c_weights* w, int64_t B, int64_t Fr);
int ddsp_unit2ctrl_fwd_keep(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* w, const float* units,
                            const float* f0_frames, const float* phase_frames, const float* volume,
                            const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host,
                            const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, const int32_t* n_frames, void* keep,
                            int64_t keep_bytes, float* ctrl);
int ddsp_unit2ctrl_bwd_kept(ddsp_ctx* ctx, void* stream, const ddsp_u2c_weights* w, const float* units,
                            const float* f0_frames, const float* phase_frames, const float* volume,
                            const int64_t* spk_id, int64_t n_spk_id, const int64_t* mix_ids_host,
                            const float* mix_w_host, int n_mix, int64_t B, int64_t Fr, const int32_t* n_frames, void* keep,
                            int64_t keep_bytes, const float* d_ctrl, const ddsp_u2c_weights* grads_host);
/* Adjoint of ddsp_ragged_frames with hold = 1, in place on a gradient d (B, Fr, C): d[b][n_b - 1][:] += sum_{i >= n_b} d[b][i][:]
 * (i ascending: a fixed order), then d[b][i >= n_b][:] = 0.  ddsp_ragged_crop is its own adjoint. */
int ddsp_ragged_frames_adjoint(ddsp_ctx* ctx, void* stream, float* d, const int32_t* n_frames, int64_t B, int64_t Fr, int64_t C);

/* ---- device-resident training dataset: a batch in one launch (reference: B calls of AudioDataset.__getitem__ / get_data,
 * data_loaders.py:88-146, and the DataLoader's torch.stack collations) -------------------------------------------------------
 * The dataset is packed once into arenas, all on the device: the files' audio back to back (fp32, or fp16 with fp16 = 1), each
 * file's first sample at an offset that is a multiple of 8 elements; (n_aunit + 1) units arenas of (total_frames, n_unit)
 * values of the same type, one behind the other (total_frames * n_unit is padded to a multiple of 8, so every arena starts on
 * 16 bytes); f0 and volume as (total_frames) fp32.  Per file i: audio_off[i] and audio_len[i] (samples), frame_off[i] (its
 * first row in the frame arenas) and frames[i], spk_id[i], duration[i] in seconds as the host computed it, and next_valid[i]:
 * the first file at or cyclically after i with duration >= waveform_sec + 0.1, the reference's skip (-1: there is none). */
typedef struct ddsp_dataset_view {
    const void* audio;
    const void* units;
    const float* f0;
    const float* volume;
    const int64_t* audio_off;
    const int64_t* audio_len;
    const int64_t* frame_off;
    const int32_t* frames;
    const int64_t* spk_id;
    const double* duration;
    const int32_t* next_valid;
    int64_t n_files, total_frames;
    int32_t n_aunit, n_unit, hop, sample_rate, fp16;
} ddsp_dataset_view;
/* One launch builds B rows.  Row b is the triple (file, start_frame, unit_idx):
 *   injected: triples (B, 3) int32 on the device (perm = NULL), used as they are;
 *   drawn:    triples = NULL and perm (n_perm) int32 on the device, cursor + B <= n_perm:
 *               file = next_valid[perm[cursor + b]], unit_idx uniform in 0..n_aunit,
 *               start_frame = (int)((u * (duration[file] - waveform_sec - 0.1)) / (hop / sample_rate)) in fp64, u in [0, 1);
 *             u and unit_idx are counter hashes of (seed, cursor + b), so a row's draw does not depend on the batch it is in.
 * The row copies len_b frames from start_frame on - len_b = crop_frames, or len_rows[b] (device, (B,) int32, injected triples
 * only: whole utterances of different length) - and writes exact zeros up to Fr_out: audio (B, Fr_out * hop), units
 * (B, Fr_out, n_unit), f0 (B, Fr_out[, 1]), volume (B, Fr_out) in fp32 whatever the arenas hold, spk_id (B[, 1]) int64, and
 * draws (B, 3) int32, the triples it used.  A triple that points outside its file (or a len_b outside [0, Fr_out]) is not
 * used as an index: the row comes out as zeros with spk_id 0 and the context's device error word is set (DDSP_ERR_ARG from
 * the next ddsp_dataset_gather / ddsp_unit2ctrl_* call or from ddsp_ctx_poll_error).  16-byte accesses where the widths allow
 * (fp32: hop % 4 == 0, n_unit % 4 == 0; fp16: hop % 8 == 0, n_unit % 8 == 0, 8-byte loads for n_unit % 4 == 0), scalar
 * otherwise; any hop >= 1 and n_unit >= 1 work.  Nothing synchronises and nothing is read back. */
int ddsp_dataset_gather(ddsp_ctx* ctx, void* stream, const ddsp_dataset_view* ds_host, const int32_t* triples,
                        const int32_t* perm, int64_t n_perm, int64_t cursor, uint64_t seed, const int32_t* len_rows,
                        int64_t crop_frames, double waveform_sec, int64_t B, int64_t Fr_out, float* audio, float* units,
                        float* f0, float* volume, int64_t* spk_id, int32_t* draws);

/* ---- backward of a5-a8 (training: reference autograd through frequency_filter, solver.py:113) ------------ */
/* Adjoints of ddsp_ltv_fir for an upstream gradient d_out (B,T): d_audio (B,T) or NULL = gradient w.r.t. the
 * input signal; d_ir (B,Fr,n) or NULL = gradient w.r.t. the filter frames (needs the forward input: audio with
 * its excitation mode, or DDSP_EXC_GENERATE + the same noise_seed). */
int ddsp_ltv_fir_bwd(ddsp_ctx* ctx, void* stream, const float* audio, int excitation, uint64_t noise_seed,
                     const float* ir, const float* d_out, int64_t B, int64_t Fr, int hop, int n, float* d_audio,
                     float* d_ir);
/* Adjoint of ddsp_fir_from_ctrl: d_ir (rows, n) [scaled in place by the dynamic window in DYNAMIC mode; the weight is formed
 * in fp64 and rounded once with the product: d_ir is within an fp32 ulp of d_ir x window, element by element] ->
 * d_ctrl, written to `n_mag` columns at row stride d_ctrl_ld (a column block of the control-gradient matrix). */
int ddsp_fir_from_ctrl_bwd(ddsp_ctx* ctx, void* stream, int mode, const float* ctrl, int64_t ctrl_ld, int n_mag,
                           const float* f0_frames, int64_t rows, int sr, float* d_ir, float* d_ctrl,
                           int64_t d_ctrl_ld);

/* ---- a10: additive sinusoid bank ----------------------------------------------------------- */
/* replaces ddsp/vocoder.py:397,402-412 + ddsp/core.py:24-28: amplitudes exp(ctrl)/128 masked by
 * ((k*f0 < sr/2) + 1e-7), upsampled per harmonic, times sin(k*phase), summed over k = 1..n_harmonics.
 * ctrl rows (B*Fr) at stride ctrl_ld; f0_frames (B*Fr); phase (B,T) radians as produced by
 * ddsp_phase_scan; out (B,T).  hop must be a power of two. */
int ddsp_sins_bank(ddsp_ctx* ctx, void* stream, const float* ctrl, int64_t ctrl_ld, int n_harmonics,
                   const float* f0_frames, const float* phase, int64_t B, int64_t Fr, int hop, int sr, float* out);

/* ---- a11: CombSubFast windowed spectral overlap-add ------------------------------------------ */
/* replaces ddsp/vocoder.py:462-490.  ctrl rows (B*Fr) at stride ctrl_ld hold
 * [harmonic_magnitude NB | harmonic_phase NB | noise_magnitude NB], NB = hop + 1; comb (B,T) from ddsp_phase_scan
 * (DDSP_COMB_SINC_GATED); noise (B,T) U[0,1) draws with excitation DDSP_EXC_UNIT_NOISE, or NULL with
 * DDSP_EXC_GENERATE + noise_seed; out (B,T).  hop in {128, 256, 512} (frames of 2*hop points); ddsp_spectral_ola_bwd
 * takes the same hops. */
int ddsp_spectral_ola(ddsp_ctx* ctx, void* stream, const float* ctrl, int64_t ctrl_ld, const float* comb,
                      const float* noise, int excitation, uint64_t noise_seed, int64_t B, int64_t Fr, int hop,
                      float* out);

/* Adjoints of a10 / a11 w.r.t. their control blocks (training of Sins / CombSubFast): d_out (B,T) -> d_ctrl written
 * to the same column block layout as the forward reads, at row stride d_ctrl_ld.
 * ddsp_sins_bank_bwd: hop a power of two <= 1024; n_harmonics <= 4096 when hop <= 512 and n_harmonics % 32 == 0,
 * else n_harmonics <= 2048 (DDSP_ERR_ARG above it). */
int ddsp_sins_bank_bwd(ddsp_ctx* ctx, void* stream, const float* ctrl, int64_t ctrl_ld, int n_harmonics,
                       const float* f0_frames, const float* phase, const float* d_out, int64_t B, int64_t Fr, int hop,
                       int sr, float* d_ctrl, int64_t d_ctrl_ld);
int ddsp_spectral_ola_bwd(ddsp_ctx* ctx, void* stream, const float* ctrl, int64_t ctrl_ld, const float* comb,
                          const float* noise, int excitation, uint64_t noise_seed, const float* d_out, int64_t B,
                          int64_t Fr, int hop, float* d_ctrl, int64_t d_ctrl_ld);

/* ---- a13: random-scale spectral loss ---------------------------------------------------------- */
/* replaces ddsp/loss.py:7-43 `RSSLoss.forward(x_pred, x_true)` for a given draw of scales: n_ffts_host holds the
 * n_scale values the reference draws with torch.randint(fft_min, fft_max) (ddsp/loss.py:39; the caller draws, so
 * data-parallel ranks can share one draw).  Per scale N: Hann(periodic) window, center=False, hop = hops_host[s] -
 * the caller evaluates the reference's `int(n_fft * (1 - overlap))` (ddsp/loss.py:13) in its own floating point - or
 * hop = N when hops_host is NULL (overlap = 0, what every reference caller uses); magnitude / sqrt(sum w^2) + eps;
 * L_N = mean_b ||S_t-S_p||_F/||S_t+S_p||_F + alpha*mean|ln S_t - ln S_p|; loss = mean_N.
 * x_pred, x_true (B,T) 16-byte aligned, T % 4 == 0; loss: device float[1]; grad_pred (B,T) or NULL receives
 * d loss / d x_pred (the caller's autograd scales it by the upstream gradient).
 * Rows of different length: n_samples_host (B ints, 1 <= n <= T) and the same counts on the device (n_samples_dev, int32), both
 * or neither (NULL: every row holds T samples).  Row b has F_b = (n_b - N) / hop + 1 frames at scale N (0 when n_b < N).  The
 * convergence term is the mean over the rows with F_b > 0, each norm over the row's own frames; the log term the mean over the
 * sum_b F_b * (N/2 + 1) cells that exist.  Samples from (F_b - 1) * hop + N on are not read into arithmetic (selection), and
 * grad_pred is 0 there.  With every count == T the result has the bits of the call without counts.  A scale at which no row has
 * a frame: DDSP_ERR_ARG before anything is launched.
 * The rows as ONE RANK'S SHARE of a global batch (data-parallel training on ragged shards): global_n_samples_host (with the
 * local counts only; NULL: the local rows are the whole batch, n_global is not read), the n_global >= B sample counts (each
 * >= 1; they may exceed T, another rank pads to its own longest row) of every rank's rows, the local rows among them.  Both
 * denominators - the rows with a frame and the cells that exist at scale N - are taken over the GLOBAL counts, the sums over the
 * local rows: loss is this rank's share of the loss of the global batch and grad_pred the gradient of that share.  Shares summed
 * over the ranks give the one-process loss; gradients summed over the ranks (no division by the number of ranks) its gradient.
 * A scale at which no GLOBAL row has a frame: DDSP_ERR_ARG before anything is launched.  A scale at which no LOCAL row has a
 * frame (n_fft > T included) contributes 0 and is not launched.  With global_n_samples_host equal to n_samples_host the result
 * has the bits of the call without it. */
int ddsp_rss_loss(ddsp_ctx* ctx, void* stream, const float* x_pred, const float* x_true, int64_t B, int64_t T,
                  const int* n_samples_host, const int32_t* n_samples_dev, const int* global_n_samples_host, int64_t n_global,
                  const int* n_ffts_host, const int* hops_host, int n_scale, float alpha, float eps, float* loss,
                  float* grad_pred);
/* One loss per row instead of the batch's scalar (validation: every utterance counts once; no gradient): the arguments of
 * ddsp_rss_loss with both counts, loss_rows a device float[B].  loss_rows[b] = mean_N (||S_t - S_p||_F / ||S_t + S_p||_F +
 * alpha * mean|ln S_t - ln S_p|), both terms over row b's own F_b * (N/2 + 1) cells - the loss of x[b][0..n_b) scored alone.
 * The framing, transform and statistics kernels are those of the calls above; only the last kernel differs.  A row without a
 * frame at one of the scales (n_b < N): DDSP_ERR_ARG before anything is launched. */
int ddsp_rss_loss_rows(ddsp_ctx* ctx, void* stream, const float* x_pred, const float* x_true, int64_t B, int64_t T,
                       const int* n_samples_host, const int32_t* n_samples_dev, const int* n_ffts_host, const int* hops_host,
                       int n_scale, float alpha, float eps, float* loss_rows);
/* The conversion leg of validation (reference solver.py:46-54) in one launch: f0 (B, Fr), src_spk (B) int64 1-based, lfo
 * (n_spk) the per-speaker log-f0 statistic (f0_stats.npy, entry id - 1), all on the device.  tgt_spk[b] = (src + 1) % n_spk,
 * and 0 becomes 1; f0_out[b][i] = exp(lfo[tgt] * ln(f0) / lfo[src]) in fp32, exactly 0 where f0 == 0, and 0 for
 * i >= n_frames[b] (device int32 (B), or NULL: every row has Fr frames; nothing is read there).  A source id outside
 * [1, n_spk] is not used as an index: the row is zeros, its target 0, and the context's device error word is set. */
int ddsp_vc_f0_map(ddsp_ctx* ctx, void* stream, const float* f0, const int64_t* src_spk, const float* lfo, int n_spk, int64_t B,
                   int64_t Fr, const int32_t* n_frames, float* f0_out, int64_t* tgt_spk);

/* ---- a14: SOLA splice of the real-time path -------------------------------------------------- */
/* S streams of one geometry in one call (realtime.StreamBank; S = 1: the reference's single stream): every tensor has a leading
 * dimension S (1 <= S <= DDSP_MAX_STREAMS), contiguous rows, with the stream as a grid dimension of the kernels.  Per row the
 * arithmetic and the order of every reduction do not depend on S, so row s of every output equals the S = 1 call on row s bit
 * for bit, and no row reads another row's audio, score or buffer. */
#define DDSP_MAX_STREAMS 4096
/* replaces gui.py:405-430: within audio[-block-xfade-search-delay : -delay] find the lag (0..search) that
 * maximises the energy-normalised correlation with sola_buffer (xfade,), cross-fade (sin^2 windows,
 * gui.py:349-351) the head with sola_buffer, emit `block` samples, and keep the next xfade samples in
 * sola_buffer (updated in place).  audio (S, n_audio), sola_buffer (S, xfade), emitted (S, block), shift (S): device int32 (no
 * host sync); each row splices at its own arg-max (first maximum) and hands over its own tail.  S > 1: search < 65535 and
 * n_audio < 2^31. */
int ddsp_sola(ddsp_ctx* ctx, void* stream, const float* audio, int S, int64_t n_audio, int block, int xfade, int search,
              int delay, float* sola_buffer, float* emitted, int* shift);

/* the sliding input window of the real-time callback (gui.py:373-374), in place on a buffer whose address never changes
 * (a captured graph reads it): window[s][:] = append(window[s][block:], block_in[s]); window (S, n_in), block_in (S, block)
 * outside the windows, 1 <= block < n_in (DDSP_ERR_ARG otherwise, nothing written).  The kept part is staged through the
 * context's scratch arena (two launches in stream order), so the overlapping shift is exact whatever order workgroups run in. */
int ddsp_stream_push(ddsp_ctx* ctx, void* stream, float* window, int S, int64_t n_in, const float* block_in, int64_t block);

/* The row movers of a bank's active set (realtime.StreamBank, `active=`): a call that advances A of the S slots runs them as a
 * compact batch of W rows, A <= W <= S.  rows (W) int32 DEVICE: entry r is the slot of compact row r, or -1 for a padding row;
 * it is read when the kernels run, so a captured graph follows a table that the host rewrites between replays.  An entry is
 * tested against [0, S) before it forms an address, and one outside is a padding row.  No slot may be named twice (the caller
 * checks it: two rows of one slot would race for its window).  A slot that `rows` does not name is neither read nor written.
 * ddsp_bank_gather, for every compact row r with slot s = rows[r]:
 *   window[s][:] = append(window[s][block:], block_in[r]) in place, as ddsp_stream_push does it and as exact: launch 1 writes
 *   the pushed window to cwindow[r] (W, n_in), outside the windows, launch 2 (stream order) copies it back to window[s], so no
 *   launch reads what it writes;  csola[r] = sola_buffer[s] (xfade);  cmix_ids[r] / cmix_w[r] = mix_ids[s] / mix_w[s] (K, the
 *   speaker mix of ddsp_unit2ctrl_fwd_rowmix, 1 <= K <= 16);  cpitch[r] = pitch[s];  crequest[r] = request[s] (the enhancer's
 *   key request; both NULL for a bank without one).
 * A padding row gets a zero window and buffer, speaker 1 with weight 1, pitch 1 and request 0.  block_in (W, block); window
 * (S, n_in), sola_buffer (S, xfade) and the tables have S rows, their compact forms W.  Rows move by 16-byte vector accesses when
 * n_in and block are multiples of 4 and the bases are 16-byte aligned, else by single words.  DDSP_ERR_ARG, and nothing written,
 * for W > S, S > DDSP_MAX_STREAMS, block >= n_in, a null pointer, or compact rows that overlap the bank's.
 * ddsp_bank_scatter, after the splice: sola_buffer[rows[r]] = csola[r] for every row that is no padding. */
int ddsp_bank_gather(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int S, float* window, int64_t n_in,
                     const float* block_in, int64_t block, float* cwindow, const float* sola_buffer, int xfade, float* csola,
                     const int32_t* mix_ids, const float* mix_w, int K, int32_t* cmix_ids, float* cmix_w, const float* pitch,
                     float* cpitch, const int32_t* request, int32_t* crequest);
int ddsp_bank_scatter(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int S, const float* csola, int xfade,
                      float* sola_buffer);

/* The speaker glide of a bank (realtime.StreamBank, `glide_breakpoints=`): the per-frame mix weights of one call's W rows
 * (ddsp_unit2ctrl_fwd_framemix's w) from per-SLOT state, and the advance of those slots' clocks, one launch per block.  Per slot
 * s < S, all DEVICE: clock[s] int64, the device samples pushed into the slot since its timeline started (read AND written);
 * bp_n[s] int32, its breakpoint count, clamped to [0, P_max], 0 = no timeline; bp_t[s] (P_max) int64, the breakpoint times in
 * device samples, strictly increasing; bp_w[s] (P_max, K) fp32, the weights there; spk_w[s] (K) fp32, the slot's row mix.
 * rows (W) int32 DEVICE as for ddsp_bank_gather, or NULL: row r is slot r.  Row r belongs to slot s = rows ? rows[r] : r, tested
 * against [0, S) before it forms an address.  An s outside is a padding row: every frame gets (1, 0, ..., 0), no clock is read
 * or written and no error word is set.  For a real row c = clock[s] + block is the stream position just behind the window's
 * newest sample, and frame t < Fr of the window (n_in samples, frames `hop` samples apart, hop possibly fractional) has time
 * tau = (double)(c - n_in) + t * hop.  With bp_n[s] == 0 every frame gets spk_w[s].  With a timeline the weights are its
 * breakpoints interpolated at tau as ddsp_mix_timeline interpolates: the first breakpoint's before it, the last one's after it,
 * between two w0 + (w1 - w0) * ((tau - t0) / (t1 - t0)) in fp64, rounded to fp32 (at a breakpoint exactly its fp32 value).
 * Then clock[s] = c: one workgroup per row reads the clock in every thread, meets behind its last frame and stores once.  No
 * slot may be named twice (the caller checks it: two rows would race for the clock).  PAUSED SLOTS: a slot that `rows` does not
 * name has no address of clock, bp_n, bp_t, bp_w or spk_w formed for it.  w_frames (W, Fr, K) fp32.  DDSP_ERR_ARG, and nothing
 * written, for a null pointer (rows excepted), W > 65535, K outside [1, 16], P_max outside [1, 64], Fr < 1 or block < 1.  Does not
 * synchronise, allocate or read back. */
int ddsp_bank_glide(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int S, int64_t* clock, const int32_t* bp_n,
                    const int64_t* bp_t, const float* bp_w, int P_max, const float* spk_w, int K, int64_t Fr, int64_t n_in,
                    int64_t block, double hop, float* w_frames);
/* The KEY glide of a bank (realtime.StreamBank, `pitch_breakpoints=`): the per-frame f0 factors of one call's W rows from
 * per-SLOT state, and the advance of those slots' key clocks, one launch per block: ddsp_bank_glide's launch with a key
 * timeline (the rule stated at ddsp_pieces_gather_keys) in place of the weights.  Per slot s < S, all DEVICE: key_clock[s] int64
 * (read AND written); key_n[s] int32, clamped to [0, P_max], 0 = no timeline; key_t[s] (P_max) int64, the breakpoint times in
 * device samples, strictly increasing; key_semi[s], key_fac[s] (P_max) fp32, their semitones and host-formed factors; pitch[s]
 * fp32, the slot's one factor.  rows, padding rows, c = key_clock[s] + block, tau = (double)(c - n_in) + t * hop, the clock's
 * store behind the barrier and the paused-slot rule are ddsp_bank_glide's.  pitch_frames (W, Fr) fp32: a padding row gets 1 in
 * every frame; a slot with key_n[s] == 0 gets pitch[s]; a slot with a timeline the rule's factor at tau.  DDSP_ERR_ARG, and
 * nothing written, for a null pointer (rows excepted), W > 65535, P_max outside [1, 64], Fr < 1 or block < 1.  Does not
 * synchronise, allocate or read back. */
int ddsp_bank_key_glide(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int S, int64_t* key_clock, const int32_t* key_n,
                        const int64_t* key_t, const float* key_semi, const float* key_fac, int P_max, const float* pitch,
                        int64_t Fr, int64_t n_in, int64_t block, double hop, float* pitch_frames);

/* The FORMANT SHIFT: a warp of spectral-envelope columns of the control matrix ctrl (rows, sum) fp32 along the frequency axis,
 * IN PLACE, between the control network and the filter synthesis; one launch, one pass over the warped columns.  A definition of
 * this project (the reference has no such control).
 * THE RULE.  A segment is n consecutive columns of a row with an origin o: 0 for magnitude bins (bin j lies at j * df), 1 for
 * harmonics (column j is harmonic j + 1).  For a factor a > 0 the warped segment is the envelope read at f / a, in fp32 with one
 * rounding per operation and nothing contracted:
 *     p  = fl(fl(float(j + o) / a) - float(o));   p = min(max(p, 0), float(n - 1))
 *     i0 = (int)floor(p);  i1 = min(i0 + 1, n - 1);  t = p - float(i0)                 (exact)
 *     out[j] = (t == 0) ? in[i0] : fl(in[i0] + fl(fl(in[i1] - in[i0]) * t))
 * t == 0 is a SELECTION: a == 1, every exact hit and every clamped end return the input's bits (-0.0, inf, NaN included); a
 * segment with n == 1 is copied.  The columns are the network's raw outputs, log-magnitudes, so the interpolation is geometric in
 * magnitude; a = 2 ** (s / 12) raises the formants by s semitones.
 * segments: HOST array of n_seg <= 3 triples (first column, n, origin), read during the call; 1 <= n <= 4096, inside the row,
 * origin 0 or 1.  rows = B * Fr.  The factor of a row, all DEVICE, read when the kernel runs: factor[row] (per_frame != 0,
 * factor (rows)), factor[row / Fr] (per_frame == 0, factor (B)), or - slot_of_row (B) int32 given, per_frame == 0 -
 * factor[slot_of_row[row / Fr]] with factor (S); the table's entry is tested against [0, S) before it forms an address and one
 * outside it is a padding row, factor 1.  n_frames (B) int32 DEVICE or NULL: a frame at or past its row's count (held in
 * [1, Fr]) has factor 1 whatever the array holds.  A factor that is not finite or not > 0 leaves the row as it was and raises
 * the device error word (DDSP_ERR_ARG from the next call that takes it, or ddsp_ctx_poll_error): no address depends on the
 * factor's value.  A row is staged per segment in the LDS before its first store and belongs to one workgroup.  Row strides are
 * arbitrary (16-byte vectors are used only where the row's own address allows).  DDSP_ERR_ARG, and nothing launched, for a null
 * pointer, rows not a multiple of Fr, a bad segment, or a row table beside a factor per frame.  Does not synchronise, allocate
 * or read back; graph-capturable. */
int ddsp_ctrl_warp(ddsp_ctx* ctx, void* stream, float* ctrl, int64_t rows, int64_t sum, const int32_t* segments, int n_seg,
                   const float* factor, int per_frame, int64_t Fr, const int32_t* slot_of_row, int64_t S, const int32_t* n_frames);

/* PITCH CORRECTION: the f0 of a row, f0 (B, Fr) fp32 IN PLACE, is pulled toward the notes of a scale, with a strength and a
 * retune speed; it runs between the analysis (after the key) and the synthesiser.  A definition of this project (the reference
 * has no such control).  One launch; every pointer is a DEVICE pointer, read when the kernel runs.
 * THE SETTING of an owner (a job offline, a slot live), J of them: mask (J) int32 - bit p in 0..11 allows pitch class p, C = 0,
 * MIDI note n has class n mod 12; only those twelve bits count and none of them set means OFF -; param (J, 3) fp64: a4 in Hz,
 * the strength s in [0, 1], alpha in (0, 1].  The host forms alpha = 1 - exp(-hop_seconds / retune_seconds), 1 for a retune of 0.
 * The owner of row b is owner[b] (int32), or b for owner == NULL; n_frames (B) int32 or NULL are the rows' counts n_b, held in
 * [1, Fr].
 * THE RULE.  A frame is VOICED when its f0 is finite and > 0.  For t = 0 .. n_b - 1, all in fp64 with one rounding per operation
 * and nothing contracted:
 *     m_t = 69 + 12 * log2(f_t / a4)
 *     n_t = the integer n with bit (n mod 12) of mask set that minimises |n - m_t|; a tie takes the smaller n
 *     d_t = n_t - m_t        (|d_t| <= 6; 0 where m_t is not finite, which takes an a4 beyond 1e+-260)
 *     c_t = d_t                                  if t is the row's first voiced frame, or frame t-1 is unvoiced   (a RESET)
 *     c_t = (1 - alpha) * c_(t-1) + alpha * d_t  otherwise
 *     out_t = (s * c_t == 0) ? f_t (its bits) : (float)((double)f_t * exp2(s * c_t / 12))
 * alpha == 1 with s == 1 is hard tuning; a small alpha low-passes the correction, so vibrato survives and note changes glide.
 * The recurrence restarts at every row start: the kernel carries no state from one call to the next.
 * UNTOUCHED, by selection and not by arithmetic, so their bits stay: unvoiced frames; frames at or past the row's count; rows
 * whose owner is off (no bit of the mask, or s == 0); rows whose owner index lies outside [0, J) - padding: the index is tested
 * before any address is formed and the error word is not set.
 * A BAD SETTING - a mask with a4 not finite or not > 0, s outside [0, 1] or alpha outside (0, 1] - leaves its rows untouched
 * and raises the device error word (DDSP_ERR_ARG from the next call that takes it, or ddsp_ctx_poll_error); a setting without a
 * mask is off and is not judged, nor is one that no row names.  No address depends on a setting's value.
 * corr (B, Fr) fp64 or NULL: c_t, and 0 where nothing is corrected (every element of the array is written).
 * One wave per row steps over the row 64 frames at a time: an inclusive wavefront scan of the affine maps c -> A * c + B
 * ((1 - alpha, alpha * d), (0, d) on a reset, (0, 0) unvoiced), the carry handed from step to step.  Its grouping differs from
 * the serial order by rounding alone (some 1e-15 a composition, |c| <= 6); with alpha == 1 it is bit for bit.
 * DDSP_ERR_ARG, and nothing launched, for a null f0, mask or param or B, Fr or J < 1.  Does not synchronise, allocate or read
 * back; graph-capturable. */
int ddsp_f0_tune(ddsp_ctx* ctx, void* stream, float* f0, int64_t B, int64_t Fr, const int32_t* n_frames, const int32_t* owner,
                 int64_t J, const int32_t* mask, const double* param, double* corr);

/* UNIT RETRIEVAL: every frame's unit vector, units (rows, Fr, C) fp32 IN PLACE, is blended with a weighted mean of its nearest
 * stored units of a voice's index; it runs between the units encoder and the synthesiser.  A definition of this project (the
 * reference has no such control; RVC calls the blend weight the "index rate").  Every pointer is a DEVICE pointer, read when
 * the kernels run.
 * AN INDEX is vec (N, C) fp32, row-major, N >= 1, C a multiple of 4 and at most 1024, with the derived row
 * nrm[i] = sum_c vec[i][c]^2, formed once by ddsp_units_index_norms in fp32 in a fixed order.  AN INDEX BANK is X indices in one
 * arena: off (X + 1) int64 row offsets, vec (N_total, C), nrm (N_total); N_max is the largest N of the bank (a host number: it
 * sizes the grid and the workspace and forms no address).
 * THE SETTING of a row (a slice offline, a slot's window live), J of them: index_of_row (J) int32 - -1 or anything outside
 * [0, X): none - and ratio_of_row (J) fp32.  Row b takes setting owner[b] (int32; outside [0, J): a padding row, it has none and
 * is not judged), or setting b for owner == NULL (J >= rows then).  One k per call, 1 <= k <= 16; k_eff = min(k, N_x).  n_frames (rows) int32 or NULL: the rows'
 * counts, held in [1, Fr].
 * THE RULE, for a frame x of a row with index x_i and ratio r:
 *     t_i = nrm[i] - 2 * <x, vec[i]>                  the score: it ranks as the squared distance does, |x|^2 being common
 *     the k_eff entries with the smallest t are selected, equal t goes to the smaller entry id; they are ordered by (t, id)
 *     s_j = sum_c (x[c] - vec[j][c])^2                recomputed directly in fp32 in the blend pass, not derived from the score
 *     w_j = 1 / max(s_j, 1e-12)^2, normalised to sum 1   (RVC's inverse square of the squared distance; the floor makes an
 *                                                      exact hit a large finite weight and not a NaN)
 *     y = sum_j w_j vec[j],  out = x + r * (y - x)     in fp32, nothing contracted
 * UNTOUCHED, by selection and not by arithmetic, so their bits stay: rows with no index; rows with r == 0; frames at or past a
 * row's count.  A row's setting is judged only if the row names an index: one with r not finite or outside [0, 1] keeps its
 * bits and raises the device error word (DDSP_ERR_ARG from the next call that takes it, or ddsp_ctx_poll_error).  The index id,
 * the two offsets behind it (0 <= off[x] < off[x+1] <= N_total, else the row has no index) and every entry id are tested before
 * they form an address.
 * nn_id (rows, Fr, k) int32 or NULL: the selected entry ids, local to the row's index, -1 in unused places (all k of an
 * untouched frame); nn_dist (rows, Fr, k) fp32 or NULL: the recomputed s_j, 0 in unused places.  Every element is written.
 * TWO LAUNCHES.  Search: a workgroup takes a tile of 32 query frames of one row and one chunk of the row's index, streams the
 * chunk through the LDS, forms the scores with fp32 MFMA and keeps a running top-k by (t, id) per query; it writes k candidates
 * per (query, chunk) to `workspace`.  The chunk count follows from N_max and the device's CU count.  Merge and blend: one wave
 * per query merges the chunks' candidates by (t, id), gathers the k vectors with 16-byte loads, and stores out, nn_id, nn_dist.
 * workspace: the caller's, at least ddsp_units_retrieve_workspace(R, Fr, k, N_max) bytes for some R >= rows, 16-byte aligned.
 * DDSP_ERR_ARG, and nothing launched, for a null units, index_of_row, ratio_of_row, off, vec, nrm or workspace, rows, Fr or X < 1,
 * rows * Fr or N_total >= 2^31, N_max outside [1, N_total], k outside [1, 16], C no multiple of 4 in 4..1024, or a workspace
 * that is too small.  Does not synchronise, allocate or read back; graph-capturable. */
int ddsp_units_retrieve(ddsp_ctx* ctx, void* stream, float* units, int64_t rows, int64_t Fr, int64_t C, const int32_t* n_frames,
                        const int32_t* owner, int64_t J, const int32_t* index_of_row, const float* ratio_of_row, int64_t X, const int64_t* off, const float* vec,
                        const float* nrm, int64_t N_total, int64_t N_max, int k, void* workspace, int64_t workspace_bytes,
                        int32_t* nn_id, float* nn_dist);
/* *bytes = a workspace that serves every ddsp_units_retrieve call of AT MOST `rows` rows at this Fr, k and N_max on the
 * context's device (a host computation).  It is an upper bound that grows with rows - the exact need, rows * Fr * chunks * k * 8
 * with chunks = ceil(2 CUs / (rows * ceil(Fr / 32))) capped at ceil(N_max / 128), does not, because of the ceil -, so one
 * workspace sized for a bank's S slots serves every narrower width of its ladder. */
int ddsp_units_retrieve_workspace(ddsp_ctx* ctx, int64_t rows, int64_t Fr, int k, int64_t N_max, int64_t* bytes);
/* nrm (N) fp32 = the squared norms of vec (N, C) fp32: one wave per entry, a lane adds the squares of its 16-byte pieces in
 * ascending channel order, then a butterfly over the wave.  One launch; DDSP_ERR_ARG for a null pointer, N < 1 or a bad C. */
int ddsp_units_index_norms(ddsp_ctx* ctx, void* stream, const float* vec, int64_t N, int64_t C, float* nrm);

/* UNIT INDEX REDUCTION: a large index vec (N, C) fp32, finite, is reduced to at most K k-means centres before it is served
 * (`infer_offline.UnitIndex.reduce`).  A definition of this project, like the retrieval rule (RVC reduces with scikit-learn's
 * MiniBatchKMeans, which draws at random; this rule is deterministic); tests/kmeans_cases.py states it in numpy fp64 and Python
 * integers.  C a multiple of 4 in 4..1024, 1 <= K <= N < 2^31, iters >= 0.  Every pointer is a DEVICE pointer; vec and cen are
 * 16-byte aligned (the kernels read them 16 bytes at a time).
 * INITIAL CENTRES: cen[j] = vec[floor(j * N / K)], bit for bit - the `max_entries` subset, so iters = 0 is max_entries = K.
 * ONE ITERATION is three calls on one stream:
 *   1. cnrm = ddsp_units_index_norms(cen)
 *   2. ddsp_units_kmeans_assign: t_ij = cnrm[j] - 2 * <x_i, cen[j]> in fp32 on the fp32 matrix pipe (the retrieval score),
 *      a_i = the j with the smallest (t_ij, j): equal scores go to the smaller centre id.  *moved += the number of entries
 *      whose a_i differs from the value `assign` held before the call (all -1 before the first iteration: N then).
 *   3. ddsp_units_kmeans_update: exact, order-free sums in 64-bit fixed point, so integer atomics give the same bits on every
 *      run.  The HOST forms shift = 62 - E - L with max|vec| < 2^E (the frexp exponent; 0 for an all-zero index) and
 *      L = bit_length(N - 1);  q_ic = (int64) rint(ldexp((double) x_ic, shift));  sum_jc = the sum of q_ic over a_i == j
 *      (|sum| <= 2^62);  n_j = their count.  n_j > 0: cen[j][c] = (float) ldexp((double) sum_jc / (double) n_j, -shift) - the
 *      int64 -> double conversion rounds to nearest even, one fp64 division, one rounding to fp32.  n_j == 0: the centre
 *      keeps its bits.
 * RESULT of iters >= 1 iterations: the centres with n_j > 0 in the last one, in id order; of iters == 0: the K strided rows.
 * No early stop, no read-back between iterations.
 *
 * ddsp_units_kmeans_assign, one launch: assign (N) int32 is READ as the previous assignment and overwritten; moved: one int32,
 * added to.  A workgroup owns a tile of 128 entries and marches over ALL centres in stages of 128 centres x 32 channels through
 * the LDS; every wave forms 64 entries x 64 centres of scores with v_mfma_f32_32x32x2_f32 (centres as A, entries as B: a
 * lane's accumulators are centres of ONE entry) and keeps the entry's running (t, id) minimum in registers.  No candidate
 * lists, no workspace, no merge launch: four lanes see an entry, one thread merges them, stores the int32 and the workgroup
 * adds its moved count with one atomic.  An entry whose every score is NaN (inputs that are not finite) gets -1.
 * DDSP_ERR_ARG, and nothing launched, for a null pointer, N or K < 1, K > N, N >= 2^31, a bad C, or a vec or cen that is not
 * 16-byte aligned. */
int ddsp_units_kmeans_assign(ddsp_ctx* ctx, void* stream, const float* vec, int64_t N, int64_t C, const float* cen,
                             const float* cnrm, int64_t K, int32_t* assign, int32_t* moved);
/* Step 3.  cen (K, C) is updated IN PLACE; count (K) int32 is written, every element.  workspace: at least K * C * 8 bytes,
 * 16-byte aligned; the call zeroes it itself.  Two launches behind two clears: accumulate - a group of C / 4 threads walks a run
 * of neighbouring entries (neighbouring frames, which often share a centre), sums runs of equal assignment in registers and adds
 * each run with 64-bit integer vector atomics - then finalise.  An assignment outside [0, K) is tested before it forms an
 * address: its entry belongs to no centre (-1 is the defined "none").
 * DDSP_ERR_ARG, and nothing launched, for a null pointer, N or K < 1, K > N, N >= 2^31, a bad C, a shift outside [-97, 210]
 * (what the rule can give), a workspace that is too small, or a vec, cen or workspace that is not 16-byte aligned.
 * Neither call synchronises, allocates or reads back; both are graph-capturable. */
int ddsp_units_kmeans_update(ddsp_ctx* ctx, void* stream, const float* vec, int64_t N, int64_t C, const int32_t* assign,
                             int64_t K, int shift, float* cen, int32_t* count, void* workspace, int64_t workspace_bytes);

/* ENVELOPE MIX: the converted output is held to the SOURCE's loudness envelope (`infer_offline.EnvelopeMix`, a job's eighth
 * entry, realtime.StreamBank(envelope=True)).  Not a definition of this project: it restates RVC's
 * `change_rms(data1, sr1, data2, sr2, rate)` (its `rms_mix_rate`; so-vits-svc's "loudness envelope adjustment"), eight lines of
 * librosa and torch.  data1 is the source, data2 the converted output, rate in [0, 1] the share of the OUTPUT's own envelope
 * that is kept: 1 leaves the output as it is, 0 gives it the source's envelope.  tests/envelope_cases.py is the same in numpy fp64.
 * THE RULE, all in fp64, one rounding per operation as written, nothing contracted:
 *   1. FRAME RMS as librosa.feature.rms documents it with center=True: a row of n samples has N = 1 + n / hop frames (integer
 *      division); frame i covers [i * hop - win / 2, i * hop + win / 2), samples outside [0, n) count as 0 ('constant' padding);
 *      rms[i] = sqrt(sum x^2 / win).  win = m * hop with m even, 2 <= m <= 8: RVC's offline frame_length = sr / 2 * 2,
 *      hop_length = sr / 2 is m = 2, hop = sr / 2; its real-time path is hop = sr / 100, m = 4.  The squares of an fp32 source
 *      are exact in fp64.
 *   2. LINEAR INTERPOLATION to the output's length n2, as F.interpolate(mode="linear", align_corners=False) does, of BOTH
 *      envelopes - the source's from its own n1, hop1, N1, the output's from n2, hop2, N2.  For output sample t:
 *          x = max((t + 0.5) * N / n2 - 0.5, 0);  i0 = min(floor(x), N - 1);  i1 = min(i0 + 1, N - 1);  lam = x - i0
 *          e = (1 - lam) * env[i0] + lam * env[i1]
 *   3. GAIN: e2 = max(e2, 1e-6) behind the interpolation, as RVC has it; g = e1^(1 - rate) * e2^(rate - 1);
 *      out[t] = data2[t] * g.
 * Nothing is added: no smoothing, no cap on the gain (a quiet output frame under a loud source frame is raised by up to
 * (e1 * 1e6)^(1 - rate)).  e1 == 0 with rate < 1 gives a gain of exactly 0: a SILENT SOURCE SILENCES THE OUTPUT, as in RVC.
 *
 * THE ROWS of both calls come in one of two forms.  MATRIX: an fp32 matrix (R, T) with counts n (R) int32 DEVICE or NULL (T for
 * every row); a count is held inside [0, T].  SPANS: an fp64 tensor of `total` elements with a DEVICE table spans (R, 2) int64
 * of (base, count) per row - the job spans of a stitched tensor.  A span with base < 0, count < 1 or base + count > total, or
 * with more samples than the call's width (N_max frames, n_max samples) is refused on the device: the error word is raised,
 * nothing of it is read or written (its envelope is 0).  Exactly one of the two data pointers is non-NULL.  R <= 65535.
 *
 * ddsp_envelope_rms: env (R, N_max) fp64 = the frame RMS of every row, 0 at and behind frame N of a row; blocks (R, N_max) fp64
 * is the caller's workspace.  MATRIX needs N_max >= 1 + T / hop.  Two kernels, no allocation: win = m * hop, so a frame is the
 * sum of m consecutive hop-blocks [k * hop, (k + 1) * hop); the first kernel forms one fp64 sum of squares per (row, block) with
 * every sample read from memory once - 16-byte loads wherever the whole vector lies inside the block at an aligned address, a
 * bounds select at its ends; the padding behind a count and between spans is never read -, the second sums the m blocks of a
 * frame in ascending order.  From hop >= 2048 a workgroup strides one block, below a wave does and a workgroup takes 16 blocks.
 * The order of every sum is fixed by that shape (strided terms per lane, a shuffle butterfly, a tree over the waves; no
 * floating-point atomics): the same input gives the same bits on every run.  It differs from numpy's pairwise order by at most
 * terms * 2^-53 relative.
 *
 * ddsp_envelope_apply: in place on the output rows (y64 with spans, or y32 (R, T) with n_out), steps 2 and 3.  env_out
 * (R, N_out_max) and env_src (R_src, N_src_max) are ddsp_envelope_rms results at hop_out and hop_src; N_out_max >= 1 + n_max /
 * hop_out, n_max the longest output row (T for MATRIX).  The source of row r is src_of_row[r] (int32) or r; its count n1 is
 * n_src[source] (int32) or n_src_all for NULL; its frames N1 = 1 + n1 / hop_src are held to N_src_max.  The rate of row r is
 * rate[owner[r]] (fp64, J of them; owner int32) or rate[r] for owner == NULL - a job offline, a slot live.
 * UNTOUCHED, by selection and not by arithmetic, so their bits stay: rows whose rate is exactly 1 (0^0 is never formed); rows
 * whose owner is -1 (padding: no error); elements outside every span or behind a row's count.
 * REFUSED on the device - the row keeps its bits, the error word is raised (DDSP_ERR_ARG from the next call that takes it, or
 * ddsp_ctx_poll_error), the other rows are done -: a rate that is not finite or outside [0, 1]; an owner other than -1 outside
 * [0, J); a source row outside [0, R_src); n1 < 1; a bad span.  Every row index, base and count is tested before it forms an
 * address.  An element reads its one or two entries of each envelope from memory (a few KB per row, shared by the lanes of a
 * wave: they stay in the cache; nothing is staged in the LDS).
 * Both: DDSP_ERR_ARG, and nothing launched, for a null pointer, both or neither data pointer, a hop outside [1, 2^27], an m
 * other than 2, 4, 6, 8 or widths that do not fit.  They do not synchronise, allocate or read back; graph-capturable. */
int ddsp_envelope_rms(ddsp_ctx* ctx, void* stream, const float* x32, int64_t T, const int32_t* n_samples, const double* x64,
                      int64_t total, const int64_t* spans, int64_t R, int64_t hop, int m, int64_t N_max, double* blocks,
                      double* env);
int ddsp_envelope_apply(ddsp_ctx* ctx, void* stream, double* y64, int64_t total, const int64_t* spans, float* y32, int64_t T,
                        const int32_t* n_out, int64_t R, int64_t n_max, const double* env_out, int64_t N_out_max, int64_t hop_out,
                        const double* env_src, int64_t R_src, int64_t N_src_max, int64_t hop_src, const int32_t* n_src,
                        int64_t n_src_all, const int32_t* src_of_row, const int32_t* owner, const double* rate, int64_t J);

/* The row movers of a bank with a model per slot (realtime.StreamBank, `models=`): the analysis of a call runs once over its row
 * batch of R rows, then every model renders its own rows as a compact batch of W rows.  rows (W) int32 DEVICE, read when the
 * kernels run: entry r is the row OF THE CALL'S BATCH (not a slot) behind compact row r.  An entry is tested against [0, R)
 * before it forms an address; -1 or any other entry outside is a padding row: never a fault, and the error word stays clear.
 * ddsp_bank_features_gather, one launch: for every compact row r with s = rows[r], cunits[r] = units[s] (Fr * C), cf0[r] =
 *   f0[s] (Fr), cvolume[r] = volume[s] (Fr), cnoise[r] = noise[s] (T, the injected excitation; both NULL: none), cmix_ids[r] /
 *   cmix_w[r] = mix_ids[s] / mix_w[s] (K, 1 <= K <= 16).  A padding row gets zero units, f0 0, volume 0, noise 0 and speaker 1
 *   with weight 1.  The batch's tensors have R rows, the compact ones W, and the compact ones lie outside the batch's, so the
 *   launch reads nothing that it writes.  Each segment moves by 16-byte vector accesses when its row length is a multiple of 4
 *   floats and its two bases are 16-byte aligned (Fr * C with C % 4 == 0 and T usually are, Fr alone often is not), else by
 *   single words.
 * ddsp_bank_signal_scatter: sig[rows[r]] = csig[r] (T) for every compact row that is no padding; csig (W, T), sig (R, T).  No
 *   row of the batch may be named twice (every row belongs to one model; the caller sees to it).  A row that `rows` does not
 *   name is not written.
 * DDSP_ERR_ARG, and nothing written, for W or R outside [1, DDSP_MAX_STREAMS], a null pointer, or overlapping tensors. */
int ddsp_bank_features_gather(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int R, int64_t Fr, int64_t C, int64_t T,
                              const float* units, const float* f0, const float* volume, const float* noise,
                              const int32_t* mix_ids, const float* mix_w, int K, float* cunits, float* cf0, float* cvolume,
                              float* cnoise, int32_t* cmix_ids, float* cmix_w);
int ddsp_bank_signal_scatter(ddsp_ctx* ctx, void* stream, const int32_t* rows, int W, int R, const float* csig, int64_t T,
                             float* sig);

/* ---- a15: volume gate ------------------------------------------------------------------------ */
/* replaces gui.py:14-31 `phase_vocoder(a, b, fade_out, fade_in)` (the optional cross-fade of gui.py:417-423; SURVEY
 * 8(f) rank 3): a = kept tail, b = head of the new block, out, all (S, n) as for ddsp_sola; the fade windows (n) are shared.
 * n <= 65536. */
int ddsp_phase_vocoder(ddsp_ctx* ctx, void* stream, const float* a, const float* b, const float* fade_out,
                       const float* fade_in, int S, int n, float* out);

/* replaces main.py:111-116,159 / gui.py:108-112,127: signal (B,T) *= upsample(dilate9(volume > threshold)),
 * in place (threshold = 10^(dB/20), linear); volume (B,Fr). */
int ddsp_volume_gate(ddsp_ctx* ctx, void* stream, float* signal, const float* volume, float threshold, int64_t B,
                     int64_t Fr, int hop);
/* The same gate for a RAGGED batch of slices of one file, in one launch: signal (B, T_max) in place, volume (Fr) of the WHOLE
 * file, start_frame / n_frames (B) int32 DEVICE arrays.  Row b, sample t < n_frames[b] * hop, is multiplied by the file's gate
 * at sample start_frame[b] * hop + t - the value ddsp_volume_gate computes there (one device function serves both kernels), so
 * the dilation sees the slice's neighbours and the last frame of a slice interpolates towards the file's next frame.  Samples
 * from n_frames[b] * hop on are not touched.  T_max >= 1; hop a power of two.  A row with start_frame < 0, n_frames < 0,
 * start_frame + n_frames > Fr or n_frames * hop > T_max is left as it is and sets the context's device error word
 * (DDSP_ERR_ARG from ddsp_ctx_poll_error or the next call that takes it). */
int ddsp_volume_gate_rows(ddsp_ctx* ctx, void* stream, float* signal, const float* volume, const int32_t* start_frame,
                          const int32_t* n_frames, float threshold, int64_t B, int64_t T_max, int64_t Fr, int hop);
/* The gate for a ragged batch whose rows are slices of SEVERAL files: volume (F, Fr_max) holds the files' tracks padded,
 * file_frames (F) int32 DEVICE their own frame counts (1 <= file_frames[f] <= Fr_max), file (B) int32 DEVICE the file of every
 * row.  Row b is gated as ddsp_volume_gate_rows gates it with file[b]'s track of file_frames[file[b]] frames alone (one kernel
 * and one device function serve both calls): the 9-frame dilation and its edge padding stop at the file's OWN first and last
 * frame, and the file's last frame interpolates as in a solo call; what lies behind a file's frames is never read.  A row with
 * file[b] outside [0, F), a file count outside [1, Fr_max], or frames outside its file or its own row is left as it is and sets
 * the context's device error word like a bad row of ddsp_volume_gate_rows. */
int ddsp_volume_gate_files(ddsp_ctx* ctx, void* stream, float* signal, const float* volume, const int32_t* file_frames, int64_t F,
                           const int32_t* file, const int32_t* start_frame, const int32_t* n_frames, float threshold, int64_t B,
                           int64_t T_max, int64_t Fr_max, int hop);

/* ---- the rows of a ragged group from several files (main.py:143-159, one slice of one file at a time there) -------------
 * ONE launch forms R rows from a padded batch of F files: audio (F, T_max), f0 and volume (F, Fr_max), key_factor (F) fp32,
 * n_file_samples / n_file_frames (F) int32 the files' own counts, table (R, 5) int32 rows (file, start_frame, n_frames,
 * start_sample, n_samples), all DEVICE arrays.  The host forms the sample range (the hop may be fractional: int(start_frame *
 * hop_size), as main.split snaps).
 *   wav (R, S_max):      wav[r][j] = audio[file][start_sample + j] for j < n_samples, exactly 0 after;
 *   f0_rows (R, N_max):  f0[file][start_frame + j] * key_factor[file] for j < n_frames - ONE rounded fp32 product per element,
 *                        contracted with nothing -, exactly 0 after;
 *   vol_rows (R, N_max): volume[file][start_frame + j] for j < n_frames, exactly 0 after.
 * audio and wav may both be NULL (no sample rows: table columns 3, 4 are ignored), or f0, volume, key_factor, f0_rows and
 * vol_rows all NULL (no frame rows: columns 1, 2 are ignored); volume and vol_rows alone may be NULL too (the f0 rows without
 * the volume rows, as the enhancer takes them).  16-byte loads and stores where a run of four lies inside the
 * piece (the row) at an aligned address, a scalar select elsewhere: no address outside a file's own row of audio, f0 or volume is
 * formed.  A row with file outside [0, F), a negative number, a range that leaves its file's counts, n_samples > S_max or
 * n_frames > N_max is written as zeros and sets the context's device error word (DDSP_ERR_ARG from ddsp_ctx_poll_error or the
 * next call that takes it).  R <= 65535.  Does not synchronise, allocate or read back. */
int ddsp_pieces_gather(ddsp_ctx* ctx, void* stream, const float* audio, const float* f0, const float* volume,
                       const float* key_factor, const int32_t* n_file_samples, const int32_t* n_file_frames, int64_t F,
                       int64_t T_max, int64_t Fr_max, const int32_t* table, int64_t R, int64_t S_max, int64_t N_max, float* wav,
                       float* f0_rows, float* vol_rows);
/* The same launch for the rows of JOBS - a job is one conversion of a file to one voice and key, and several jobs may share
 * a file: table (R, 6) int32 rows (file, start_frame, n_frames, start_sample, n_samples, job) and key_factor (J) fp32 by JOB.
 * The file names the source of audio, f0 and volume - read in place, never copied per job -, the job names the key factor:
 * f0_rows[r][j] = f0[file][start_frame + j] * key_factor[job].  A job outside [0, J) is a bad row like a file outside [0, F)
 * (tested before key_factor is indexed): zeros and the device error word.  Everything else as above. */
int ddsp_pieces_gather_jobs(ddsp_ctx* ctx, void* stream, const float* audio, const float* f0, const float* volume,
                            const float* key_factor, const int32_t* n_file_samples, const int32_t* n_file_frames, int64_t F,
                            int64_t T_max, int64_t Fr_max, int64_t J, const int32_t* table, int64_t R, int64_t S_max,
                            int64_t N_max, float* wav, float* f0_rows, float* vol_rows);
/* The rows of jobs whose KEY moves over the file: ddsp_pieces_gather_jobs with a breakpoint range per job in place of
 * key_factor (J).  THE KEY TIMELINE RULE (csrc/key_timeline.h; ddsp_bank_key_glide applies it too): a timeline is n >= 1
 * breakpoints with times strictly increasing, each with its key in semitones (fp32) and the f0 factor the host formed for it,
 * 2 ** (key / 12) stored to fp32 - what key_factor holds for a constant key.  The key at time tau is linear in semitones between
 * two breakpoints, the first one's before them and the last one's after them.  The STORED factor of a breakpoint is used where no
 * slope is at work: tau before the first breakpoint (the first one's), behind the last (the last one's), exactly on a breakpoint
 * (its own), or between two of equal semitones (the earlier one's).  Elsewhere the factor is
 * exp2((s0 + (s1 - s0) * ((tau - t0) / (t1 - t0))) / 12.0) in fp64, every step one rounded operation, rounded to fp32.  So a
 * one-breakpoint timeline, and every constant stretch, multiplies with the bits of the constant key.
 * Job j owns the breakpoints bp_off[j] .. bp_off[j + 1] - 1 (bp_off (J + 1) int32, a prefix table): bp_frame (P) int32 their
 * positions in FILE frames, strictly increasing inside a job, bp_semi (P) and bp_fac (P) fp32.  Frame t < n_frames of row r is
 * file frame start_frame + t: f0_rows[r][t] = f0[file][start_frame + t] * factor(start_frame + t), one rounded fp32 product;
 * exact zeros behind n_frames.  wav and vol_rows are ddsp_pieces_gather_jobs' bits.  A job outside [0, J), or one whose
 * breakpoint range is empty or leaves [0, P), is tested before any address is formed from it: zeros and the device error word,
 * like a file outside [0, F).  f0, f0_rows (and volume, vol_rows) may be NULL as above; the breakpoint tables never.  1 <= P <
 * 2^31.  Everything else as above. */
int ddsp_pieces_gather_keys(ddsp_ctx* ctx, void* stream, const float* audio, const float* f0, const float* volume,
                            const int32_t* bp_off, const int32_t* bp_frame, const float* bp_semi, const float* bp_fac, int64_t P,
                            const int32_t* n_file_samples, const int32_t* n_file_frames, int64_t F, int64_t T_max,
                            int64_t Fr_max, int64_t J, const int32_t* table, int64_t R, int64_t S_max, int64_t N_max, float* wav,
                            float* f0_rows, float* vol_rows);
/* The speaker timelines of jobs -> the per-frame mix of one render group (ddsp_unit2ctrl_fwd_framemix's tables), one launch.
 * table (R, 6) as above.  Job j owns the breakpoints bp_off[j] .. bp_off[j + 1] - 1 (bp_off (J + 1) int32, a prefix table):
 * bp_frame (P) int32 their positions in FILE frames, strictly increasing inside a job; bp_w (P, K) fp32 the weights of the
 * job's K slots there; job_ids (J, K) int32 the slots' 1-based speaker ids.  ids_rows (R, K) = job_ids[job]; w_rows
 * (R, N_max, K): frame t < n_frames of row r is file frame f = start_frame + t and gets the piecewise-linear interpolation of
 * its job's breakpoints at f - constant before the first and after the last, so one breakpoint is a constant mix -, computed
 * in fp64 as w0 + (w1 - w0) * ((f - f0) / (f1 - f0)) and rounded to fp32; frames t >= n_frames get exact zeros.  A job outside
 * [0, J), or a breakpoint range that is empty or leaves [0, P), is tested before it forms an address: such a row is a padding
 * row, ids 1 and weights 0 (no error word).  R <= 65535, 1 <= K <= 16.  Does not synchronise, allocate or read back. */
int ddsp_mix_timeline(ddsp_ctx* ctx, void* stream, const int32_t* table, int64_t R, int64_t J, const int32_t* bp_off,
                      const int32_t* bp_frame, const float* bp_w, int64_t P, const int32_t* job_ids, int K, int64_t N_max,
                      int32_t* ids_rows, float* w_rows);

/* ---- the stitch of an offline conversion (main.py:165-173 with `cross_fade`, main.py:50-57) ----------------------------
 * Places S rendered pieces into one fp64 output in ONE launch.  `pieces` is a DEVICE table of S rows; piece i holds `len`
 * fp32 samples at the device address `x` (a row of a ragged group tensor, or a tensor of its own: nothing is packed first),
 * starts at output sample `p` and cross-fades its first `fade` samples with what the earlier pieces left there.  Output sample
 * t is a fold over the pieces in order from v = 0: for each i with p <= t < p + len and j = t - p,
 *     j <  fade:  v = (1 - k) * v + k * x[j],  k = numpy's linspace(0, 1, fade)[j] in fp64: j * (1 / (fade - 1)), the last
 *                 element exactly 1, and 0 for fade == 1 (a one-sample fade keeps the earlier sample);
 *     j >= fade:  v = x[j] converted to fp64.
 * Every step of the blend is one rounded fp64 operation (nothing is contracted), so the output equals the reference's host
 * loop bit for bit; a sample no piece covers is 0.
 * The caller guarantees (the Python mirror's `stitch_plan` checks it on the host): len >= 1, p nondecreasing, fade =
 * max(0, end of piece i-1 - p) <= len - so the ends p + len are nondecreasing too, and a workgroup finds its first piece by
 * binary search on them - and total >= every end.  A table that breaks this gives wrong samples, but no write leaves
 * out[0, total) and no read leaves x[0, len) of a piece.  out (total) fp64, 16-byte aligned; 16-byte stores, and 16-byte loads
 * wherever four output samples lie inside one piece at a 16-byte aligned address (a scalar select elsewhere: no address outside
 * a piece is formed).  total == 0 launches nothing.  Does not synchronise, allocate or read back. */
typedef struct ddsp_stitch_piece {
    const float* x;
    int64_t p, len, fade;
} ddsp_stitch_piece;
int ddsp_stitch(ddsp_ctx* ctx, void* stream, const ddsp_stitch_piece* pieces, int64_t S, double* out, int64_t total);

/* ---- 16-bit PCM of a stitched waveform (what the offline command line writes into a .wav) --------------------------------
 * ONE pass over x (n) fp64: out[t] = clip(rint(x[t] * 32768), -32768, 32767) as int16, rint rounding half to even - numpy's
 * `np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)` bit for bit for every finite x (NaN is out of contract, as
 * numpy's cast is undefined there).  spans (J, 2) int64 DEVICE rows (base, total), ascending and disjoint (the layout of
 * `stitch_plan_many`: bases even), or NULL: the one span (0, n), J ignored.  A sample inside no span is written as 0.
 * peak (J) fp64 and clipped (J) int64, each or both NULL: per span the largest |x| and the number of samples whose
 * rint(x * 32768) lies outside [-32768, 32767]; the call zeroes them on the stream first, then every workgroup adds its part
 * with one atomic max and one atomic add per span it touches (wave shuffles and an LDS step in front).  x needs 8-byte
 * alignment only: 16-byte loads where four samples lie before n at a 16-byte aligned address, 8-byte words elsewhere.  A span
 * entry decides which samples count, never an address: whatever the table holds, nothing outside x[0, n) and out[0, n) is
 * touched.  n == 0 launches nothing.  Does not synchronise, allocate or read back. */
int ddsp_pcm16(ddsp_ctx* ctx, void* stream, const double* x, int64_t n, const int64_t* spans, int64_t J, int16_t* out,
               double* peak, int64_t* clipped);

/* ---- the device-side steps immediately before the synthesis path ------------- */
/* replaces ddsp/vocoder.py:116-137 `Volume_Extractor.extract`: audio (B,T) -> volume (B, T/hop + 1), the RMS of
 * non-overlapping hop-sized blocks of the signal reflect-padded by (hop/2, (hop+1)/2) (numpy 'reflect': T must
 * exceed (hop+1)/2).
 * n_samples: NULL, or a ragged batch - a DEVICE array of B int32 (the caller checks (hop+1)/2 < n_samples[b] <= T); row b then
 * reflects at its own ends (i >= n_b -> 2 (n_b - 1) - i), has n_samples[b] / hop + 1 frames and exact zeros after them;
 * audio[b][i] for i >= n_samples[b] is never read. */
int ddsp_volume_extract(ddsp_ctx* ctx, void* stream, const float* audio, int64_t B, int64_t T, const int32_t* n_samples, int hop,
                        float* volume);
/* ddsp_volume_extract at the non-integral hop `block_size * sample_rate / model_rate` that an input at another rate than the model's
 * gives (main.py:72,109, gui.py:94): volume (B, int(T // hop_size) + 1), block n = padded[int(n * hop_size) :
 * int((n + 1) * hop_size)] of the signal reflect-padded by (int(hop_size // 2), int((hop_size + 1) // 2)), all in fp64
 * like the reference's Python floats; each block's mean divides by its own length.  1 <= hop_size <= 2^20, and T must
 * exceed int((hop_size + 1) // 2).  An integral hop_size gives exactly what ddsp_volume_extract gives. */
int ddsp_volume_extract_frac(ddsp_ctx* ctx, void* stream, const float* audio, int64_t B, int64_t T, double hop_size,
                             float* volume);
/* replaces the alignment tail of ddsp/vocoder.py:201-211 `Units_Encoder.encode`: out[b][i][:] = units[b][j][:] with
 * j = min(rint(ratio * i), Lu - 1), ratio = (hop/sample_rate) / (encoder_hop/encoder_sample_rate) as fp32, rint =
 * round half to even (torch.round); units (B,Lu,C) -> out (B,n_frames,C).
 * n_units, n_out: both NULL, or (a ragged batch) DEVICE arrays of B int32: row b has n_out[b] <= n_frames frames of its own,
 * taken from its own n_units[b] <= Lu unit rows (j = min(rint(ratio * i), n_units[b] - 1)), and exact zeros from frame n_out[b]
 * on. */
int ddsp_align_units(ddsp_ctx* ctx, void* stream, const float* units, int64_t B, int64_t Lu, int64_t C, int64_t n_frames,
                     float ratio, const int32_t* n_units, const int32_t* n_out, float* out);

/* replaces the host-side f0 re-timing of enhancer.py:56-62 (`f0_np *= real_factor`; `np.interp(time_frame, time_org, f0_np,
 * left=f0_np[0], right=f0_np[-1])`): out[i] = interp(i * step_dst) over the knots x_j = (step_num * j) / div with values
 * fl32(f0[j] * scale), evaluated in fp64 like numpy; f0 (n_src,) -> out (n_dst,) with B = 1 and n_src_rows = n_dst_rows = NULL.
 * No host copy of the track.
 * A ragged batch (n_src_rows, n_dst_rows: both or neither, DEVICE arrays of B int32; n_dst >= 1): f0 (B, n_src) -> out (B, n_dst);
 * row b has n_src_rows[b] <= n_src knots and n_dst_rows[b] <= n_dst targets of its own: the ends are held at the row's own first
 * and last frame, f0 past the row's knots is never read, and the outputs from n_dst_rows[b] on are 0. */
int ddsp_retime_f0(ddsp_ctx* ctx, void* stream, const float* f0, int64_t B, int64_t n_src, const int32_t* n_src_rows,
                   double step_num, double div, float scale, double step_dst, int64_t n_dst, const int32_t* n_dst_rows, float* out);
/* A ragged ddsp_retime_f0 with the (div, scale) of row b taken from two DEVICE tables of n_keys entries by the row's key,
 * key[b] (a DEVICE array of B int32, clamped into 0..n_keys-1 before it indexes anything): per row what
 * ddsp_retime_f0 gives with div_by_key[key[b]] (fp64) and scale_by_key[key[b]] (fp32). */
int ddsp_retime_f0_keyed(ddsp_ctx* ctx, void* stream, const float* f0, int64_t B, int64_t n_src, const int32_t* n_src_rows,
                         double step_num, const int32_t* key, int n_keys, const double* div_by_key, const float* scale_by_key,
                         double step_dst, int64_t n_dst, const int32_t* n_dst_rows, float* out);

/* the adaptive key of `Enhancer.enhance` (enhancer.py:34-38) for S rows, decided on the device: f0 (S, Fr) -> key (S) int32 in
 * [0, max_key], 0 <= max_key <= 12.  request (S) int32: -1 = 'auto', k >= 0 = that key (clamped to max_key).  'auto': with
 * f0max the highest f0 of the row's frames from cut_frames on and q = fl32(f0max / 760) (an IEEE fp32 division), the first k
 * with q <= thresholds[k], max_key when there is none, 0 when f0max <= 0.  thresholds: DEVICE array of max_key + 1 fp32, the
 * largest fp32 value <= 2^(k/12) each (the caller rounds them from fp64): the comparison decides ceil(12 log2 q) <= k exactly
 * as the reference's numpy expression does, without a device log2.  DIVERGENCE: the reference has no max_key (its key is
 * unbounded); a keyed batch needs a finite set of working rates, so keys above max_key are clamped to it. */
int ddsp_enhancer_keys(ddsp_ctx* ctx, void* stream, const float* f0, int64_t S, int64_t Fr, int64_t cut_frames, int max_key,
                       const int32_t* request, const float* thresholds, int32_t* key);

/* ---- sample-rate conversion ------------------------------------------------------ */
/* replaces `torchaudio.transforms.Resample(orig_freq, new_freq, lowpass_filter_width)` as the reference uses it (gui.py:399-404,
 * enhancer.py:50-53,69-73; windowed-sinc polyphase, Hann window, rolloff 0.99 - torchaudio's published algorithm; the package
 * is not in the image, so parity at that boundary is unpinned): x (B,T) -> out (B, ddsp_resample_length(T, orig, new)).
 * The tap table of a rate pair is built on first use and cached in the context. */
int64_t ddsp_resample_length(int64_t T, int orig_freq, int new_freq);
/* n_samples: NULL, or a ragged batch - a DEVICE array of B int32, row b holds n_samples[b] <= T samples of its own.
 * x[b][i] is selected as 0 for i >= n_samples[b] where it is loaded (the padding may hold anything), so the row's
 * first ddsp_resample_length(n_samples[b], ...) outputs are those of the row resampled alone; the outputs after them are 0. */
int ddsp_resample(ddsp_ctx* ctx, void* stream, const float* x, int64_t B, int64_t T, const int32_t* n_samples, int orig_freq,
                  int new_freq, int lowpass_filter_width, float* out);
/* Keyed batches: one launch in which row b is resampled with the rate pair key[b] of a set of up to 13 pairs with one lowpass
 * width (the enhancer's working rates, one per adaptive key).
 * ddsp_resample_keyed_plan builds the set: the tap tables of all its pairs, the ones ddsp_resample builds for each pair, in
 *   one allocation owned by the plan.  They are ready when the call returns (it waits for the stream), stay resident
 *   together until ddsp_resample_keyed_plan_destroy, and are outside the context's cache of solo tables, which can neither
 *   evict them nor be filled by them.  A plan belongs to the context's DEVICE, not to the context: any context of that
 *   device may run it, a captured one included (build the plan before the capture).  A pair with orig == new copies the row.
 * ddsp_resample_keyed_length: the padded output width for inputs of width T, the largest ddsp_resample_length over the pairs.
 * ddsp_resample_keyed: x (B, T), n_samples and key DEVICE arrays of B int32 -> out (B, ddsp_resample_keyed_length(plan, T)).
 *   With k = key[b] clamped into the set (before it indexes anything), the row's first
 *   ddsp_resample_length(n_samples[b], orig[k], new[k]) outputs are bit for bit those of ddsp_resample of that row alone at
 *   that pair (same taps, same kernel body, same summation order) and every output after them is 0; x past n_samples[b] is
 *   never read into arithmetic.  The grid and the LDS are sized for the largest pair; the pair is uniform per workgroup. */
typedef struct ddsp_resample_plan ddsp_resample_plan;
int ddsp_resample_keyed_plan(ddsp_ctx* ctx, void* stream, int n_pairs, const int* orig_freq, const int* new_freq,
                             int lowpass_filter_width, ddsp_resample_plan** plan);
void ddsp_resample_keyed_plan_destroy(ddsp_resample_plan* plan);
int64_t ddsp_resample_keyed_length(const ddsp_resample_plan* plan, int64_t T);
int ddsp_resample_keyed(ddsp_ctx* ctx, void* stream, const ddsp_resample_plan* plan, const float* x, int64_t B, int64_t T,
                        const int32_t* n_samples, const int32_t* key, float* out);

/* ---- the NSF-HiFiGAN post-net (enhancer.py:24-101, nsf_hifigan/models.py:106-276, nvSTFT.py:65-119) ---- */
/* One utterance per call (B = 1, n_frames = NULL, frame_scale = 1), or a padded batch of rows of different length ("Ragged
 * batches of the post-net" below); activations frame-major (T, C) fp32.
 * ddsp_conv1d: replaces `Conv1d(Cin, Cout, k, dilation=d, padding="same")(leaky_relu(x, in_slope))` (+ residual): the
 *   resblock convolutions (models.py:45-77), conv_pre (:234) and - with weights packed as the host mirror's
 *   `_pack_conv_transpose` does - the ConvTranspose1d upsamplers (:240-243).  x (T,Cin), w_packed (Cout, k*Cin) with column
 *   tap*Cin + ci, bias (Cout) or NULL, residual (T,Cout) or NULL; in_slope = 1 applies no activation.  The result y goes to
 *   out (T,Cout) and / or, as leaky_relu(y, act_slope), to out_act (either may be NULL): every convolution of the generator
 *   reads an activated input, so a producer that emits it lets the consumer run with in_slope = 1 - and only then (with
 *   Cin % 32 == 0) does the convolution run on the LDS-DMA GEMM in the context's product arithmetic; otherwise on the
 *   register-staged fp32 kernel, which activates while loading.  Split layout (split-bf16 arithmetic only): every group of 8
 *   consecutive floats of a row replaced by its 8 bf16 high parts and 8 bf16 remainders (32 bytes, same footprint) - what the
 *   matrix instructions consume; w_split is w_packed in that layout (the host mirror converts once at load), flags say
 *   whether x arrives so and whether out_act is to be written so (Cout % 64 == 0): a chain of convolutions then converts
 *   every activation once, where it is produced, instead of once per tile that reads it.
 * ddsp_nsf_source: replaces `SourceModuleHnNSF.forward(f0, upp)` (:180-216 with `SineGen` :106-177, 9 harmonics): f0 (L) Hz per
 *   frame, rand_ini (9) the harmonics' initial phases in cycles (the reference's torch.rand draw, element 0 = 0), lin_w (9),
 *   lin_b (1) of `l_linear`; out (L*upp) = tanh(linear(sine_amp * sin(2 pi cumsum(f0 h / sr)))).
 * ddsp_nsf_noise_conv: replaces `noise_convs[i]` (:244-249), a Conv1d(1, C, K, stride, padding=pad) on the source signal:
 *   src (T_src), w (C,K), b (C) -> out (T_out, C).
 * ddsp_nsf_post: replaces `tanh(conv_post(leaky_relu(x, slope)))` (:268-270): x (T,C), w (K,C) tap-major, b (1) -> out (T).
 * ddsp_nsf_mean: (a [+ b [+ c]]) / n_terms elementwise - the mean over a stage's residual blocks (:259-266) - to out and / or,
 *   activated, to out_act (as in ddsp_conv1d).
 * ddsp_log_mel: replaces the spectral half of `STFT.get_mel` (nvSTFT.py:100-117): frames (n_frames, n_fft) of the padded
 *   signal, dft_table (2*ldm, n_fft) rows (w cos, -w sin) per bin with ldm = bins rounded up to 4, mel_basis (n_mels, ldm);
 *   out (n_frames, n_mels) = log(max(mel . sqrt(re^2 + im^2 + 1e-9), clip)). */
#define DDSP_CONV_X_SPLIT 1   /* x is in the split layout (written so by a producer with DDSP_CONV_ACT_SPLIT) */
#define DDSP_CONV_ACT_SPLIT 2 /* write out_act in the split layout */
int ddsp_conv1d(ddsp_ctx* ctx, void* stream, const float* x, const float* w_packed, const float* bias, int64_t B, int64_t T,
                int Cin, int Cout, int ktaps, int dil, float in_slope, const float* residual, float* out, float* out_act,
                float act_slope, const float* w_split, int flags, const int32_t* n_frames, int frame_scale);
/* One residual pair of `ResBlock1` (nsf_hifigan/models.py:41-90: xt = c1(leaky_relu(x)); xt = c2(leaky_relu(xt)); x = xt + x) of a
 * narrow stage in one launch: x (T,C) raw, c1 with `dil`, c2 with dilation 1, both `ktaps` taps, weights packed as for
 * ddsp_conv1d; out = the new x, out_act = leaky_relu(out, slope) (either may be null).  Only x is read and the results
 * written: the activations happen on load and c1's output stays in the LDS.  Products follow the context's arithmetic.
 * ddsp_conv1d_pair_supported: 1 when (C, ktaps, dil) is a geometry the fused kernel takes (else use two ddsp_conv1d calls). */
int ddsp_conv1d_pair_supported(ddsp_ctx* ctx, int C, int ktaps, int dil);
int ddsp_conv1d_pair(ddsp_ctx* ctx, void* stream, const float* x, const float* w1, const float* b1, const float* w2,
                     const float* b2, int64_t B, int64_t T, int C, int ktaps, int dil, float slope, float* out, float* out_act,
                     const int32_t* n_frames, int frame_scale);

int ddsp_nsf_source(ddsp_ctx* ctx, void* stream, const float* f0, const float* rand_ini, const float* lin_w,
                    const float* lin_b, int64_t B, int64_t L, int upp, int sr, float sine_amp, const int32_t* n_frames,
                    float* out);
int ddsp_nsf_noise_conv(ddsp_ctx* ctx, void* stream, const float* src, int64_t B, int64_t T_src, const float* w, const float* b,
                        int C, int K, int stride, int pad, int64_t T_out, float* out);
int ddsp_nsf_post(ddsp_ctx* ctx, void* stream, const float* x, const float* w, const float* b, int64_t B, int64_t T, int C, int K,
                  float slope, float* out, const int32_t* n_frames, int frame_scale);
int ddsp_nsf_mean(ddsp_ctx* ctx, void* stream, const float* a, const float* b, const float* c, int n_terms, int64_t n,
                  float* out, float* out_act, float act_slope, int flags);
int ddsp_log_mel(ddsp_ctx* ctx, void* stream, const float* frames, const float* dft_table, const float* mel_basis,
                 int64_t n_frames, int n_fft, int n_mels, float clip, float* out);
/* Ragged batches of the post-net (inference): B rows of different length as ONE padded batch, flattened on the time axis.
 * Activations are (B * T, C): row b owns the T frames from b * T on and is valid for its first T_b = n_frames[b] * frame_scale
 * of them (n_frames: a DEVICE array of B int32, 1 <= n_frames[b] <= T / frame_scale, uploaded once and never read back, so the
 * calls can be captured in a HIP graph; frame_scale = the product of the upsampling rates so far; T % frame_scale == 0).
 * n_frames = NULL is a rectangular batch: every row T long.  The contract, one rule throughout:
 *   - every tensor a convolution READS (x, and what a residual adds) must be exactly 0 at t >= T_b;
 *   - every entry point WRITES exactly 0 at t >= T_b of each output, whatever bias, residual or source would put there.
 * A tap that leaves [0, T_b) then reads 0 as a solo call's "same" padding does, and no tap reaches a neighbouring row, so
 * row b of each output is, over [0, T_b), what the solo entry point returns for that row alone at its own length.  A caller
 * whose first input may hold anything past T_b zeroes it first (ddsp_ragged_frames with hold = 0).
 * ddsp_conv1d: x (B*T, Cin), residual / out / out_act (B*T, Cout).  For a transposed convolution in its 3-tap form
 *   the (B*T, u*Cout) result is the (B*T*u, Cout) output, row t holding samples t*u .. t*u+u-1 of the same batch row: the mask
 *   stays per input row (frame_scale of the INPUT).
 * ddsp_conv1d_pair: windows are cut per batch row, halo reads stop at the row's own ends, and the intermediate
 *   leaky_relu(c1(x) + b1) is zeroed at t >= T_b before c2 reads it.
 * ddsp_nsf_source: f0 (B, L), rand_ini (B, 9): one phase scan per row from the row's own initial phases; f0 past
 *   n_frames[b] is never read; out (B, L*upp) is 0 from n_frames[b] * upp on.
 * ddsp_nsf_noise_conv: src (B, T_src) -> out (B*T_out, C), taps row-local (no counts: its consumer masks).
 * ddsp_nsf_post: x (B*T, C) -> out (B, T), tanh(. + b) replaced by 0 at t >= T_b.
 * (ddsp_nsf_mean needs no ragged form: the mean of masked tensors is masked.)
 * ddsp_stft_frames: the framing of `STFT.get_mel` (nvSTFT.py:88-98) for audio (B, T) with n_samples[b] <= T samples
 *   per row (DEVICE int32, NULL: T): per row pad_left = (n_fft - hop) / 2, pad_right = max((n_fft - hop + 1) / 2,
 *   n_fft - n_b - pad_left), reflect padding where pad_right < n_b and zeros otherwise - chosen PER ROW -, frames (B, L, n_fft)
 *   with L_b = (n_b + pad_left + pad_right - n_fft) / hop + 1 frames of the row and 0 in frames >= L_b.  Audio past n_b is
 *   never read.  ddsp_log_mel then runs on the B * L rows. */
int ddsp_stft_frames(ddsp_ctx* ctx, void* stream, const float* audio, int64_t B, int64_t T, const int32_t* n_samples, int n_fft,
                     int hop, int64_t L, float* out);

/* ---- a15: optimiser step --------------------------------------------------------------------- */
/* replaces one parameter's update of torch.optim.AdamW (train.py:41, solver.py:114): decoupled weight decay,
 * bias-corrected moments, `step` counted from 1.  All buffers hold n fp32 values. */
int ddsp_adamw_step(ddsp_ctx* ctx, void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                    int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step);
/* the same update for n_tensors parameters that share hyper-parameters and step (one optimizer.step() of
 * solver.py:114 over a param group), a handful of launches instead of one per tensor.  params / grads / exp_avg /
 * exp_avg_sq are HOST arrays of n_tensors device pointers, numel a host array of element counts (0 allowed).
 * grad_scale (finite): every gradient is multiplied by it as it is read - the 1 / world of a data-parallel mean applied to a
 * bucket that holds the SUM over the ranks, without a pass of its own over the gradients; grads are not written.  Exactly 1.0f
 * runs the kernel that does not multiply. */
int ddsp_adamw_step_multi(ddsp_ctx* ctx, void* stream, int n_tensors, float* const* params, const float* const* grads,
                          float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale);

/* ---- building block: fp32-in / fp32-accumulate MFMA GEMM ---------------------------------------- */
/* C[m][n] = sum_k A(m,k) B(k,n) (+ bias[n]).  a_k_contig: A(m,k) = A[m*lda+k] else A[k*lda+m];
 * b_k_contig: B(k,n) = B[n*ldb+k] (nn.Linear weight layout) else B[k*ldb+n].  Rows must start 16-byte aligned
 * (lda, ldb multiples of 4).  Exposed for unit tests of the block every contraction of the path is built on.
 * tile selects the kernel and its tiling; a code from 10 on that is not listed here is DDSP_ERR_ARG and launches nothing:
 *   0        what the network's layers run: the choice by shape and math mode (any layout)
 *   1..6     register-staged kernel (any layout): 64x64, 64x128, 128x128 on 4 waves; 128x128, 128x64, 256x128 on 8 waves
 *            (every other code below 10 runs 6)
 *   10..16   LDS-DMA kernel, fp32 products (row-major A, [N][K] B, K % 32 == 0): 10 128x64, 11 128x128, 12 256x128 with a
 *            3-stage ring; 13 128x128, 14 128x64 with 2 stages; 15 64x64, 16 64x128 on 4 waves
 *   30       LDS-DMA kernel, 128x128 with 2 stages, split-bf16 products
 *   70, 75   wave-specialised kernel (as 10.., and K >= 256, N % 64 == 0, 16-byte aligned C): 70 128x128, 75 128x64 tiles
 * variant is read by tiles 70 and 75 only, as products + epilogue (any other bit is DDSP_ERR_ARG):
 *   products  0 fp32, 3 split-bf16 (operands split in the loop), 8 split-bf16 on operands that arrive in the pre-split
 *             layout (ddsp_gemm_res_ln below); tile 75 takes 8 only
 *   epilogue  + 0 C = A B^T + bias; + 16 (tile 75) C += A B^T + bias; + 32 (tile 70, bias, N % 128 == 0) gated pair:
 *             C gets N / 2 columns */
int ddsp_gemm_f32(ddsp_ctx* ctx, void* stream, const float* A, int64_t lda, int a_k_contig, const float* B,
                  int64_t ldb, int b_k_contig, const float* bias, float* C, int64_t ldc, int M, int N, int K, int tile,
                  int variant);

/* The fused building block of the control network's residual Linear layers (pcmer.py:221-251 `to_out`, :42-63 pw2) at large
 * batches: X = res + A W^T + bias (M x 256; X may be res) and Y = LayerNorm(X) * gamma + beta (eps 1e-5) in one launch.
 * A (M x K) and W (256 x K) are in the pre-split operand layout (per 8 consecutive k: 8 bf16 hi, then 8 bf16 lo); Y is
 * written in that layout too (y_split & 1) or as fp32; y_split & 2: A is given as plain fp32 rows and split in the kernel.  Same bits as ddsp_gemm_f32 on split operands followed by the
 * LayerNorm kernel.  Exposed for tests. */
int ddsp_gemm_res_ln(ddsp_ctx* ctx, void* stream, const float* A_split, const float* W_split, const float* bias,
                     const float* res, const float* gamma, const float* beta, int M, int K, float* X, float* Y, int y_split);

/* The conformer's conv-module tail (pcmer.py:42-63: depthwise conv k31 -> SiLU -> pw2, then the residual and the next LayerNorm)
 * on split-bf16 operands, as ddsp_unit2ctrl_fwd runs it at large batches: glu (B*Fr, 512) fp32 = the pw1 + GLU output, taps
 * [31][512] and dw_bias [512] of the depthwise convolution, W_split (256, 512) pre-split, n_frames null or B frame counts
 * (input frames at or behind a row's count read as zero), causal 0 / 1.  fused = 0: the depthwise kernel writes its split
 * output to scratch (B*Fr, 512) and ddsp_gemm_res_ln's kernel reads it; fused = 1: one launch that convolves in the GEMM's
 * operand stage (scratch unused, may be null).  X and Y (split) as in ddsp_gemm_res_ln; the same bits either way.
 * Exposed for tests. */
int ddsp_u2c_dwconv_pw2(ddsp_ctx* ctx, void* stream, const float* glu, const float* taps, const float* dw_bias,
                        const float* W_split, const float* bias, const float* res, const float* gamma, const float* beta,
                        const int* n_frames, int B, int Fr, int causal, int fused, float* scratch, float* X, float* Y);

/* ---- building block: the linear attention of one PCmer layer without its Linear layers ------------------------------ */
/* replaces ddsp/pcmer.py:69-77,123-159 (`softmax_kernel` feature maps + `linear_attention`, non-causal): q, k, v
 * (B*Fr, 512) = 8 heads x 64, proj (266, 64) the layer's `projection_matrix`; out (B*Fr, 512) = the merged heads before
 * `to_out`.  math: DDSP_MATH_FP32 (fp32 matrix products) or DDSP_MATH_SPLIT_BF16 (the feature projections from six bf16
 * piece products - they enter an exponential -, the two context products from three).  Exposed for unit tests of the
 * kernels ddsp_unit2ctrl_fwd runs at inference (it picks the split kernels from 32 utterances on).
 * math = DDSP_ATTENTION_CAUSAL: `causal_linear_attention` (pcmer.py:170-188, `c: true` networks) instead - the running sums
 * over the frames up to and including each one, as chunked products with fp32 arithmetic.
 * math = DDSP_ATTENTION_PAIR: DDSP_MATH_SPLIT_BF16 with the key side and the query side as two kernels (the fused kernel's
 * independent comparison in the tests).  Any other code is DDSP_ERR_ARG. */
#define DDSP_ATTENTION_CAUSAL 200
#define DDSP_ATTENTION_PAIR 100
int ddsp_performer_attention(ddsp_ctx* ctx, void* stream, const float* q, const float* k, const float* v,
                             const float* proj, int64_t B, int64_t Fr, float* out, int math);

/* ---- the units encoder (HuBERT-Soft, encoder/hubert/model.py; ddsp/vocoder.py:140-229) ------------------- */
/* Device pointers into the HubertSoft state dict, fp32, dense, in the reference's key order (the two keys `units` does not
 * read, `masked_spec_embed` and `label_embedding.weight`, are left out):
 *   conv0_w  feature_extractor.conv0.weight (512,1,10)      norm0_w/_b  feature_extractor.norm0.{weight,bias} (512)
 *   conv_w[i] feature_extractor.conv{i+1}.weight (512,512,3) for i < 4, (512,512,2) for i = 4, 5
 *   fp_norm_w/_b, fp_proj_w/_b  feature_projection.norm (512), feature_projection.projection (768,512), (768)
 *   pos_b, pos_g, pos_v  positional_embedding.conv.{bias (768), weight_g (1,1,128), weight_v (768,48,128)}
 *   norm_w/_b  norm (768)
 *   layer[i]   encoder.layers.i.{self_attn.in_proj_weight (2304,768), self_attn.in_proj_bias, self_attn.out_proj.weight
 *              (768,768), .bias, linear1.weight (3072,768), .bias, linear2.weight (768,3072), .bias, norm1.*, norm2.*}
 *   proj_w/_b  proj (256,768), (256)
 * `version` as in ddsp_u2c_weights: 0 = prepare the weights (conv repacking, weight-norm fold: ~36 MB) on every call;
 * otherwise the context keeps its prepared copy while every pointer AND the version are what they were, so the caller
 * advances the version with every write to a weight. */
typedef struct ddsp_hubert_layer {
    const float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b, *linear1_w, *linear1_b, *linear2_w, *linear2_b;
    const float *norm1_w, *norm1_b, *norm2_w, *norm2_b;
} ddsp_hubert_layer;

typedef struct ddsp_hubert_weights {
    const float *conv0_w, *norm0_w, *norm0_b;
    const float* conv_w[6];
    const float *fp_norm_w, *fp_norm_b, *fp_proj_w, *fp_proj_b;
    const float *pos_b, *pos_g, *pos_v;
    const float *norm_w, *norm_b;
    ddsp_hubert_layer layer[12];
    const float *proj_w, *proj_b;
    uint64_t version;
} ddsp_hubert_weights;

/* Encoder frames of T samples at 16 kHz: T' = T + 80, (T' - 10) / 5 + 1, then (n - 3) / 2 + 1 four times and (n - 2) / 2 + 1
 * twice; 0 when the audio is too short for the conv stack, -1 for T < 0.  Host only. */
int64_t ddsp_hubert_frames(int64_t T);
/* replaces `HubertSoft.units(wav (B,1,T))` (encoder/hubert/model.py): wav (B,T) 16 kHz -> units (B, Fr, 256),
 * Fr = ddsp_hubert_frames(T).  The GEMMs use the context's product arithmetic (ddsp_ctx_set_math); conv0, the norms and
 * the softmax attention run in fp32.  No host synchronisation once the scratch arena (and the prepared-weight slot) exist,
 * so the call can be captured into a HIP graph.  n_samples: NULL, or a ragged batch ("the units encoder over a ragged batch"). */
int ddsp_hubert_soft_units(ddsp_ctx* ctx, void* stream, const ddsp_hubert_weights* w, const float* wav, int64_t B, int64_t T,
                           const int32_t* n_samples, float* units);
/* `Hubert.encode(wav, layer)` without the final projection, for tests and callers of intermediate features:
 * layer -1 = the conv stack's output (B, Fr, 512); 0..12 = the hidden state (B, Fr, 768) after that many transformer layers. */
int ddsp_hubert_encode(ddsp_ctx* ctx, void* stream, const ddsp_hubert_weights* w, const float* wav, int64_t B, int64_t T,
                       const int32_t* n_samples, int layer, float* out);
/* building block: softmax attention softmax(q k^T / 8) v per (utterance, head), no mask, any L (online softmax: no L x L
 * matrix).  q, k, v, out (B*L, heads*64) rows, head h at columns 64h..64h+63.  math: DDSP_MATH_FP32 or
 * DDSP_MATH_SPLIT_BF16; both run fp32 products (the attention is ~3 % of the encoder's work at a 4.5 s window).  Exposed for
 * unit tests.  n_keys: NULL, or a DEVICE array of B int32 (held inside 0..L): utterance b attends over its first n_keys[b] rows,
 * which are also the only rows of `out` that are written. */
int ddsp_softmax_attention(ddsp_ctx* ctx, void* stream, const float* q, const float* k, const float* v, int64_t B, int64_t L,
                           int heads, float* out, int math, const int32_t* n_keys);

/* ---- the units encoder over a ragged batch (ddsp_hubert_soft_units / ddsp_hubert_encode with n_samples) -------------------
 * n_samples: DEVICE array of B int32, the 16 kHz samples of each row inside the padded (B, T) wav; the caller checks
 * 1 <= n_samples[b] <= T and ddsp_hubert_frames(n_samples[b]) >= 1 (the kernels hold a count inside 0..T).  The per-row frame
 * counts are derived on the device and nothing is read back, so the call can be captured like the rectangular one.
 * Row b of the result is, over its own ddsp_hubert_frames(n_samples[b]) frames, what the rectangular call returns for
 * wav[b][:n_samples[b]] alone, and exactly 0 after them.  wav[b][i] for i >= n_samples[b] may hold anything (NaN included): it
 * is replaced by selection where it is loaded.  Every place that looks across frames stops at the row's own end: conv0's
 * zero padding, the GroupNorm statistics (partitioned and divided as for the row alone), the zero edge of the positional
 * convolution, the keys of the softmax attention.  The GEMMs run over all B * Fr padded rows.  `units` / `out` must be
 * 16-byte aligned (DDSP_ERR_ARG otherwise). */

/* ---- the units encoder in fairseq's HuBERT-base form (ContentVec, HuBERT-base: ddsp/vocoder.py:231-332) -----------------
 * fairseq's `HubertModel.extract_features(source, padding_mask = all False, output_layer = n_layers)`, optionally followed by
 * `final_proj`.  It is the network above with three differences: the audio is NOT padded, the transformer stops after
 * n_layers layers, and the attention's input projections are three (768, 768) matrices with a bias each.  The library packs
 * them into the (2304, 768) operand of its QKV GEMM when it prepares the weights (with the conv repacking and the
 * weight-norm fold), into the same per-context slot under the same rule: prepared again whenever a pointer or `version`
 * differs, on every call for version 0.  The two forms share that slot, so alternating them on one context prepares anew.
 * Device pointers into a fairseq HubertModel state dict, fp32, dense:
 *   conv0_w, conv_w[i]  feature_extractor.conv_layers.{0, i+1}.0.weight     norm0_w/_b  feature_extractor.conv_layers.0.2.*
 *   fp_norm_w/_b  layer_norm (512)      fp_proj_w/_b  post_extract_proj (768,512), (768)
 *   pos_b, pos_g, pos_v  encoder.pos_conv.0.{bias, weight_g (1,1,128), weight_v (768,48,128)}     norm_w/_b  encoder.layer_norm
 *   layer[i]  encoder.layers.i.{self_attn.q_proj, .k_proj, .v_proj, .out_proj (each weight (768,768) and bias),
 *             self_attn_layer_norm (ln1), fc1 (3072,768), fc2 (768,3072), final_layer_norm (ln2)}
 *   proj_w/_b  final_proj (256,768), (256) */
typedef struct ddsp_hubert_base_layer {
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *out_w, *out_b;
    const float *ln1_w, *ln1_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *ln2_w, *ln2_b;
} ddsp_hubert_base_layer;

typedef struct ddsp_hubert_base_weights {
    const float *conv0_w, *norm0_w, *norm0_b;
    const float* conv_w[6];
    const float *fp_norm_w, *fp_norm_b, *fp_proj_w, *fp_proj_b;
    const float *pos_b, *pos_g, *pos_v;
    const float *norm_w, *norm_b;
    ddsp_hubert_base_layer layer[12];
    const float *proj_w, *proj_b;
    uint64_t version;
} ddsp_hubert_base_weights;

/* Frames of T unpadded samples: (T - 10) / 5 + 1, then (n - 3) / 2 + 1 four times and (n - 2) / 2 + 1 twice (400 samples give
 * the first frame, 720 the second); 0 when the audio is too short for the conv stack, -1 for T < 0.  Host only. */
int64_t ddsp_hubert_base_frames(int64_t T);
/* wav (B,T) 16 kHz -> out (B, Fr, 768) for project = 0: the hidden state after n_layers (1..12) transformer layers; or
 * (B, Fr, 256) for project = 1: `final_proj` of it.  Fr = ddsp_hubert_base_frames(T).  n_samples: NULL, or a ragged batch
 * exactly as for ddsp_hubert_soft_units (counts checked against ddsp_hubert_base_frames; `out` 16-byte aligned).  Product
 * arithmetic, capture and read-backs (none) as for ddsp_hubert_soft_units. */
int ddsp_hubert_base_units(ddsp_ctx* ctx, void* stream, const ddsp_hubert_base_weights* w, const float* wav, int64_t B, int64_t T,
                           const int32_t* n_samples, int n_layers, int project, float* out);

/* ---- the f0 extractor (CREPE, ddsp/vocoder.py:39-113 with torchcrepe.predict and librosa's Viterbi restated) ---------- */
/* Device pointers into a CREPE state dict (torchcrepe's keys), fp32, dense: conv_w[i] = `conv{i+1}.weight` (Cout, Cin, k, 1),
 * conv_b[i] = `conv{i+1}.bias`, bn_*[i] = `conv{i+1}_BN.{weight,bias,running_mean,running_var}`, cls_w / cls_b =
 * `classifier.{weight,bias}` (360, 4 * width[5]).  width = output channels of conv1..conv6: {1024, 128, 128, 128, 256, 512}
 * for 'full', every one / 8 for 'tiny' (each a multiple of 16).  `version`: as ddsp_hubert_weights::version (the prepared
 * copies - repacked convolutions, batch norms folded into a scale and shift - are kept in the context while it and the
 * struct's other bytes stand; 0 = prepare on every call). */
typedef struct ddsp_crepe_weights {
    const float* conv_w[6];
    const float* conv_b[6];
    const float* bn_w[6];
    const float* bn_b[6];
    const float* bn_mean[6];
    const float* bn_var[6];
    const float *cls_w, *cls_b;
    int width[6];
    uint64_t version;
} ddsp_crepe_weights;

/* CREPE frames of T16 samples at 16 kHz with pad=True: 1 + T16 / hop; -1 for T16 < 0 or hop < 1.  Host only. */
int64_t ddsp_crepe_frames(int64_t T16, int hop);
/* torchcrepe.infer over the frames of torchcrepe.preprocess(pad=True): audio16 (B,T) 16 kHz -> probs (B, Fr, 360) sigmoid
 * activations, Fr = ddsp_crepe_frames(T, hop).  Each 1024-sample frame (zero padding of 512 on each side of the audio) is
 * normalised by its mean and unbiased standard deviation (fp64 statistics, divisor max(1e-10, std)).  The convolutions and
 * the classifier are GEMMs in the context's product arithmetic; ReLU, batch norm and the 2x1 max-pool are their epilogue.
 * No host synchronisation once the scratch arena (and the prepared-weight slot) exist.
 * n_samples, frame_prefix, n_packed: all three, or NULL, NULL and an n_packed that is not read ("the f0 extractor over a ragged
 * batch" below, like n_frames of the decode and n_crepe / n_out of the tail). */
int ddsp_crepe_activations(ddsp_ctx* ctx, void* stream, const ddsp_crepe_weights* w, const float* audio16, int64_t B, int64_t T,
                           const int32_t* n_samples, const int32_t* frame_prefix, int64_t n_packed, int hop, float* probs);
/* torchcrepe.postprocess with the Viterbi decoder: bins [:minidx] and [maxidx:] of probs (B, Fr, 360) masked (minidx =
 * floor, maxidx = ceil of (1200 log2(f / 10) - 1997.3794084376191) / 20 in fp32, Python slice rules), emissions
 * log(softmax + fp32 tiny), transitions log(max(12 - |i - j|, 0) / row sum + tiny), uniform start, fp64 values, first index
 * on ties (librosa.sequence.viterbi).  The track is decoded in independent pieces of `segment` frames (torchcrepe.predict
 * decodes each batch of `batch_size` frames on its own; 0 = the whole track).  Outputs (B, Fr): f0 = 10 * 2^(cents / 1200),
 * cents = 20 * bin + 1997.3794084376191 (+ a triangular dither on (-20, 20) cents drawn from a counter hash of
 * `dither_seed` when use_dither != 0); periodicity = the masked activation at the chosen bin; bins (int32, may be null).
 * seed_dev: NULL, or the dither seed in device memory (8-byte aligned; dither_seed is then not read): the decode uses *seed_dev
 * exactly as it uses dither_seed (bit-identical outputs for the same value), and a one-thread kernel behind it replaces the word
 * by seed * 6364136223846793005 + 1442695040888963407 (mod 2^64), use_dither or not.  Captured into a HIP graph, every replay
 * therefore dithers with a new seed (a by-value seed would be frozen at its capture-time value).  Not together with n_frames
 * (DDSP_ERR_ARG). */
int ddsp_crepe_decode(ddsp_ctx* ctx, void* stream, const float* probs, int64_t B, int64_t Fr, const int32_t* n_frames, float fmin,
                      float fmax, int64_t segment, uint64_t dither_seed, uint64_t* seed_dev, int use_dither, float* f0,
                      float* periodicity, int32_t* bins);
/* The crepe tail of F0_Extractor.extract (ddsp/vocoder.py:96-113): f0, pd (B, Fr) -> out (B, n_frames): MedianPool1d(pd, 4),
 * f0 = NaN where that is < threshold, MaskedAvgPool1d(f0, 4) (reflect padding (1, 2), Fr >= 3), the re-timing
 * out[start_frame + n] = f0[min(rint(n * hop / sr / 0.005), Fr - 1)] for n < n_frames - start_frame (fp64 index arithmetic,
 * hop may be fractional), zeros before start_frame, then with uv_interp != 0 numpy.interp over the zero frames (fp64, when
 * any frame is non-zero) and out = max(out, f0_min). */
int ddsp_f0_postfilter(ddsp_ctx* ctx, void* stream, const float* f0, const float* pd, int64_t B, int64_t Fr, const int32_t* n_crepe,
                       int sr, double hop, int64_t n_frames, int64_t start_frame, const int32_t* n_out, float threshold,
                       int uv_interp, float f0_min, float* out);

/* ---- the f0 extractor over a ragged batch --------------------------------------------------------------------------------
 * Every count is a DEVICE array of B int32 that the caller has checked and that is never read back; a kernel holds a value
 * outside its range at the nearest bound.  Row b of each result is what the rectangular call returns for the row alone at
 * its own length, and exactly 0 after it; what the inputs hold past a row's end (NaN included) is never read into arithmetic.
 * ddsp_crepe_activations: audio16 (B, T) with n_samples[b] <= T samples per row -> probs (B, Fr, 360), Fr =
 *   ddsp_crepe_frames(T, hop), row b with Fr_b = ddsp_crepe_frames(n_samples[b], hop) frames.  A frame depends on its own
 *   1024 samples only, so the network runs over the PACKED list of the rows' real frames: frame_prefix is the DEVICE array
 *   of B + 1 int32 exclusive prefix sums of Fr_b (frame_prefix[0] = 0) and n_packed = frame_prefix[B] its total, which the
 *   host knows.  A frame reads samples < 0 or >= n_samples[b] of its row as 0 by a bounds test.
 * ddsp_crepe_decode: probs (B, Fr, 360) with n_frames[b] <= Fr frames per row.  The pieces of `segment` frames are cut
 *   per row, the last one ends at the row's own last frame, and the dither is drawn for the row-local frame: row b equals
 *   ddsp_crepe_decode of probs[b][:n_frames[b]] alone with the same seed, bit for bit.
 * ddsp_f0_postfilter: f0, pd (B, Fr) with n_crepe[b] in 3..Fr frames per row -> out (B, n_frames) with n_out[b] <=
 *   n_frames frames per row (both counts or neither; with them start_frame must be 0, DDSP_ERR_ARG otherwise): the reflect windows and the re-timing clamp use n_crepe[b], and the
 *   uv_interp fill looks at the row's own n_out[b] frames only. */
/* ---- the autocorrelation f0 extractor (Boersma 1993; the algorithm behind the reference's 'parselmouth' branch,
 * ddsp/vocoder.py:55-69,107-113, restated from the paper's formulae: Praat itself is not a dependency and agreement with it
 * is not pinned) -----------------------------------------------------------------------------------------------------------
 * Hanning window of 3 / f0_min seconds, autocorrelation by an FFT of nfft >= 1.5 window lengths divided by the window's own,
 * candidates r > 0.3 refined by Hann-windowed sinc interpolation (depth 30, then Brent on depth 70; fp64), at most
 * max(15, floor(f0_max / f0_min)) <= 32 per frame with the unvoiced one, and a Viterbi path with voicing threshold 0.6, silence
 * threshold 0.03, octave cost 0.01, octave-jump cost 0.35 and voiced/unvoiced cost 0.14.  The signal path up to the normalised
 * autocorrelation is fp32.  Deterministic: there is no dither.
 * ddsp_f0_ac_frames: analysis frames of T samples, floor((T / sr - 3 / f0_min) / (hop / sr)) + 1 in fp64, 0 when the audio is
 *   shorter than one window (-1: bad arguments).  A host computation.
 * ddsp_f0_ac: audio (B, T) at `sr` -> out (B, n_frames): `start_frame + (floor(T / hop) - nF + 1) / 2` zeros, the nF =
 *   ddsp_f0_ac_frames(T, ...) frames (0 where unvoiced), zeros after; with uv_interp != 0 numpy.interp over the zero frames
 *   (fp64, when any frame is non-zero) and out = max(out, f0_min).  `choice` (B, nF) int32, may be null: the chosen candidate
 *   of every analysis frame (0 = unvoiced).  T must hold one window; the FFT is at most 8192 points (DDSP_ERR_ARG otherwise).
 *   n_samples: NULL, or n_samples[b] <= T samples per row (a DEVICE array, as in the section above; start_frame must then be
 *   0): row b is the row analysed alone at its own length, bit for bit, with floor(n_samples[b] / hop) + 1 frames and exactly 0
 *   after them; `choice` is (B, ddsp_f0_ac_frames(T, ...)).  The caller has checked that every row holds one window. */
int64_t ddsp_f0_ac_frames(int64_t T, int sr, double hop, double f0_min);
int ddsp_f0_ac(ddsp_ctx* ctx, void* stream, const float* audio, int64_t B, int64_t T, const int32_t* n_samples, int sr, double hop,
               double f0_min, double f0_max, int64_t n_frames, int64_t start_frame, int uv_interp, float* out, int32_t* choice);

/* ---- the silence slicer (reference: slicer.py `Slicer.slice`, the stage in front of main.py's per-slice loop) -------------
 * Two kernels.  Frame RMS as librosa.feature.rms documents it: frame i of a row of n samples covers the samples
 * [i * hop - win / 2, i * hop - win / 2 + win) (integer division), a sample outside [0, n) reads 0 (pad_mode
 * DDSP_SLICER_PAD_CONSTANT, librosa >= 0.10) or the sample numpy's 'reflect' rule names (DDSP_SLICER_PAD_REFLECT, older
 * librosa) - selected by a bounds test, never materialised - and the value is sqrt(sum(x^2) / win) with fp32 products summed
 * in fp64.  Then one wave per row walks the row's values and reproduces the reference's tagging state machine and chunk
 * assembly (slicer.py:32-111) exactly: `threshold` is the linear level a frame must stay below to be silent, `min_length`,
 * `min_interval` and `max_sil_kept` are in FRAMES as the reference's constructor rounds them; a row with n <= min_length (a
 * sample count against a frame count, as the reference compares) is one un-sliced chunk; every argmin returns the lowest index
 * among equal minima.
 * ddsp_slicer_frames: 1 + (n + 2 * (win / 2) - win) / hop, the frames of n samples (-1: bad arguments).  A host computation.
 * ddsp_slicer: audio (B, T) -> rms (B, F), F = ddsp_slicer_frames(T, win, hop); table (B, capacity, 3) int32 rows
 *   (start_sample, end_sample, is_silence) in the reference's order, zero-length silence chunks included, and count (B) int32;
 *   the table's rows from count[b] on are zeros.
 *   Capacity: a tag needs a silent run of its own of at least min_interval frames, or the leading rule, which fires once; K
 *   tags give at most 2 K + 1 chunks (a voiced chunk in front of each tag and one behind the last).  So capacity =
 *   2 * (F / min_interval + 1) + 1 rows always suffice.  A row that would exceed a smaller capacity writes the chunks that fit,
 *   count[b] = capacity, and sets the context's device error word (DDSP_ERR_ARG from ddsp_ctx_poll_error or the next call that
 *   takes it).
 *   n_samples: NULL, or n_samples[b] in 1..T samples per row (a DEVICE array): row b is the row cut alone at its own length,
 *   bit for bit; samples from n_samples[b] on are never read and rms[b][i] = 0 from the row's own frame count on.
 * T + 4 * hop + win < 2^31, 1 <= win, 1 <= hop, 1 <= min_interval.  The call does not synchronise, allocate or read back. */
#define DDSP_SLICER_PAD_CONSTANT 0
#define DDSP_SLICER_PAD_REFLECT 1
int64_t ddsp_slicer_frames(int64_t n, int64_t win, int64_t hop);
int ddsp_slicer(ddsp_ctx* ctx, void* stream, const float* audio, int64_t B, int64_t T, const int32_t* n_samples, int64_t win,
                int64_t hop, double threshold, int64_t min_length, int64_t min_interval, int64_t max_sil_kept, int pad_mode,
                float* rms, int32_t* table, int32_t* count, int64_t capacity);

/* ---- measurement: per-kernel-family HIP-event timing on the launch stream --------------------- */
/* ddsp_profile_begin arms the families in `family_mask` (bit i = family i, see the name returned); while armed,
 * each kernel launch of such a family is bracketed by hipEventRecord on the caller's stream.  ddsp_profile_end
 * disarms, waits for the events and returns one aggregated entry per family that launched: launches, summed
 * duration, and the ALGORITHMIC flops / HBM bytes the library attributes to those launches. */
typedef struct ddsp_prof_entry {
    int family;
    char name[36];
    int64_t launches;
    double ms_total;
    double flops_total;
    double bytes_total;
} ddsp_prof_entry;
int ddsp_profile_begin(ddsp_ctx* ctx, uint64_t family_mask);
/* While armed: change the bracketed families (0 = pause) without dropping the records taken so far - for callers that bracket a
 * SAMPLE of their steps (bench.py: every fifth step of the timed region), since an event record costs ~2 us of stream time. */
int ddsp_profile_mask(ddsp_ctx* ctx, uint64_t family_mask);
int ddsp_profile_end(ddsp_ctx* ctx, ddsp_prof_entry* out, int max_entries, int* n_entries);

#ifdef __cplusplus
}
#endif
#endif /* DDSP_AMD_H */
