// Plain GEMM entry point of the fp32-MFMA kernel: unit tests of the building block and tile/schedule A/B timing.
#include "gemm_ws.h"
#include "gemm_ln.h"

extern "C" int ddsp_gemm_f32(ddsp_ctx* ctx, void* stream, const float* A, int64_t lda, int a_k_contig, const float* B,
                             int64_t ldb, int b_k_contig, const float* bias, float* C, int64_t ldc, int M, int N, int K,
                             int tile, int variant) {
    DDSP_REQUIRE(ctx, ctx && A && B && C, "ddsp_gemm_f32: null argument");
    DDSP_REQUIRE(ctx, M >= 1 && N >= 1 && K >= 1 && lda >= 1 && ldb >= 1 && ldc >= N, "ddsp_gemm_f32: bad shape");
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    gemm::Args g = gemm::make(A, lda, B, ldb, M, N, K);
    gemm::EpiStore e{C, ldc, bias, 1, 0, 0};
    ddsp_prof_begin(ctx, st, PF_OTHER);
#define GO(BM, BN, AK, BK_, NW) gemm::launch_tile<BM, BN, AK, BK_, gemm::A_PLAIN, gemm::EpiStore, NW>(st, g, 1, e)
#define TILE(AK, BK_)                                                        \
    if (tile == 0) gemm::launch<AK, BK_, gemm::A_PLAIN>(st, g, 1, e);        \
    else if (tile == 1) GO(64, 64, AK, BK_, 4);                              \
    else if (tile == 2) GO(64, 128, AK, BK_, 4);                             \
    else if (tile == 3) GO(128, 128, AK, BK_, 4);                            \
    else if (tile == 4) GO(128, 128, AK, BK_, 8);                            \
    else if (tile == 5) GO(128, 64, AK, BK_, 8);                             \
    else GO(256, 128, AK, BK_, 8);
    if (tile >= 70) {
        // wave-specialised kernel (gemm_ws.h).  variant: 0 fp32 products, 3 split-bf16 (split in the loop), 8 both operands
        // arrive in the pre-split layout; + 16: residual epilogue (C += ..., tile 75), + 32: gated pair epilogue (C gets
        // N / 2 columns, tile 70)
        DDSP_REQUIRE(ctx, (variant & ~63) == 0, "ddsp_gemm_f32: unknown ws variant");
        DDSP_REQUIRE(ctx, a_k_contig && b_k_contig && gemm::ws_ok(g, 5, (variant & 48) == 16), "ddsp_gemm_f32: ws tiles need row-major A, [N][K] B, K % 32 == 0, K >= 256, aligned rows");
        const int math = variant & 15, kind = variant & 48;
        DDSP_REQUIRE(ctx, (math == 0 || math == 3 || math == 8) && ((uintptr_t)C % 16) == 0 && ldc % 4 == 0 && N % 64 == 0, "ddsp_gemm_f32: ws variant");
        hipError_t he = hipSuccess;
#define WS(BM, BN, NS, MATH)                                                                                                   \
        do {                                                                                                                   \
            if (kind == 16) { DDSP_REQUIRE(ctx, false, "ws residual: tile 75"); }                                              \
            else if (kind == 32) { gemm::WsGlu e2{C, ldc, bias}; DDSP_REQUIRE(ctx, bias && N % BN == 0 && BN == 128, "ws gated pair needs a bias and whole 128-column tiles"); \
                if constexpr (BN == 128) he = gemm::launch_ws_one<BM, BN, gemm::WsGlu, NS, MATH, true>(st, g, e2); }           \
            else { gemm::WsStore e2{C, ldc, bias};                                                                             \
                he = (N % BN == 0) ? gemm::launch_ws_one<BM, BN, gemm::WsStore, NS, MATH, true>(st, g, e2)                     \
                                   : gemm::launch_ws_one<BM, BN, gemm::WsStore, NS, MATH, false>(st, g, e2); }                 \
        } while (0)
#define WSM(BM, BN, NS)                                                     \
        do {                                                                \
            if (math == 0) WS(BM, BN, NS, 0);                               \
            else if (math == 3) WS(BM, BN, NS, 3);                          \
            else WS(BM, BN, NS, 8);                                         \
        } while (0)
        g.xcd = 1;
        if (tile == 70) WSM(128, 128, 4);
        else if (tile == 75) { DDSP_REQUIRE(ctx, math == 8 && kind != 32, "tile 75: pre-split operands, plain or residual store");
            if (kind == 16) { gemm::WsResidual e2{C, C, ldc, bias}; he = gemm::launch_ws_one<128, 64, gemm::WsResidual, 5, 8, true>(st, g, e2); }
            else { gemm::WsStore e0{C, ldc, bias}; he = gemm::launch_ws_one<128, 64, gemm::WsStore, 5, 8, true>(st, g, e0); } }
        else return ddsp_fail(ctx, DDSP_ERR_ARG, "ddsp_gemm_f32", "unknown ws tile");
#undef WSM
#undef WS
        DDSP_HIP(ctx, he);
    } else if (tile >= 10) {
        DDSP_REQUIRE(ctx, a_k_contig && b_k_contig && gemm::dma_ok(g), "ddsp_gemm_f32: DMA tiles need row-major A, [N][K] B, K % 32 == 0, aligned rows");
        if (tile == 10) gemm::launch_dma<128, 64>(st, g, 1, e);
        else if (tile == 11) gemm::launch_dma<128, 128>(st, g, 1, e);
        else if (tile == 12) gemm::launch_dma<256, 128>(st, g, 1, e);
        else if (tile == 13) gemm::launch_dma<128, 128, gemm::EpiStore, 2>(st, g, 1, e);
        else if (tile == 14) gemm::launch_dma<128, 64, gemm::EpiStore, 2>(st, g, 1, e);
        else if (tile == 15) gemm::launch_dma<64, 64, gemm::EpiStore, 3, 4>(st, g, 1, e);    // 4 waves, 64x64
        else if (tile == 16) gemm::launch_dma<64, 128, gemm::EpiStore, 3, 4>(st, g, 1, e);   // 4 waves, 64x128
        else if (tile == 30) gemm::launch_dma<128, 128, gemm::EpiStore, 2, 8, gemm::A_PLAIN, 3>(st, g, 1, e);   // split-bf16 x3
        else return ddsp_fail(ctx, DDSP_ERR_ARG, "ddsp_gemm_f32", "unknown tile");
    } else if (a_k_contig && b_k_contig) {
        TILE(true, true)
    } else if (a_k_contig && !b_k_contig) {
        TILE(true, false)
    } else if (!a_k_contig && !b_k_contig) {
        TILE(false, false)
    } else {
        TILE(false, true)
    }
    ddsp_prof_end(ctx, st, 2.0 * M * N * (double)K, 4.0 * ((double)M * K + (double)N * K + (double)M * N));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}

// x = res + A W^T + bias (M x 256) and y = LayerNorm(x) * gamma + beta in one launch (gemm_ln.h); A (M x K) and W (256 x K) in
// the pre-split operand layout.  The building block ddsp_unit2ctrl_fwd runs for its out-projection / pw2 layers at large batches.
extern "C" int ddsp_gemm_res_ln(ddsp_ctx* ctx, void* stream, const float* A_split, const float* W_split, const float* bias,
                                const float* res, const float* gamma, const float* beta, int M, int K, float* X, float* Y,
                                int y_split) {
    DDSP_REQUIRE(ctx, ctx && A_split && W_split && bias && res && gamma && beta && X && Y, "ddsp_gemm_res_ln: null argument");
    gemm::LnArgs a{A_split, W_split, K, K, M, K, bias, res, X, gamma, beta, Y, (y_split & 1) ? 1 : 0};   // y_split bit 1 (value 2): A is fp32 rows
    DDSP_REQUIRE(ctx, M >= 1 && K >= 64 && gemm::res_ln_ok(a), "ddsp_gemm_res_ln: K % 32 == 0, K >= 64, 16-byte aligned operands");
    hipStream_t st = (hipStream_t)stream;
    DDSP_ENTER_DEVICE(ctx);
    ddsp_prof_begin(ctx, st, PF_OTHER);
    DDSP_HIP(ctx, gemm::launch_res_ln(st, a, (y_split & 2) == 0));
    ddsp_prof_end(ctx, st, 2.0 * M * 256.0 * K, 4.0 * M * (K + 4.0 * 256));
    DDSP_LAUNCH_CHECK(ctx);
    return DDSP_OK;
}
