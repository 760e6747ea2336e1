// What the frame-varying FIR kernels of ltv_fir.hip (hop 512) and ltv_fir_hop.hip (hop 128, 256) share: the noise
// draw, the Toeplitz-block product loop on the fp32 matrix pipe, and the entry points of the second file.
#pragma once
#include "common.h"

// hop 128 / 256 (ltv_fir_hop.hip); arguments as ddsp_ltv_fir / ddsp_ltv_fir_bwd, already checked by them
int ddsp_ltv_fir_hop(ddsp_ctx* ctx, hipStream_t st, const float* audio, int excitation, uint64_t noise_seed,
                     const float* ir, int64_t B, int64_t Fr, int hop, int n, const float* add_in, float* out,
                     float* out_sum);
int ddsp_ltv_fir_hop_bwd(ddsp_ctx* ctx, hipStream_t st, const float* audio, int excitation, uint64_t noise_seed,
                         const float* ir, const float* d_out, int64_t B, int64_t Fr, int hop, int n, float* d_audio,
                         float* d_ir);

#ifdef __HIPCC__
namespace {

__device__ __forceinline__ float noise_u(uint64_t seed, uint64_t idx) {
    // A stateless hash of the sample counter (every block that needs sample idx regenerates it).  Round 3: two rounds of a 32-bit
    // integer finaliser (multiply / xor-shift, constants of the "lowbias32" family) instead of the splitmix64 finaliser - its three
    // 64 x 64-bit multiplies were ~45 vector instructions per sample in the FIR kernel's staging waves, which regenerate every
    // sample twice (50 % overlapped frames); this is ~16 (`ddsp_hash32`, common.h).
    const float u = (float)(ddsp_hash32(seed, idx) >> 8) * (1.0f / 16777216.0f);   // 24-bit U[0,1) like torch.rand fp32
    return u * 2.0f - 1.0f;                                   // exact in fp32
}

// acc[s] += sum_{q=qa..qb} A_q * B_q for the four k-steps s of a 16x16x16 Toeplitz-block product:
//   a = ap[16q + SA*4s], b = bp[s*bstep + SB*q]   (lane-constant parts already folded into ap / bp).
// Software-pipelined with two register sets: operands of shift q+1 are fetched from LDS before the MFMAs of
// shift q issue (sched_group_barrier pins [8 LDS reads][4 MFMAs]; hipcc otherwise sinks the reads).
// qa, qb MUST be wave-uniform (SGPR) values - see the readfirstlane note in the kernels.
template <int SA, int SB>
__device__ __forceinline__ void toeplitz_accumulate(const float* __restrict__ ap, const float* __restrict__ bp,
                                                    int bstep, int qa, int qb, f32x4 (&acc)[4]) {
    if (qa > qb) return;
    float a0[4], b0[4], a1[4], b1[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        a0[s] = ap[16 * qa + SA * 4 * s];
        b0[s] = bp[s * bstep + SB * qa];
    }
    int q = qa;
    for (; q + 1 <= qb; q += 2) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            a1[s] = ap[16 * (q + 1) + SA * 4 * s];
            b1[s] = bp[s * bstep + SB * (q + 1)];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], b0[s], acc[s], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        const int q2 = (q + 2 <= qb) ? q + 2 : qb;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            a0[s] = ap[16 * q2 + SA * 4 * s];
            b0[s] = bp[s * bstep + SB * q2];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[s], b1[s], acc[s], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    if (q == qb) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[s], b0[s], acc[s], 0, 0, 0);
    }
}

}  // namespace
#endif
