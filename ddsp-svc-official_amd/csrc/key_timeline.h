// The key timeline rule, stated once for the kernels that apply it (ddsp_pieces_gather_keys: time in file frames;
// ddsp_bank_key_glide: time in device samples).  A timeline is n >= 1 breakpoints with times bt strictly increasing; every
// breakpoint carries its key in semitones (semi, fp32) and the f0 factor the HOST formed for it (fac = 2 ** (key / 12) as a
// Python float stored to fp32: the very number a constant key multiplies with).  The key at tau is linear IN SEMITONES between
// two breakpoints, the first one's before them and the last one's after them.  The STORED factor is returned where no slope is
// at work - tau before the first breakpoint, behind the last, exactly on one, or between two of equal semitones - so a constant
// key, given as a timeline, multiplies with the bits it always had.  Only on a real slope is the factor computed here:
// exp2((s0 + (s1 - s0) * ((tau - t0) / (t1 - t0))) / 12.0) in fp64, every step one rounded operation, rounded to fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace keytl {

// T: the type of the breakpoint times (int32 file frames, int64 device samples).  bt, semi and fac are indexed in [0, n) only;
// the caller has checked n >= 1.
template <typename T>
__device__ __forceinline__ float factor_at(const T* __restrict__ bt, const float* __restrict__ semi, const float* __restrict__ fac,
                                           int n, double tau) {
    // the first breakpoint behind tau: [p, q) shrinks to it
    int p = 0, q = n;
    while (p < q) {
        const int mid = (p + q) >> 1;
        if ((double)bt[mid] > tau) q = mid;
        else p = mid + 1;
    }
    if (p == 0) return fac[0];
    if (p == n) return fac[n - 1];
    const double t0 = (double)bt[p - 1], t1 = (double)bt[p];
    const double s0 = (double)semi[p - 1], s1 = (double)semi[p];
    if (tau == t0 || s0 == s1 || !(t1 > t0)) return fac[p - 1];
    return (float)exp2((s0 + (s1 - s0) * ((tau - t0) / (t1 - t0))) / 12.0);
}

}  // namespace keytl
