// The order of unit retrieval and of the k-means assignment: (t, id) ascending, equal scores to the smaller id.  False when t
// is NaN: such a score is never selected.
#pragma once

__device__ __forceinline__ bool before(float t, int i, float t2, int i2) { return t < t2 || (t == t2 && i < i2); }
