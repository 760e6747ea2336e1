"""Unit index reduction: the rule of `ddsp_units_kmeans_assign` / `ddsp_units_kmeans_update` (include/ddsp_amd.h) stated in numpy
fp64 and Python integers - the kernels' only yardstick - and the generators of its tests.  No GPU, no torch."""
import math

import numpy as np

from retrieval_cases import same_bits, score_bound, scores  # noqa: F401  (the score and its error bound are the retrieval's)


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def init(vec, K):
    """cen[j] = vec[floor(j * N / K)], bit for bit: the `max_entries` subset."""
    N = vec.shape[0]
    return np.ascontiguousarray(vec[[(j * N) // K for j in range(K)]], dtype=np.float32)


def assign(vec, cen):
    """a_i = the j with the smallest (t_ij, j), t_ij = |cen[j]|^2 - 2 <x_i, cen[j]> in fp64 -> (N,) int32."""
    t = scores(vec, cen)                                               # (N, K): the entries are the queries, the centres the index
    ids = np.arange(cen.shape[0])
    return np.array([np.lexsort((ids, row))[0] for row in t], dtype=np.int32)


def fixed_shift(vec):
    """S = 62 - E - L: max|vec| < 2^E (the frexp exponent; E = 0 for an all-zero index), L = (N - 1).bit_length()."""
    top = float(np.abs(vec).max())
    E = math.frexp(top)[1] if top > 0 else 0
    return 62 - E - (vec.shape[0] - 1).bit_length()


def fixed(x, S):
    """q = (int64) rint(ldexp((double) x, S)) as a Python int."""
    return int(np.rint(math.ldexp(float(x), S)))


def update(vec, a, cen, S):
    """The centres after one update with Python integers -> (cen' (K, C) fp32, count (K,) int32).  An assignment outside [0, K)
    belongs to no centre; a centre without entries keeps its bits."""
    K, C = cen.shape
    q = np.rint(np.ldexp(vec.astype(np.float64), S))                   # exact: |q| <= 2^62 / N, integers in fp64 or rounded to them
    out = cen.copy()
    count = np.zeros(K, dtype=np.int32)
    for j in range(K):
        rows = np.nonzero(a == j)[0]
        count[j] = len(rows)
        if len(rows):
            for c in range(C):
                total = sum(int(v) for v in q[rows, c])
                out[j, c] = np.float32(math.ldexp(float(total) / float(len(rows)), -S))    # float(int): nearest even
    return out, count


def reduce(vec, K, iters, on_iteration=None):
    """The reduction -> (centres kept, {"moved", "count", "dropped", "shift"}, cen (K, C) of the last iteration).
    on_iteration(cen, a) sees every iteration's centres before the assignment and the assignment."""
    vec = np.ascontiguousarray(vec, dtype=np.float32)
    N = vec.shape[0]
    S = fixed_shift(vec)
    cen = init(vec, K)
    a = np.full(N, -1, dtype=np.int32)
    moved, count = [], np.ones(K, dtype=np.int32)
    for _ in range(iters):
        new = assign(vec, cen)
        if on_iteration is not None:
            on_iteration(cen, new)
        moved.append(int((new != a).sum()))
        a = new
        cen, count = update(vec, a, cen, S)
    keep = count > 0 if iters else np.ones(K, dtype=bool)
    return cen[keep], {"moved": moved, "count": count, "dropped": int((~keep).sum()), "shift": S}, cen


def naive_update(vec, a, cen, S):
    """One update with loops only, for the host check of the statement."""
    K, C = cen.shape
    out = [[cen[j, c] for c in range(C)] for j in range(K)]
    count = [0] * K
    for j in range(K):
        total = [0] * C
        for i in range(vec.shape[0]):
            if int(a[i]) == j:
                count[j] += 1
                for c in range(C):
                    total[c] += fixed(vec[i, c], S)
        if count[j]:
            for c in range(C):
                out[j][c] = np.float32(math.ldexp(float(total[c]) / float(count[j]), -S))
    return np.array(out, dtype=np.float32), np.array(count, dtype=np.int32)


def naive_assign(vec, cen):
    out = []
    for x in vec:
        t = []
        for j, y in enumerate(cen):
            nrm = sum(float(v) ** 2 for v in y)
            t.append((nrm - 2.0 * sum(float(p) * float(v) for p, v in zip(x, y)), j))
        out.append(min(t)[1])
    return np.array(out, dtype=np.int32)


# ---- generators ---------------------------------------------------------------------------------------------------------------
# (N, K, C).  The issue's: one entry; odd sizes below a tile; several entry tiles and two centre stages with partial last ones;
# wide; the widest.  Then the edges of the kernel's tiles - 128 entries a workgroup (64 a wave), 128 centres a stage (64 a wave),
# 32 channels a slice: one less and one more than each.
ASSIGN_SHAPES = [(1, 1, 4), (7, 3, 36), (333, 130, 36), (4099, 257, 256), (600, 300, 768),
                 (127, 127, 28), (129, 129, 36), (128, 128, 32), (257, 63, 64), (255, 65, 60), (130, 1, 4)]
UPDATE_SHAPES = ASSIGN_SHAPES[:5] + [(129, 129, 36), (130, 1, 4)]


def integer_case(N, K, C, seed=0):
    """Entries and centres in {-2..2} as fp32: every product and sum of a score is exact in fp32, so ties are real ties and the
    ids are decided by the rule alone -> (vec (N, C), cen (K, C))."""
    rng = np.random.default_rng(seed)
    return rng.integers(-2, 3, (N, C)).astype(np.float32), rng.integers(-2, 3, (K, C)).astype(np.float32)


def twice_case(C=36, seed=5):
    """K = N = 64 with every row present twice (row i and row i + 32): as entries AND as centres, so every entry ties between
    two centres and the smaller id takes it."""
    half = np.random.default_rng(seed).integers(-2, 3, (32, C)).astype(np.float32)
    both = np.concatenate([half, half])
    return both, both.copy()


SEPARATED_NOISE = 0.02


def separated_case():
    """The issue's real data: 40 well-separated normal centres at C = 256 and 1500 entries, each a centre plus small noise, in
    runs as neighbouring frames come: entries floor(j * 1500 / 40) .. floor((j + 1) * 1500 / 40) - 1 lie near centre j, so the
    strided initial centres of a K = 40 reduction are one member of every cluster and no two centres ever share a cluster (two that
    did would lie a noise apart, and no gap condition could hold) -> (vec (1500, 256), centres (40, 256)).
    |centre_a - centre_b|^2 is about 2 C = 512 and the noise moves a score by some 2 * 0.02 * sqrt(2 C) = 1, while
    2 x `score_bound` is about 0.03: the gap condition is asserted on every entry by `gap_condition`, by the tests."""
    rng = np.random.default_rng(11)
    centres = rng.standard_normal((40, 256)).astype(np.float32)
    which = np.searchsorted((np.arange(40) * 1500) // 40, np.arange(1500), side="right") - 1
    vec = (centres[which] + SEPARATED_NOISE * rng.standard_normal((1500, 256))).astype(np.float32)
    return vec, centres


def gap_condition(vec, cen):
    """Asserts that for EVERY entry the gap between the best and the second-best fp64 score exceeds 2 x `score_bound`
    -> (smallest gap, bound).  One centre: nothing to confuse."""
    bound = score_bound(vec, cen)
    if cen.shape[0] == 1:
        return math.inf, bound
    t = np.sort(scores(vec, cen), axis=1)
    gap = t[:, 1] - t[:, 0]
    assert (gap > 2 * bound).all(), (float(gap.min()), bound)
    return float(gap.min()), bound
