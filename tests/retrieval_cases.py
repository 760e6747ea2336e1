"""Unit retrieval: the rule of `ddsp_units_retrieve` (include/ddsp_amd.h) stated in numpy fp64 - the kernels' only yardstick -
and the generators of its tests.  No GPU, no torch."""
import numpy as np

FLOOR = 1e-12
ERR_RETRIEVE = 8


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def scores(x, vec):
    """t_i = nrm[i] - 2 <x, vec[i]> in fp64 for the queries x (Q, C) against vec (N, C)."""
    vec = vec.astype(np.float64)
    return (vec * vec).sum(1)[None, :] - 2.0 * (x.astype(np.float64) @ vec.T)


def select(t, k):
    """The min(k, N) entries with the smallest (t, id) of every row of t (Q, N), ordered by (t, id) -> (Q, min(k, N)) ids."""
    ids = np.arange(t.shape[1])
    return np.stack([np.lexsort((ids, row))[:min(k, t.shape[1])] for row in t])


def blend(x, vec, ids, r):
    """One frame: s_j, the inverse-square weights with their floor, the mean and the blend, in fp64 -> (out, s)."""
    x, v = x.astype(np.float64), vec[ids].astype(np.float64)
    s = ((x[None, :] - v) ** 2).sum(1)
    w = 1.0 / np.maximum(s, FLOOR) ** 2
    w = w / w.sum()
    y = (w[:, None] * v).sum(0)
    return x + float(r) * (y - x), s


def retrieve_rows(units, indices, index_of_row, ratio_of_row, k, n_frames=None):
    """The statement.  units (rows, Fr, C) fp32; indices: a list of (N_x, C) fp32 arrays (the bank); index_of_row, ratio_of_row
    per row; n_frames per row or None -> (out (rows, Fr, C) fp32, nn_id (rows, Fr, k) int32, -1 unused, nn_dist (rows, Fr, k)
    fp64, 0 unused, err: True when a row that names an index has a ratio that is not finite or outside [0, 1]).
    Rows with no index (an id outside [0, X)), rows with ratio 0 and frames at or past the count keep their bits."""
    units = np.ascontiguousarray(units, dtype=np.float32)
    rows, Fr, C = units.shape
    out = units.copy()
    nn_id = np.full((rows, Fr, k), -1, dtype=np.int32)
    nn_dist = np.zeros((rows, Fr, k), dtype=np.float64)
    err = False
    for b in range(rows):
        xi = int(index_of_row[b])
        if not 0 <= xi < len(indices):
            continue
        r = np.float32(ratio_of_row[b])
        if not (np.isfinite(r) and 0 <= r <= 1):
            err = True
            continue
        if r == 0:
            continue
        n = Fr if n_frames is None else min(max(int(n_frames[b]), 1), Fr)
        vec = np.asarray(indices[xi], dtype=np.float32)
        ids = select(scores(units[b, :n], vec), k)
        for f in range(n):
            y, s = blend(units[b, f], vec, ids[f], r)
            out[b, f] = y.astype(np.float32)
            nn_id[b, f, :ids.shape[1]] = ids[f]
            nn_dist[b, f, :ids.shape[1]] = s
    return out, nn_id, nn_dist, err


def naive_frame(x, vec, k, r):
    """The same frame with loops only, for the host check of the statement -> (out, ids, s)."""
    N, C = vec.shape
    t = []
    for i in range(N):
        nrm = sum(float(vec[i, c]) ** 2 for c in range(C))
        dot = sum(float(x[c]) * float(vec[i, c]) for c in range(C))
        t.append((nrm - 2.0 * dot, i))
    chosen = [i for _, i in sorted(t)[:min(k, N)]]
    s = [sum((float(x[c]) - float(vec[j, c])) ** 2 for c in range(C)) for j in chosen]
    w = [1.0 / max(v, FLOOR) ** 2 for v in s]
    total = sum(w)
    out = [float(x[c]) + float(r) * (sum(w[a] / total * float(vec[j, c]) for a, j in enumerate(chosen)) - float(x[c]))
           for c in range(C)]
    return np.array(out), chosen, np.array(s)


# ---- generators ---------------------------------------------------------------------------------------------------------------
# (N, C, k, rows, Fr): one entry; k > N; odd sizes below one stage; several chunks with a partial last one; wide and k = 16
EXACT_SHAPES = [(1, 4, 8, 1, 1), (7, 36, 8, 2, 5), (333, 36, 3, 3, 37), (4099, 256, 8, 2, 70), (1500, 768, 16, 1, 33)]


def integer_case(N, C, rows, Fr, seed=0):
    """Entries in {-2..2}, queries in {-3..3}, as fp32: every product and sum of a score is exact in fp32 (and in split bf16),
    so ties are real ties and the ids are decided by the rule alone."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-2, 3, (N, C)).astype(np.float32), rng.integers(-3, 4, (rows, Fr, C)).astype(np.float32))


def copies_case(C=36, seed=3):
    """Three copies of each of five distinct vectors (entry 5 * c + v is copy c of vector v) and five queries, query q nearest to
    vector q: with k = 4 the ids are the three copies of the nearest, ascending, and the lowest-id copy of the next."""
    rng = np.random.default_rng(seed)
    base = (4 * np.arange(5)[:, None] + rng.integers(0, 2, (5, C))).astype(np.float32)     # vector v lies around 4 v
    q = base + np.where(np.arange(C)[None, :] == 0, 1.0, 0.0).astype(np.float32)           # one step off vector q, toward q + 1
    return np.tile(base, (3, 1)), q[None]


def real_case():
    """The issue's generator: 1000 x 256 normal entries, 74 queries near entries -> (idx, q (2, 37, 256))."""
    rng = np.random.default_rng(2)
    idx = rng.standard_normal((1000, 256)).astype(np.float32)
    j = rng.integers(0, 1000, 74)
    q = (0.7 * idx[j] + 0.5 * rng.standard_normal((74, 256))).astype(np.float32)
    return idx, q.reshape(2, 37, 256)


def score_bound(x, vec):
    """Worst-case fp32 error of one score: (C + 2) 2^-24 (max|y|^2 + 2 max|x| max|y|), |.| the Euclidean norm of a vector and
    the maxima over the entries y and the queries x: the norm's sum and the product's sum each round at most C + 1 times on
    terms whose absolute sum is at most |y|^2 and |x| |y| (Cauchy-Schwarz)."""
    C = vec.shape[1]
    mx = float(np.sqrt((x.astype(np.float64) ** 2).sum(-1)).max())
    my = float(np.sqrt((vec.astype(np.float64) ** 2).sum(-1)).max())
    return (C + 2) * 2.0 ** -24 * (my * my + 2 * mx * my)


def kth_gap(x, vec, k):
    """The smallest gap between the k-th and the (k+1)-th fp64 score over the queries x (Q, C)."""
    t = np.sort(scores(x, vec), axis=1)
    return float((t[:, k] - t[:, k - 1]).min())


def blend_bound(vec):
    """4 (C + 2) 2^-24 max|idx|, |.| the Euclidean norm as in `score_bound`: the worst-case rounding of the direct fp32
    distance, carried through the inverse square and the normalisation."""
    return 4 * (vec.shape[1] + 2) * 2.0 ** -24 * float(np.sqrt((np.asarray(vec, dtype=np.float64) ** 2).sum(-1)).max())
