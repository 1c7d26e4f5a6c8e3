"""numpy float64 restatement of the identity scoring kernels (tpg_identity.hip): unit rows, the
full similarity matrix, and the top-k rule -- score descending, equal scores by the lower gallery
index, one skipped index per probe, -1 / -inf past the eligible rows -- plus the rigorous float32
error bound the GPU tests hold the kernels to."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


def normalize(x):
    """float64 unit rows of x (a row of norm 0 stays 0) and the norms."""
    x = np.asarray(x, np.float64)
    n = np.sqrt((x * x).sum(1))
    return x / np.where(n == 0, 1.0, n)[:, None], n


def similarity(pu, gu):
    """float64 [P, G] dot products of unit rows."""
    return np.asarray(pu, np.float64) @ np.asarray(gu, np.float64).T


def bound(pu, gu):
    """Per (probe, gallery row): (3 D + 16) * 2^-24 * sum_k |p_k g_k| on the float64 unit rows.
    D * u is the k-ordered float32 fmaf chain of D products (gamma_D ~ D u, any fixed order); each
    float32 normalisation (sum of squares of D terms, sqrt, divide, and the rounding of the stored
    unit value) is within (D / 2 + 3) u relative per element, (D + 6) u for both operands of a
    product; the rest covers second-order terms."""
    pu, gu = np.asarray(pu, np.float64), np.asarray(gu, np.float64)
    return (3 * pu.shape[1] + 16) * U * (np.abs(pu) @ np.abs(gu).T)


def pair_bound(au, bu):
    """The same bound for row-wise pairs: float64 [n]."""
    au, bu = np.asarray(au, np.float64), np.asarray(bu, np.float64)
    return (3 * au.shape[1] + 16) * U * (np.abs(au) * np.abs(bu)).sum(1)


def topk(sim, k, skip=None):
    """(idx int32 [P, k], score float64 [P, k]) of a [P, G] similarity matrix: a stable sort by
    (-score, index) of the gallery rows other than skip[p]; slots past them hold -1 / -inf."""
    sim = np.asarray(sim, np.float64)
    P, G = sim.shape
    idx = np.full((P, k), -1, np.int32)
    score = np.full((P, k), -np.inf, np.float64)
    for p in range(P):
        rows = np.lexsort((np.arange(G), -sim[p]))  # by -score, then by index
        if skip is not None:
            rows = rows[rows != int(skip[p])]
        for r, g in enumerate(rows[:k]):
            idx[p, r] = g
            score[p, r] = sim[p, g]
    return idx, score


def cosine_pairs(a, b):
    au, _ = normalize(a)
    bu, _ = normalize(b)
    return (au * bu).sum(1)
