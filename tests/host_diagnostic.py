"""The diagnostic variables' definition restated in numpy (include/rscm_gpu.h, "diagnostic variables"): per member and row
    w_k = scale_k * P[row_k]   (or scale_k alone where the term has no parameter row)
    y   = w_0 * x_0;  y = y + w_k * x_k  for k = 1 .. K - 1 in order
elementwise in float64, every product and sum one IEEE operation.  Nothing else."""
import numpy as np

from tests.helpers import two_layer_noise_case as two_layer_case  # noqa: F401  (the GPU file's two-layer handles)


def weights(terms, P):
    """[K] weights, each [N] (or a scalar for a term without a parameter row); ``terms``: (source, param_row_or_None, scale)."""
    out = []
    with np.errstate(all="ignore"):
        for _, row, scale in terms:
            out.append(np.float64(scale) if row is None else np.float64(scale) * np.asarray(P, dtype=np.float64)[row])
    return out


def diagnostic(terms, sources, P):
    """[R][N]: ``sources[k]`` is the [R][N] rows of term k's variable, ``P`` the [P][N] parameter block."""
    w = weights(terms, P)
    with np.errstate(all="ignore"):
        y = w[0] * np.asarray(sources[0], dtype=np.float64)
        for k in range(1, len(terms)):
            y = y + w[k] * np.asarray(sources[k], dtype=np.float64)
    return y


def diagnostic_right_to_left(terms, sources, P):
    """The same terms summed from the last to the first: what the definition is NOT."""
    w = weights(terms, P)
    with np.errstate(all="ignore"):
        y = w[-1] * np.asarray(sources[-1], dtype=np.float64)
        for k in range(len(terms) - 2, -1, -1):
            y = y + w[k] * np.asarray(sources[k], dtype=np.float64)
    return y


HEAT_CONTENT = [(1, 4, 1.0), (2, 5, 1.0)]    # C Ts + Cd Td of a two-layer handle: the GPU file's two-term case
RANDOM_ROWS = (10, 11, 12)                   # the rows of that case that hold random_rows() instead of the run's values


def random_rows(n, offset=0, n_total=None):
    """[2][3][n]: what the GPU file writes into RANDOM_ROWS of the two stored variables -- random doubles with full mantissas and
    mixed signs, so that a fused multiply-add would round differently from multiply-then-add somewhere."""
    n_total = n if n_total is None else n_total
    rng = np.random.default_rng(7919 + n_total)
    x = np.where(rng.random((2, 3, n_total)) < 0.5, -1.0, 1.0) * rng.uniform(0.01, 5.0, (2, 3, n_total))
    return np.ascontiguousarray(x[:, :, offset:offset + n])


def random_case(n_terms, n_members, n_rows=3, n_params=10, seed=20260418):
    """Data that can expose a contraction or another order: doubles with full mantissas and mixed signs and magnitudes.
    Returns (terms, sources [K][R][N], P [n_params][N])."""
    rng = np.random.default_rng(seed + 97 * n_terms)
    sign = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    P = sign((n_params, n_members)) * rng.uniform(0.5, 200.0, (n_params, n_members))
    sources = sign((n_terms, n_rows, n_members)) * rng.uniform(0.01, 5.0, (n_terms, n_rows, n_members))
    scales = (1.0, -2.5, 16.1, 0.3)
    terms = [(k + 1, (4 + k) % n_params, scales[k]) for k in range(n_terms)]
    return terms, sources, P
