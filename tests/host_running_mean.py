"""The restatement of the running-mean diagnostics (rscm_ens_define_running_mean; the definition is stated in include/rscm_gpu.h) in
numpy, written as the loop it is, and two functions that state what the definition is NOT: the reversed order and the sliding
update.  Every add and the division is one float64 operation over a whole row of members."""
import numpy as np


def back(window, align):
    """The terms of a window before its row: window - 1 ("trailing") or (window - 1) // 2 ("centre")."""
    assert align in ("trailing", "centre"), align
    return window - 1 if align == "trailing" else (window - 1) // 2


def valid_rows(n_rows, window, align, step=1):
    """(first, last): the first and the last row of a series of n_rows rows whose window is complete (last < first: none)."""
    b = back(window, align)
    return b * step, n_rows - 1 - (window - 1 - b) * step


def running_mean(x, window, align, step, t_begin, t_end, t_stride):
    """[R][N]: the rows t_begin, t_begin + t_stride, ... < t_end of the running mean of x[T][N]."""
    x = np.asarray(x, dtype=np.float64)
    b = back(window, align)
    out = []
    with np.errstate(all="ignore"):
        for t in range(t_begin, t_end, t_stride):
            assert t - b * step >= 0 and t + (window - 1 - b) * step < x.shape[0], (t, window, align, step)
            s = x[t - b * step].copy()
            for j in range(1, window):
                s = s + x[t + (j - b) * step]
            out.append(s / float(window))
    return np.array(out, dtype=np.float64).reshape(len(out), *x.shape[1:])


def all_rows(x, window, align, step=1):
    """(values, first_index): every row of x with a complete window, as rscm_amd.variability.series_running_mean returns them."""
    first, last = valid_rows(np.asarray(x).shape[0], window, align, step)
    return running_mean(x, window, align, step, first, last + 1, 1), first


def reversed_order(x, window, align, step, t_begin, t_end, t_stride):
    """NOT the definition: the same terms added from the last to the first."""
    x = np.asarray(x, dtype=np.float64)
    b = back(window, align)
    out = []
    with np.errstate(all="ignore"):
        for t in range(t_begin, t_end, t_stride):
            s = x[t + (window - 1 - b) * step].copy()
            for j in range(window - 2, -1, -1):
                s = s + x[t + (j - b) * step]
            out.append(s / float(window))
    return np.array(out, dtype=np.float64)


def sliding_update(x, window, align, step, t_begin, t_end):
    """NOT the definition: the first row as defined, every later one from the sum before it, s + new - old (rows step apart, so that
    consecutive windows share all but one term)."""
    x = np.asarray(x, dtype=np.float64)
    b = back(window, align)
    out = []
    with np.errstate(all="ignore"):
        s = None
        for t in range(t_begin, t_end, step):
            if s is None:
                s = x[t - b * step].copy()
                for j in range(1, window):
                    s = s + x[t + (j - b) * step]
            else:
                s = s + x[t + (window - 1 - b) * step] - x[t - (b + 1) * step]
            out.append(s / float(window))
    return np.array(out, dtype=np.float64)


def mixed_sign_rows(n_rows, n_members, seed=20261021):
    """[n_rows][n_members] of +-uniform(0.01, 5): full mantissas of mixed sign, on which the order of a sum shows in its bits."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.01, 5.0, (n_rows, n_members)) * rng.choice([-1.0, 1.0], (n_rows, n_members))
