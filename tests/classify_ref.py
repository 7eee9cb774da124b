"""The yardstick of pcv_classify_f32: a numpy restatement of its total order and of softmax / nll in float64. It is written from the
definition ("NaN above +inf, otherwise larger first, equal values by lower index, all NaNs tie, -0 ties with +0"), with float
comparisons and a stable sort - not from the kernel's integer keys - so that the two can disagree."""

import numpy as np


def _tier_value(x):
    """(tier, value) per entry: tier 1 = NaN (all NaNs tie: value 0), tier 0 = a number. Float comparison makes -0 == +0."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    return nan.astype(np.int8), np.where(nan, np.float32(0), x).astype(np.float64)


def order(x):
    """[N, J] indices: every row's entries from first to last in the total order."""
    tier, val = _tier_value(x)
    out = np.empty(val.shape, dtype=np.int64)
    idx = np.arange(val.shape[1])
    for n in range(val.shape[0]):
        out[n] = np.lexsort((idx, -val[n], -tier[n]))          # last key first: NaNs, then larger values, then lower index
    return out


def topk(x, k):
    return order(x)[:, :k]


def rank(x, labels):
    """[N] number of entries that precede (x[label], label); a label outside [0, J) gives J."""
    tier, val = _tier_value(x)
    N, J = val.shape
    labels = np.asarray(labels, dtype=np.int64)
    out = np.full(N, J, dtype=np.int64)
    idx = np.arange(J)
    for n in range(N):
        l = int(labels[n])
        if 0 <= l < J:
            t, v = tier[n], val[n]
            before = (t > t[l]) | ((t == t[l]) & ((v > v[l]) | ((v == v[l]) & (idx < l))))
            out[n] = int(before.sum())
    return out


def softmax64(x):
    """float64 softmax of the fp32 rows (finite rows only)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def nll64(x, labels):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    m = x.max(axis=1)
    lse = np.log(np.exp(x - m[:, None]).sum(axis=1)) + m
    return lse - x[np.arange(x.shape[0]), np.asarray(labels, dtype=np.int64)]


def topk_error_count(x, labels, k):
    return int((rank(x, labels) >= k).sum())


def natural_nan_row(x):
    """Rows whose softmax is NaN in the natural computation: a NaN, a +inf, or nothing but -inf."""
    x = np.asarray(x, dtype=np.float32)
    return np.isnan(x).any(axis=1) | np.isposinf(x).any(axis=1) | np.isneginf(x).all(axis=1)


def special_rows(J, rng):
    """The special rows of the sweep for row length J, fp32 [S, J]."""
    def base():
        return rng.standard_normal(J).astype(np.float32)
    rows = []
    r = base(); r[0] = np.nan; rows.append(r)                                   # NaN first
    r = base(); r[J - 1] = np.nan; rows.append(r)                               # NaN last
    r = base(); r[J // 2] = np.nan; rows.append(r)                              # NaN in the middle
    r = base(); r[[0, J // 2, J - 1]] = np.nan; rows.append(r)                  # several
    r = base()                                                                  # NaNs of other bit patterns tie with the plain one
    u = r.view(np.uint32)
    u[J // 2] = 0xFFC00000
    u[J - 1] = 0x7FC00001
    u[0] = 0x7FC00000 if J > 2 else u[0]
    rows.append(r)
    r = base(); r[0] = np.inf; r[J // 2] = np.inf; r[J - 1] = -np.inf; rows.append(r)      # +-inf, +inf twice where J allows
    r = base(); r[J // 3] = -np.inf; rows.append(r)                             # a -inf among finite values
    r = np.where(rng.integers(0, 2, J) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32); rows.append(r)   # mixed +-0
    r = np.where(rng.integers(0, 2, J) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    r[rng.integers(0, J)] = -1.0; r[rng.integers(0, J)] = 1.0; rows.append(r)   # ... around +-1
    rows.append(np.full(J, 1.5, dtype=np.float32))                              # all equal
    rows.append(np.full(J, np.nan, dtype=np.float32))                           # all NaN
    rows.append(np.full(J, -np.inf, dtype=np.float32))                          # only -inf
    rows.append(np.arange(J, dtype=np.float32))                                 # ascending
    rows.append(-np.arange(J, dtype=np.float32))                                # descending
    return np.stack(rows)
