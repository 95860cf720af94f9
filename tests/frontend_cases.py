"""Cases, references and derived tolerances for the data front end (csrc/frontend.hip: k_col_partials, k_col_finish, k_affine,
k_windows) and the initial guesses (k_initial_guess, k_initial_interp in csrc/stream_kernels.h).

Plain numpy and the oracle; the product is not imported.  tests/test_frontend_cases_cpu.py checks the table and that the bounds hold
for a correct implementation (a numpy replay of the kernels' reduction order); tests/test_gpu_frontend.py runs it on the GPU.

Statistics.  STATS_CASES: float32 and float64 x the shapes of STATS_SHAPES.  Columns cycle through the finite classes of
FINITE_CLASSES; every shape of at least 8 columns also holds one column with a NaN, one with +inf and one with -inf; the shapes of one
column take a class each from ONE_COLUMN.  The reference is exact (exact_stats): math.fsum per column on the float64 image of the
inputs, the remainder of the sum by a second fsum, the deviations and their squares in np.longdouble.  Tolerances (check_stats),
derived from two facts -- the kernels sum in double in a fixed order, and float32 inputs are exact in double:
  min, max        equal by value (the sign of a zero is not pinned)
  float32         mean and std within 1 float32 ulp of the correctly rounded exact value; a constant column gives exactly the value and
                  std == 0 (n equal 24-bit values sum exactly in double)
  float64 mean    |err| <= (n - 1) 2^-53 sum|x| / n  (recursive summation of n terms)  + half an ulp (the quotient)
  float64 std     relative error <= (n + 2) 2^-52 + (dm / sigma)^2, dm the mean's bound: a deviation, its square, n - 1 additions, the
                  quotient and the root are (n + 5) / 2 roundings of 2^-53 on the root; the mean's error enters squared, because the
                  deviations from the exact mean sum to zero: sum (x - m)^2 = sum (x - mu)^2 + n (mu - m)^2
  float64 const   std <= n 2^-52 |v|
  NaN / inf       the non-finite pattern of the four outputs is torch's on the CPU for the same column in the same dtype (torch.min and
                  torch.max hand a NaN on); min and max also equal numpy's NaN-propagating ones by value

Affine.  AFFINE_CASES: forward and inverse, standardize (shift = mean, scale = std) and normalize (shift = min, scale = max,
scale_lo = min) with the series' own exact statistics rounded to the dtype.  Reference: numpy in the same dtype, one IEEE operation
after the other; compared bit for bit.

Windows.  WINDOW_CASES; reference series[s : s + win] * mask in numpy, compared on the bit patterns (-3 * 0 is -0, NaN * 0 is NaN).

Initial guesses.  GUESS_SHAPES x (float32, float64), INTERP_FORMS.  Reference: oracle.admm_oracle.initial_guess /
initial_interpolation.  float64: the tolerances of the KATs of tests/test_gpu_parity.py.  float32: the allowance of a case is twice the
largest difference between the oracle on the float32 inputs and the oracle on their float64 image (the reference's own float32 error
on that case; twice, for a different rounding of the same size), at least one float32 ulp of the case's largest |x|.
A case of B * N >= 3 columns marks two of them: one with no observed entry, one with exactly one; every other column observes at least
3 distinct times.  (1, 6, 3, 1) has a single column, which is a regular one.
"""
import functools
import math
import warnings

import numpy as np

from oracle import admm_oracle as orc

F32, F64 = np.float32, np.float64

# ------------------------------------------------------------------------------------------------------------ statistics
STATS_SHAPES = ((2, 1), (3, 65), (4, 64), (5, 63), (255, 257), (256, 1), (257, 64), (513, 65), (300, 33, 2))
FINITE_CLASSES = ("signed", "level", "constant", "negative", "zeros")
NONFINITE_CLASSES = ("nan", "posinf", "neginf")
CLASSES = FINITE_CLASSES + NONFINITE_CLASSES
ONE_COLUMN = {("float32", (2, 1)): "level", ("float32", (256, 1)): "nan", ("float64", (2, 1)): "zeros", ("float64", (256, 1)): "neginf"}
STATS_CASES = tuple((dt, shp) for dt in ("float32", "float64") for shp in STATS_SHAPES)


def case_id(c):
    return "-".join("x".join(str(v) for v in p) if isinstance(p, tuple) else str(p) for p in c)


def stats_classes(dtype, shape):
    """The class of every (flattened) column."""
    n_cols = int(np.prod(shape[1:]))
    if n_cols == 1:
        return [ONE_COLUMN[(dtype, tuple(shape))]]
    cls = [FINITE_CLASSES[j % 5] for j in range(n_cols)]
    if n_cols >= 8:
        cls[5], cls[n_cols - 1], cls[min(40, n_cols - 2)] = "posinf", "nan", "neginf"      # n_cols 65: the NaN is in the second block
    return cls


def _column(cls, n, j, rng, dt):
    z = rng.standard_normal(n)
    if cls == "signed" or cls in NONFINITE_CLASSES:
        col = 50.0 * (z - z.mean())           # zero mean up to rounding: both signs in every column
    elif cls == "level":
        col = 1e4 + 0.1 * z
    elif cls == "constant":
        col = np.full(n, 37.7 + j)
    elif cls == "negative":
        col = -(20.0 * np.abs(z) + 1.0)
    else:                                    # zeros: signed, with -0 first and +0 last
        col = 3.0 * z
        col[0], col[n - 1] = -0.0, 0.0
    col = col.astype(dt)
    if cls == "nan":
        col[(2 * n) // 3] = np.nan           # (513: row 342, chunk 1, row lane 2)
    elif cls == "posinf":
        col[n - 1] = np.inf                  # (257, 513: the only row of the last chunk -- three row lanes hold none)
    elif cls == "neginf":
        col[0] = -np.inf
    return col


@functools.lru_cache(maxsize=None)
def stats_series(dtype, shape):
    """(series of `shape`, class per flattened column)"""
    rng = np.random.default_rng(1000 + STATS_CASES.index((dtype, shape)))
    n, n_cols = shape[0], int(np.prod(shape[1:]))
    cls = stats_classes(dtype, shape)
    x = np.stack([_column(cls[j], n, j, rng, np.dtype(dtype)) for j in range(n_cols)], 1).reshape(shape)
    x.setflags(write=False)
    return x, cls


def exact_stats(x2):
    """Per column of a finite (n, cols) array: min, max (its dtype), mean, std (unbiased; np.longdouble), sum|x| (float64)."""
    x = np.asarray(x2, dtype=F64)
    n = x.shape[0]
    mean = np.empty(x.shape[1], dtype=np.longdouble)
    for j in range(x.shape[1]):
        col = x[:, j].tolist()
        hi = math.fsum(col)                                  # the exact sum, correctly rounded
        lo = math.fsum(col + [-hi])                          # and what that rounding dropped
        mean[j] = (np.longdouble(hi) + np.longdouble(lo)) / np.longdouble(n)
    dev = x.astype(np.longdouble) - mean
    std = np.sqrt((dev * dev).sum(0) / np.longdouble(max(n - 1, 1)))
    return x2.min(0), x2.max(0), mean, std, np.abs(x).sum(0)


def pattern(v):
    """'nan' / '+inf' / '-inf' / 'finite' per entry"""
    v = np.asarray(v, dtype=F64).reshape(-1)
    return ["nan" if np.isnan(a) else "+inf" if a == np.inf else "-inf" if a == -np.inf else "finite" for a in v]


def torch_stats(col):
    """(min, max, mean, std) of one column by torch on the CPU in the column's dtype"""
    import torch
    t = torch.from_numpy(np.array(col))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return tuple(float(v) for v in (t.min(0)[0], t.max(0)[0], t.mean(0), t.std(0)))


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, dtype=F32))).astype(F64)


def _ratio(err, tol):
    return float(err / tol) if tol > 0 else 0.0


def check_stats(dtype, shape, mn, mx, mean, std=None, who=""):
    """Assert the tolerances of the module docstring on outputs of shape (1,) + shape[1:] (numpy, the series' dtype).
    std None: series_stats(std=False).  Returns the largest error / bound ratio per statistic over the finite columns."""
    x, cls = stats_series(dtype, shape)
    n, n_cols = shape[0], len(cls)
    x2 = x.reshape(n, n_cols)
    outs = [np.asarray(a) for a in ((mn, mx, mean) if std is None else (mn, mx, mean, std))]
    for a in outs:
        assert a.dtype == x.dtype and a.shape == (1,) + tuple(shape[1:]), (who, a.dtype, a.shape)
    mn, mx, mean = (a.reshape(n_cols) for a in outs[:3])
    std = outs[3].reshape(n_cols) if std is not None else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        np.testing.assert_array_equal(mn, x2.min(0), err_msg=f"{who} min")        # numpy's min / max hand a NaN on; NaN == NaN here
        np.testing.assert_array_equal(mx, x2.max(0), err_msg=f"{who} max")
    fin = [j for j in range(n_cols) if cls[j] in FINITE_CLASSES]
    for j in range(n_cols):
        if cls[j] in FINITE_CLASSES:
            continue
        want = torch_stats(x2[:, j])
        have = (mn[j], mx[j], mean[j]) + ((std[j],) if std is not None else ())
        assert pattern(have) == pattern(want[:len(have)]), (who, j, cls[j], have, want)
    worst = {"mean": 0.0, "std": 0.0}
    if not fin:
        return worst
    _, _, e_mean, e_std, sabs = exact_stats(x2[:, fin])
    u53 = 2.0 ** -53
    for k, j in enumerate(fin):
        m, s = F64(mean[j]), (F64(std[j]) if std is not None else None)
        assert np.isfinite(m) and (s is None or np.isfinite(s)), (who, j, cls[j], m, s)
        if dtype == "float32":
            cr_m, cr_s = F32(e_mean[k]), F32(e_std[k])
            if cls[j] == "constant":
                assert mean[j] == x2[0, j] and (s is None or s == 0.0), (who, j, mean[j], x2[0, j], s)
                continue
            tol_m = float(ulp32(cr_m))
            err_m = abs(m - F64(cr_m))
            assert err_m <= tol_m, (who, j, cls[j], "mean", m, cr_m, err_m, tol_m)
            worst["mean"] = max(worst["mean"], _ratio(err_m, tol_m))
            if s is not None:
                tol_s = float(ulp32(cr_s))
                err_s = abs(s - F64(cr_s))
                assert err_s <= tol_s, (who, j, cls[j], "std", s, cr_s, err_s, tol_s)
                worst["std"] = max(worst["std"], _ratio(err_s, tol_s))
        else:
            dm = (n - 1) * u53 * sabs[k] / n + 0.5 * np.spacing(abs(F64(e_mean[k])))
            err_m = float(abs(np.longdouble(m) - e_mean[k]))
            assert err_m <= dm, (who, j, cls[j], "mean", m, err_m, dm)
            worst["mean"] = max(worst["mean"], _ratio(err_m, dm))
            if s is None:
                continue
            if cls[j] == "constant" or e_std[k] == 0:          # (a column of -0 and +0 is a constant one)
                tol_s = n * 2.0 ** -52 * abs(float(x2[0, j]))
                assert 0.0 <= s <= tol_s, (who, j, "constant std", s, tol_s)
                continue
            sig = float(e_std[k])
            tol_s = ((n + 2) * 2.0 ** -52 + (dm / sig) ** 2) * sig
            err_s = float(abs(np.longdouble(s) - e_std[k]))
            assert err_s <= tol_s, (who, j, cls[j], "std", s, err_s, tol_s)
            worst["std"] = max(worst["std"], _ratio(err_s, tol_s))
    return worst


# ------------------------------------------------------------------------------------------------------------ affine
AFFINE_CASES = (("float32", (8200, 257)), ("float64", (70, 65)), ("float32", (3, 1)), ("float64", (3, 1)))
AFFINE_MODES = ("standardize", "normalize")


@functools.lru_cache(maxsize=None)
def affine_case(dtype, shape):
    """series, and per mode (shift, scale, scale_lo or None) of shape (1, n_cols) in the dtype, from the exact statistics."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(2000 + AFFINE_CASES.index((dtype, shape)))
    x = (40.0 * rng.standard_normal(shape) + 15.0 * np.arange(shape[1]) % 200 - 60.0).astype(dt)
    mn, mx, mean, std, _ = exact_stats(x)
    par = {"standardize": (mean.astype(dt)[None], std.astype(dt)[None], None), "normalize": (mn[None], mx[None], mn[None])}
    x.setflags(write=False)
    return x, par


def affine_reference(x, shift, scale, scale_lo, inverse):
    """numpy in x's dtype: (x - shift) / sc, or x * sc + shift with two roundings; sc = scale - scale_lo for 'normalize'"""
    assert x.dtype == shift.dtype == scale.dtype
    sc = scale - scale_lo if scale_lo is not None else scale
    if inverse:
        p = x * sc
        return p + shift
    return (x - shift) / sc


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == F32 else np.int64)


# ------------------------------------------------------------------------------------------------------------ windows
def _starts_65535():
    return tuple(int(v) for v in (np.arange(65535) * 7) % 4)


# name: (series shape, win, starts)
WINDOW_CASES = {
    "24x700": ((60, 700), 24, (0, 36, 7, 7, 20, 3)),              # 16 800 elements per window: the stride of k_windows is taken
    "70x257": ((90, 257), 70, (20, 0, 20, 5)),                    # 17 990 elements per window
    "whole": ((24, 12), 24, (0,)),                                # win == n_steps, B = 1
    "win1": ((9, 5, 2), 1, (8, 7, 6, 5, 4, 3, 2, 1, 0, 0, 8)),    # descending and repeated, a feature axis
    "B65535": ((4, 1), 1, None),                                  # starts: _starts_65535()
}
WINDOW_DTYPES = ("float32", "float64")


@functools.lru_cache(maxsize=None)
def window_case(name, dtype):
    """series (signed, one NaN), starts (int64), win, float32 0 / 1 mask of a window; the NaN lies under a hidden entry of window 0
    and a negative value under another."""
    shape, win, starts = WINDOW_CASES[name]
    starts = np.asarray(_starts_65535() if starts is None else starts, dtype=np.int64)
    rng = np.random.default_rng(3000 + sorted(WINDOW_CASES).index(name))
    x = (30.0 * rng.standard_normal(shape)).astype(np.dtype(dtype))
    n_cols = int(np.prod(shape[1:]))
    x2 = x.reshape(shape[0], n_cols)
    mask = (rng.random((win, n_cols)) >= 0.4).astype(F32)
    r_nan, c_nan = int(starts[0]) + win // 2, n_cols // 3
    x2[r_nan, c_nan] = np.nan
    mask[win // 2, c_nan] = 0.0
    r_neg, c_neg = int(starts[0]) + win - 1, n_cols - 1
    if (r_neg, c_neg) != (r_nan, c_nan):
        x2[r_neg, c_neg] = -3.0
        mask[win - 1, c_neg] = 0.0
    if n_cols > 1 or win > 1:
        mask[0, 0] = 1.0
    mask = mask.reshape((win,) + tuple(shape[1:]))
    for a in (x, starts, mask):
        a.setflags(write=False)
    return x, starts, win, mask


def windows_reference(x, starts, win, mask=None):
    out = np.stack([x[s:s + win] for s in starts])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return out * mask[None] if mask is not None else out       # float32 mask: the product keeps the series' dtype


def refused_starts(n_steps, win):
    """Start lists the kernel refuses: one bad index among valid ones.  None depends on how s0 + win is formed."""
    last = n_steps - win
    return [[0, last + 1, last], [last, 0, n_steps], [-1, 0, last], [0, last, 2 ** 40, 0]]


# ------------------------------------------------------------------------------------------------------------ initial guesses
GUESS_SHAPES = ((1, 6, 3, 1), (63, 24, 12, 3), (64, 24, 12, 4), (65, 24, 12, 5), (129, 12, 12, 30), (2, 3, 2, 7))      # B, T, t_in, N
GUESS_DTYPES = ("float32", "float64")
INTERP_FORMS = (("float64", "float32"), ("float64", "float64"), ("float32", "float32"))      # (signal, mask); the first is F32MOM
SCALE = 300.0
F64_GUESS_RTOL = 1e-13
F64_INTERP_RTOL, F64_INTERP_ATOL = 1e-11, 1e-9


def marked_columns(shape):
    """((b, n) with no observed entry, (b, n) with exactly one), or () for a case of fewer than 3 columns"""
    B, T, t_in, N = shape
    if B * N < 3:
        return ()
    none, one = (B - 1, N - 1), (B // 2, N // 2)
    assert none != one
    return none, one


def _allowance(x32, x64):
    """twice the reference's own float32 error, at least one float32 ulp of the largest |x|; over the finite entries"""
    fin = np.isfinite(x64)
    assert np.array_equal(fin, np.isfinite(x32))
    ref_err = float(np.abs(x32.astype(F64) - x64)[fin].max())
    floor = float(ulp32(np.abs(x64[fin]).max()))
    return max(2.0 * ref_err, floor), ref_err, floor


@functools.lru_cache(maxsize=None)
def guess_case(shape, dtype):
    """y (B, t_in, N, 1) in the dtype, the oracle's x, and for float32 (allowance, reference error, floor)"""
    B, T, t_in, N = shape
    rng = np.random.default_rng(4000 + GUESS_SHAPES.index(shape))
    y = (SCALE * rng.standard_normal((B, t_in, N, 1))).astype(np.dtype(dtype))
    x = orc.initial_guess(y, t_in, T)
    assert x.dtype == y.dtype and x.shape == (B, T, N, 1)
    allow = None
    if dtype == "float32":
        allow = _allowance(x, orc.initial_guess(y.astype(F64), t_in, T))
    for a in (y, x):
        a.setflags(write=False)
    return y, x, allow


@functools.lru_cache(maxsize=None)
def interp_case(shape, form):
    """y = signal * mask (B, T, N, 1), mask, the oracle's x, and for the float32 form (allowance, reference error, floor)"""
    B, T, t_in, N = shape
    sdt, mdt = (np.dtype(d) for d in form)
    rng = np.random.default_rng(5000 + GUESS_SHAPES.index(shape))
    sig = (SCALE * rng.standard_normal((B, T, N, 1))).astype(sdt)
    obs = rng.random((B, T, N, 1)) >= 0.4
    few = obs.sum(1) < 3                                     # (B, N, 1): give such a column the first, the middle and the last step
    for t in (0, T // 2, T - 1):
        obs[:, t] |= few
    marks = marked_columns(shape)
    if marks:
        (b0, n0), (b1, n1) = marks
        obs[b0, :, n0] = False
        obs[b1, :, n1] = False
        obs[b1, T // 2, n1] = True
    mask = obs.astype(mdt)
    y = sig * mask.astype(sdt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # 0 / 0 on the marked columns
        x = orc.initial_interpolation(y, mask)
        assert x.dtype == sdt
        allow = None
        if form == ("float32", "float32"):
            allow = _allowance(x, orc.initial_interpolation(y.astype(F64), mask.astype(F64)))
    for a in (y, mask, x):
        a.setflags(write=False)
    return y, mask, x, allow


def check_guess(got, want, dtype, allow, who="", rtol=F64_GUESS_RTOL, atol=0.0):
    """The non-finite entries are the oracle's; the finite ones obey the case's tolerance.  Returns the largest finite error."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (who, got.dtype, got.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), (who, "non-finite entries differ", int((np.isfinite(got) != fin).sum()))
    err = np.abs(got.astype(F64) - want.astype(F64))[fin]
    if dtype == "float32":
        tol, ref_err, floor = allow
        print(f"{who}: allowance {tol:.3e} (reference's float32 error {ref_err:.3e}, ulp floor {floor:.3e}), observed {err.max():.3e}")
        assert err.max() <= tol, (who, float(err.max()), tol)
    else:
        bound = atol + rtol * np.abs(want.astype(F64))[fin]
        print(f"{who}: rtol {rtol:g} atol {atol:g}, observed {err.max():.3e}, largest error / bound {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all(), (who, float(err.max()))
    return float(err.max())
