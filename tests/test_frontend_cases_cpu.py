"""tests/frontend_cases.py without a GPU: the table holds what it says, and its derived bounds hold for a correct implementation.

replay_stats repeats the reduction order of k_col_partials / k_col_finish (csrc/frontend.hip) in numpy float64: chunks of 256 rows;
in a chunk four row lanes of stride 4, each summing its rows in order; the lanes combined 0 to 3; the chunks combined in order; the
mean a quotient in double, rounded once to the series' dtype; the second pass sums squared deviations from the double mean the same
way; min and max hand a NaN on.  Every statistics case must pass check_stats on that replay."""
import warnings

import numpy as np
import pytest

import frontend_cases as fc


def _nan_min(a, v):
    return np.where((v < a) | (v != v), v, a)


def _nan_max(a, v):
    return np.where((v > a) | (v != v), v, a)


def _chunk_sums(vals, n):
    """vals(r) -> the float64 row r of what is summed; returns the total in the kernels' order"""
    total = None
    for r0 in range(0, n, 256):
        r1 = min(r0 + 256, n)
        lanes = []
        for ry in range(4):
            s = 0.0
            for r in range(r0 + ry, r1, 4):
                s = s + vals(r)
            lanes.append(s)
        t = lanes[0]
        for j in range(1, 4):
            t = t + lanes[j]
        total = (0.0 + t) if total is None else total + t
    return total


def replay_stats(x2):
    n = x2.shape[0]
    xd = x2.astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mn, mx = None, None
        for r0 in range(0, n, 256):
            r1 = min(r0 + 256, n)
            a = b = None
            for ry in range(4):
                la = lb = None
                for r in range(r0 + ry, r1, 4):
                    la = x2[r] if la is None else _nan_min(la, x2[r])
                    lb = x2[r] if lb is None else _nan_max(lb, x2[r])
                if la is not None:                   # a row lane that holds no row takes no part
                    a = la if a is None else _nan_min(a, la)
                    b = lb if b is None else _nan_max(b, lb)
            mn = a if mn is None else _nan_min(mn, a)
            mx = b if mx is None else _nan_max(mx, b)
        mean_d = _chunk_sums(lambda r: xd[r], n) / float(n)

        def sq(r):
            d = xd[r] - mean_d
            return d * d
        std_d = np.sqrt(_chunk_sums(sq, n) / float(n - 1))
    return mn, mx, mean_d.astype(x2.dtype), std_d.astype(x2.dtype)


# ------------------------------------------------------------------------------------------------------------ the table
def test_every_shape_and_class_is_present():
    assert len(fc.STATS_CASES) == 18 and {c[1] for c in fc.STATS_CASES} == set(fc.STATS_SHAPES)
    assert set(fc.STATS_SHAPES) == {(2, 1), (3, 65), (4, 64), (5, 63), (255, 257), (256, 1), (257, 64), (513, 65), (300, 33, 2)}
    n_cols = n_bad = 0
    for dt, shp in fc.STATS_CASES:
        x, cls = fc.stats_series(dt, shp)
        assert x.dtype == np.dtype(dt) and x.shape == shp and len(cls) == int(np.prod(shp[1:]))
        if len(cls) >= 8:
            assert set(cls) == set(fc.CLASSES) and all(cls.count(c) == 1 for c in fc.NONFINITE_CLASSES), (dt, shp)
        x2 = x.reshape(shp[0], -1)
        for j, c in enumerate(cls):
            col = x2[:, j]
            bad = ~np.isfinite(col)
            assert bad.sum() == (1 if c in fc.NONFINITE_CLASSES else 0)
            if c == "nan":
                assert np.isnan(col).sum() == 1
            elif c == "posinf":
                assert (col == np.inf).sum() == 1
            elif c == "neginf":
                assert (col == -np.inf).sum() == 1
            elif c == "constant":
                assert (col == col[0]).all() and col[0] != 0
            elif c == "negative":
                assert (col < 0).all()
            elif c == "zeros":
                assert np.signbit(col[0]) and col[0] == 0 and col[-1] == 0 and not np.signbit(col[-1])
            elif c == "level":
                assert np.abs(col.astype(np.float64) - 1e4).max() < 1.0
            else:
                assert (col < 0).any() and (col > 0).any() and abs(col.astype(np.float64).mean()) < 1e-4
        n_cols += len(cls)
        n_bad += sum(c in fc.NONFINITE_CLASSES for c in cls)
    one = [fc.stats_classes(dt, shp)[0] for dt, shp in fc.STATS_CASES if int(np.prod(shp[1:])) == 1]
    assert len(set(one)) == 4                                  # the one-column shapes rotate through the classes
    assert 0 < n_bad < 0.05 * n_cols, (n_bad, n_cols)


@pytest.mark.parametrize("case", fc.STATS_CASES, ids=fc.case_id)
def test_the_bounds_hold_for_a_replay_of_the_kernels_order(case):
    dt, shp = case
    x, cls = fc.stats_series(dt, shp)
    x2 = x.reshape(shp[0], -1)
    out = [a.reshape((1,) + shp[1:]) for a in replay_stats(x2)]
    worst = fc.check_stats(dt, shp, *out, who=f"replay {fc.case_id(case)}")
    fc.check_stats(dt, shp, *out[:3], who="replay, std=False")
    assert worst["mean"] <= 1.0 and worst["std"] <= 1.0
    print(f"{fc.case_id(case)}: largest error / bound over the finite columns: mean {worst['mean']:.3f}, std {worst['std']:.3f}")
    # torch's own same-dtype results on the finite columns beside the exact ones: where torch leaves a relative 1e-12
    import torch
    fin = [j for j, c in enumerate(cls) if c in fc.FINITE_CLASSES and c != "constant" and x2[:, j].any()]
    if fin:
        _, _, e_mean, e_std, sabs = fc.exact_stats(x2[:, fin])
        t = torch.from_numpy(np.array(x2[:, fin]))
        rel_m = np.abs((t.mean(0).numpy().astype(np.longdouble) - e_mean) / (sabs / shp[0])).astype(np.float64)      # of the mean |x|
        rel_s = np.abs((t.std(0).numpy().astype(np.longdouble) - e_std) / e_std).astype(np.float64)
        k = int(rel_s.argmax())
        print(f"    torch {dt} vs exact: mean err / mean|x| up to {rel_m.max():.2e}, std rel err up to {rel_s.max():.2e} "
              f"(column {fin[k]}, class {cls[fin[k]]}: torch {float(t.std(0)[k])!r}, exact {float(e_std[k])!r})")


def test_a_wrong_reduction_misses_the_bounds():
    """The bounds are not so wide that they accept anything: a float32 accumulator, a biased std, a min that drops a NaN."""
    dt, shp = "float32", (513, 65)
    x, cls = fc.stats_series(dt, shp)
    x2 = x.reshape(shp[0], -1)
    mn, mx, mean, std = [a.reshape(1, 65) for a in replay_stats(x2)]
    fc.check_stats(dt, shp, mn, mx, mean, std)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        acc32 = np.zeros(65, dtype=np.float32)
        for r in range(513):
            acc32 = acc32 + x2[r]
        with pytest.raises(AssertionError):
            fc.check_stats(dt, shp, mn, mx, (acc32 / np.float32(513)).reshape(1, 65), std)
        with pytest.raises(AssertionError):
            fc.check_stats(dt, shp, mn, mx, mean, (std.astype(np.float64) * np.sqrt(512 / 513)).astype(np.float32))
        with pytest.raises(AssertionError):
            fc.check_stats(dt, shp, np.nanmin(x2, 0).reshape(1, 65), mx, mean, std)
    dt = "float64"
    x, cls = fc.stats_series(dt, shp)
    x2 = x.reshape(shp[0], -1)
    mn, mx, mean, std = [a.reshape(1, 65) for a in replay_stats(x2)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        one_pass = np.sqrt(np.maximum((x2 * x2).sum(0) / 513 - mean[0] ** 2, 0) * 513 / 512).reshape(1, 65)     # E[x^2] - mean^2 cancels at level 1e4
        with pytest.raises(AssertionError):
            fc.check_stats(dt, shp, mn, mx, mean, one_pass)


def test_affine_and_window_tables():
    assert fc.AFFINE_CASES[0] == ("float32", (8200, 257)) and 8200 * 257 == 2107400 > 8192 * 256
    assert ("float64", (70, 65)) in fc.AFFINE_CASES and {c[1] for c in fc.AFFINE_CASES} >= {(3, 1)}
    for dt, shp in fc.AFFINE_CASES[1:]:
        x, par = fc.affine_case(dt, shp)
        for mode in fc.AFFINE_MODES:
            shift, scale, lo = par[mode]
            assert shift.dtype == scale.dtype == x.dtype and shift.shape == (1, shp[1])
            f = fc.affine_reference(x, shift, scale, lo, False)
            back = fc.affine_reference(f, shift, scale, lo, True)
            assert f.dtype == back.dtype == x.dtype and np.isfinite(f).all()
            np.testing.assert_allclose(back, x, rtol=0, atol=64 * np.finfo(x.dtype).eps * np.abs(x).max())
    big = {n for n, (shp, win, _) in fc.WINDOW_CASES.items() if win * int(np.prod(shp[1:])) > 64 * 256}
    assert big == {"24x700", "70x257"}
    for name, (shp, win, _) in fc.WINDOW_CASES.items():
        for dt in fc.WINDOW_DTYPES:
            x, starts, w, mask = fc.window_case(name, dt)
            n = shp[0]
            assert x.dtype == np.dtype(dt) and mask.dtype == np.float32 and set(np.unique(mask)) <= {0.0, 1.0}
            assert starts.min() >= 0 and starts.max() <= n - w and np.isnan(x).sum() == 1 and (x < 0).any()
            ref = fc.windows_reference(x, starts, w, mask)
            assert ref.dtype == x.dtype and ref.shape == (len(starts), w) + shp[1:]
            hidden = np.broadcast_to(mask[None] == 0, ref.shape)
            assert np.isnan(ref[hidden]).any()                                     # NaN * 0 under a hidden entry
            assert (np.signbit(ref[hidden]) & (ref[hidden] == 0)).any()            # -x * 0 = -0
            for bad in fc.refused_starts(n, w):
                assert sum(not (0 <= s <= n - w) for s in bad) == 1 and len(bad) >= 3
    s = fc.window_case("24x700", "float32")[1]
    assert 0 in s and 36 in s and list(s).count(7) == 2
    assert len(fc.window_case("B65535", "float32")[1]) == 65535
    assert fc.WINDOW_CASES["whole"][1] == fc.WINDOW_CASES["whole"][0][0] and len(fc.WINDOW_CASES["whole"][2]) == 1
    d = list(fc.WINDOW_CASES["win1"][2])
    assert fc.WINDOW_CASES["win1"][1] == 1 and d[:9] == sorted(d[:9], reverse=True)


def test_initial_guess_tables():
    assert fc.GUESS_SHAPES == ((1, 6, 3, 1), (63, 24, 12, 3), (64, 24, 12, 4), (65, 24, 12, 5), (129, 12, 12, 30), (2, 3, 2, 7))
    for shp in fc.GUESS_SHAPES:
        B, T, t_in, N = shp
        for dt in fc.GUESS_DTYPES:
            y, x, allow = fc.guess_case(shp, dt)
            assert y.dtype == np.dtype(dt) and (y < 0).any() and 100 < np.abs(y).max() < 2000 and np.isfinite(x).all()
            if dt == "float32":
                tol, ref_err, floor = allow
                assert np.isfinite(tol) and tol > 0 and tol == max(2 * ref_err, floor) and floor > 0
                print(f"guess {shp}: allowance {tol:.3e} (reference's float32 error {ref_err:.3e}, floor {floor:.3e})")
        marks = fc.marked_columns(shp)
        assert len(marks) == (2 if B * N >= 3 else 0)
        for form in fc.INTERP_FORMS:
            y, mask, x, allow = fc.interp_case(shp, form)
            assert y.dtype == x.dtype == np.dtype(form[0]) and mask.dtype == np.dtype(form[1])
            n_obs = (mask != 0).sum(1)[..., 0]                                    # (B, N); with a 0 / 1 mask: distinct times
            regular = np.ones((B, N), dtype=bool)
            if marks:
                (b0, n0), (b1, n1) = marks
                assert n_obs[b0, n0] == 0 and n_obs[b1, n1] == 1
                regular[b0, n0] = regular[b1, n1] = False
                assert not np.isfinite(x[b0, :, n0]).any() and not np.isfinite(x[b1, :, n1]).any()
            assert (n_obs[regular] >= 3).all() and np.isfinite(x[np.broadcast_to(regular[:, None, :, None], x.shape)]).all()
            if form == ("float32", "float32"):
                tol, ref_err, floor = allow
                assert np.isfinite(tol) and tol > 0 and tol == max(2 * ref_err, floor) and floor > 0
                print(f"interp {shp}: allowance {tol:.3e} (reference's float32 error {ref_err:.3e}, floor {floor:.3e})")
            else:
                assert allow is None
