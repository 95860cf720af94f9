"""The data front end (csrc/frontend.hip) and the initial guesses (k_initial_guess, k_initial_interp) on the GPU, at the shapes,
types and values of tests/frontend_cases.py: exact references and derived tolerances for the statistics, bit patterns for the affine
transform and the windows, the oracle for the initial guesses.  tests/test_frontend_cases_cpu.py checks the table and its bounds
without a GPU; the start index that wraps a signed sum is checked on the CPU only (tests/test_frontend_geom_cpu.py)."""
import os
import warnings

import numpy as np
import pytest
import torch

import frontend_cases as fc

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("case", fc.STATS_CASES, ids=fc.case_id)
def test_series_stats_meet_the_derived_bounds(case):
    from mgadmm.dataset import series_stats
    dt, shp = case
    x, _ = fc.stats_series(dt, shp)
    s = dev(x)
    out = [host(t) for t in series_stats(s)]
    assert len(out) == 4
    worst = fc.check_stats(dt, shp, *out, who=f"series_stats {fc.case_id(case)}")
    print(f"{fc.case_id(case)}: largest error / bound over the finite columns: mean {worst['mean']:.3f}, std {worst['std']:.3f}")
    out3 = [host(t) for t in series_stats(s, std=False)]
    assert len(out3) == 3
    fc.check_stats(dt, shp, *out3, who="series_stats(std=False)")
    for a, b in zip(out, out3):
        np.testing.assert_array_equal(fc.bits(a), fc.bits(b))       # fixed-order reductions: the same bits with and without the std
    np.testing.assert_array_equal(fc.bits(host(s)), fc.bits(x))      # the series is only read


def test_series_stats_refuse_more_steps_than_one_launch_covers():
    """16 776 961 steps are 65 536 row chunks, one more than gridDim.y takes: refused by name before anything is allocated."""
    from mgadmm import _lib
    from mgadmm.dataset import series_stats
    s = torch.zeros((16776961, 1), dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.MgadmmError, match="at most 16 776 960 time steps"):
        series_stats(s)
    with pytest.raises(_lib.MgadmmError, match="at most 16 776 960 time steps"):
        series_stats(s, std=False)
    del s
    dt, shp = "float32", (5, 63)
    out = [host(t) for t in series_stats(dev(fc.stats_series(dt, shp)[0]))]
    fc.check_stats(dt, shp, *out, who="after the refusal")


# ------------------------------------------------------------------------------------------------------------ affine
@pytest.mark.parametrize("case", fc.AFFINE_CASES, ids=fc.case_id)
def test_affine_is_bitwise_ieee(case):
    from mgadmm.dataset import TrafficDataset
    dt, shp = case
    x, par = fc.affine_case(dt, shp)
    for mode in fc.AFFINE_MODES:
        shift, scale, lo = par[mode]
        d_shift, d_scale, d_lo = dev(shift), dev(scale), (dev(lo) if lo is not None else None)
        want_f = fc.affine_reference(x, shift, scale, lo, False)
        want_b = fc.affine_reference(want_f, shift, scale, lo, True)
        for inverse, src, want in ((False, x, want_f), (True, want_f, want_b)):
            t = dev(src)
            r = TrafficDataset._affine(t, d_shift, d_scale, d_lo, inverse=inverse)
            assert r is t
            got = host(t)
            diff = fc.bits(got) != fc.bits(want)
            n_bad = int(diff.sum())
            if n_bad:
                i = tuple(int(v[0]) for v in np.nonzero(diff))
                print(f"{fc.case_id(case)} {mode} inverse={inverse}: {n_bad} of {diff.size} differ; first at {i}: got {got[i]!r}, want {want[i]!r}, "
                      f"x {src[i]!r}, shift {shift[0, i[1]]!r}, scale {scale[0, i[1]]!r}, lo {None if lo is None else lo[0, i[1]]!r}")
            assert n_bad == 0, (case, mode, inverse, n_bad)


# ------------------------------------------------------------------------------------------------------------ windows
@pytest.mark.parametrize("dt", fc.WINDOW_DTYPES)
@pytest.mark.parametrize("name", list(fc.WINDOW_CASES))
def test_windows_equal_numpy_on_the_bit_patterns(name, dt):
    from mgadmm.dataset import gather_windows
    x, starts, win, mask = fc.window_case(name, dt)
    s = dev(x)
    for m, st in ((None, starts.tolist()), (mask, torch.from_numpy(np.array(starts)))):
        want = fc.windows_reference(x, starts, win, m)
        got = gather_windows(s, st, win, mask=None if m is None else torch.from_numpy(np.array(m)))
        assert tuple(got.shape) == want.shape and got.dtype == s.dtype
        np.testing.assert_array_equal(fc.bits(host(got)), fc.bits(want))


@pytest.mark.parametrize("dt", fc.WINDOW_DTYPES)
def test_windows_refuse_a_bad_start_among_valid_ones(dt):
    from mgadmm import _lib
    from mgadmm.dataset import gather_windows
    for name in ("24x700", "whole", "win1"):
        x, starts, win, mask = fc.window_case(name, dt)
        s = dev(x)
        want = fc.windows_reference(x, starts, win, mask)
        for bad in fc.refused_starts(x.shape[0], win):
            with pytest.raises(_lib.MgadmmError, match="start index"):
                gather_windows(s, bad, win)
            got = gather_windows(s, starts.tolist(), win, mask=torch.from_numpy(np.array(mask)))       # and the next call is right
            np.testing.assert_array_equal(fc.bits(host(got)), fc.bits(want))
    x, starts, win, mask = fc.window_case("B65535", dt)
    s = dev(x)
    with pytest.raises(_lib.MgadmmError, match="at most 65535 windows"):
        gather_windows(s, [0] * 65536, 1)
    with pytest.raises(_lib.MgadmmError, match="window of 5 steps"):
        gather_windows(s, [0], 5)
    np.testing.assert_array_equal(fc.bits(host(gather_windows(s, starts.tolist(), win))), fc.bits(fc.windows_reference(x, starts, win)))


# ------------------------------------------------------------------------------------------------------------ initial guesses
@pytest.mark.parametrize("dt", fc.GUESS_DTYPES)
@pytest.mark.parametrize("shape", fc.GUESS_SHAPES, ids=fc.case_id)
def test_initial_guess_matches_the_oracle(shape, dt):
    from mgadmm.ADMM import initial_guess
    B, T, t_in, N = shape
    y, want, allow = fc.guess_case(shape, dt)
    got = initial_guess(torch.from_numpy(np.array(y)), t_in, T)
    assert got.dtype == torch.from_numpy(np.array(y)).dtype and not got.is_cuda
    fc.check_guess(got.numpy(), want, dt, allow, who=f"initial_guess {fc.case_id((shape, dt))}")
    np.testing.assert_array_equal(fc.bits(got.numpy()[:, :t_in]), fc.bits(y))          # the observed steps are copied


@pytest.mark.parametrize("form", fc.INTERP_FORMS, ids=fc.case_id)
@pytest.mark.parametrize("shape", fc.GUESS_SHAPES, ids=fc.case_id)
def test_initial_interpolation_matches_the_oracle(shape, form):
    from mgadmm.ADMM import initial_interpolation
    y, mask, want, allow = fc.interp_case(shape, form)
    got = initial_interpolation(torch.from_numpy(np.array(y)), torch.from_numpy(np.array(mask)))
    who = f"initial_interpolation {fc.case_id((shape,) + form)}"
    if form[0] == "float32":
        fc.check_guess(got.numpy(), want, "float32", allow, who=who)
    else:
        fc.check_guess(got.numpy(), want, "float64", None, who=who, rtol=fc.F64_INTERP_RTOL, atol=fc.F64_INTERP_ATOL)
    marks = fc.marked_columns(shape)
    if marks:
        for b, n in marks:
            assert not np.isfinite(got.numpy()[b, :, n]).any()


# ------------------------------------------------------------------------------------------------------------ data set from files
@pytest.mark.parametrize("transform", ["normalize", "standardize"])
def test_dataset_with_a_nan_column_has_the_references_pattern(tmp_path, transform):
    """A float32 series with one NaN sample: torch.min / torch.max / mean / std make that whole column NaN, and so does the
    transform; every other column stays finite.  The references are torch's reductions on the CPU."""
    import pandas as pd
    from mgadmm.dataset import TrafficDataset
    rng = np.random.default_rng(7)
    T, N = 300, 9
    raw = (200.0 + 40.0 * rng.standard_normal((T, N, 2))).astype(np.float32)
    raw[171, 4, 0] = np.nan
    raw[5, 2, 1] = np.nan                                      # second feature: dropped on load
    np.savez(os.path.join(tmp_path, "series.npz"), data=raw)
    pd.DataFrame({"from": list(range(N - 1)), "to": list(range(1, N)), "cost": [1.0 + i for i in range(N - 1)]}).to_csv(
        os.path.join(tmp_path, "dist.csv"), index=False)
    ds = TrafficDataset(str(tmp_path), "series.npz", "dist.csv", transform=transform, verbose=False)
    assert ds.data.dtype == torch.float32 and tuple(ds.data.shape) == (T, N, 1) and ds.graph_info["n_nodes"] == N
    data = torch.from_numpy(raw[..., :1].copy())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r_max, r_min = data.max(0, keepdim=True)[0], data.min(0, keepdim=True)[0]
        r_mean, r_std = data.mean(0, keepdim=True), data.std(0, keepdim=True)
    r_data = (data - r_mean) / r_std if transform == "standardize" else (data - r_min) / (r_max - r_min)
    for nm, got, want in (("data", ds.data, r_data), ("min", ds.data_min, r_min), ("max", ds.data_max, r_max), ("mean", ds.data_mean, r_mean),
                          ("std", ds.data_std, r_std)):
        assert tuple(got.shape) == tuple(want.shape), nm
        assert fc.pattern(host(got)) == fc.pattern(want.numpy()), nm
    assert torch.isnan(ds.data[:, 4]).all() and torch.isfinite(ds.data[:, [0, 1, 2, 3, 5, 6, 7, 8]]).all()
    ok = [0, 1, 2, 3, 5, 6, 7, 8]
    assert torch.equal(ds.data_min.cpu()[:, ok], r_min[:, ok]) and torch.equal(ds.data_max.cpu()[:, ok], r_max[:, ok])
    rec = ds.recover_data(ds.data[:24])
    r_rec = r_data[:24] * r_std + r_mean if transform == "standardize" else r_data[:24] * (r_max - r_min) + r_min
    assert fc.pattern(host(rec)) == fc.pattern(r_rec.numpy()) and torch.isnan(rec[:, 4]).all()      # (utils.py:110-118)
