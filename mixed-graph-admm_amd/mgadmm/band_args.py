"""The band arguments of a solve on a line-graph instance -- ``band_params`` / ``band_sets`` / ``band_of_sample`` of ``solve``,
``skips`` of ``sweep`` -- checked before the library is touched.  Every sample of a batch reads its own temporal band table
(``mgadmm_solver_set_sample_bands``): ``T x skip`` weights, row t = the weights of x[t-1-s], of the instance's width
``skip_connection``.  A narrower skip-connection interval is a table of that width whose further hops are zero.

``check_band_args`` is called by ``solve_args.parse_solve_args`` after every other check of that module; all refusals are
ValueError.  No GPU work here.
"""
import numpy as np
import torch

from . import utils as _u

BAND_PARAM_NAMES = ("skip",)


def _integers(arg, vals, n=None):
    """``vals`` as a 1-D array of integers (of length ``n`` if given)."""
    a = vals.detach().cpu().numpy() if torch.is_tensor(vals) else np.asarray(vals)
    if a.ndim == 1 and a.size == 0:
        a = a.astype(np.int64)                  # (an empty list has no dtype of its own)
    if a.ndim != 1 or (n is not None and a.shape[0] != n) or a.dtype.kind not in "iu":
        want = "a 1-D sequence of integers" if n is None else f"B = {n} integers"
        raise ValueError(f"{arg} must be {want}, got shape {tuple(a.shape)} of {a.dtype}")
    return a.astype(np.int64)


def skip_table(T, skip, width):
    """The band table of the skip-connection interval ``skip`` in a table of ``width`` hops: ``utils.skip_connection_tables``
    (rows ``1 / min(t, skip)``), zero beyond the interval, as a float32 array (T, width)."""
    if not 1 <= skip <= width:
        raise ValueError(f"skip = {skip} outside [1, skip_connection = {width}] (the width of the instance's band table)")
    tab = np.zeros((T, width), dtype=np.float32)
    tab[:, :skip] = _u.skip_connection_tables(1, T, skip)[0][:, :, 0].numpy()
    return tab


def check_skips(blk, skips):
    """``skips`` of ``sweep``: a non-empty 1-D sequence of integers in [1, skip_connection] of a line-graph instance, as a list."""
    if not blk.use_line_graph:
        raise ValueError("sweep: skips needs a line-graph instance (use_line_graph=True); a spatial temporal graph has no band table")
    vals = _integers("sweep: skips", skips)
    if vals.size == 0:
        raise ValueError("sweep: skips is empty")
    bad = np.nonzero((vals < 1) | (vals > blk.skip_connection))[0]
    if bad.size:
        raise ValueError(f"sweep: skips[{int(bad[0])}] = {int(vals[bad[0]])} outside [1, skip_connection = {blk.skip_connection}]")
    return [int(v) for v in vals]


def check_band_args(blk, band_params, band_sets, band_of_sample, B):
    """The band arguments of ``solve`` on the instance ``blk`` as ``(tables, set_of_sample)`` -- a contiguous float32 array
    (S, T, skip_connection) and an int32 array of length B -- or None without them.  ValueError for what can be refused before
    the library is touched: ``band_of_sample`` without sets, both forms given, an instance without a line graph, then
    ``band_params`` (not a dict, an unknown key, shape, range) or ``band_sets`` (empty, shape, not finite) and
    ``band_of_sample`` (missing, shape, range)."""
    if band_params is None and band_sets is None:
        if band_of_sample is not None:
            raise ValueError("band_of_sample needs band_sets")
        return None
    if band_params is not None and band_sets is not None:
        raise ValueError("band_params and band_sets exclude each other (band_params builds the sets itself)")
    if not blk.use_line_graph:
        raise ValueError("band_params / band_sets: the instance has no line graph (use_line_graph=False), its temporal graph "
                         "has no band table to vary")
    T, width = int(blk.T), int(blk.skip_connection)
    if band_params is not None:
        if not hasattr(band_params, "items"):
            raise ValueError(f"band_params must be a dict with the key 'skip', got {type(band_params).__name__}")
        for key in band_params:
            if key not in BAND_PARAM_NAMES:
                raise ValueError(f"band_params: unknown key {key!r} (expected {BAND_PARAM_NAMES[0]!r})")
        if "skip" not in band_params:
            raise ValueError("band_params needs 'skip' (the skip-connection interval of every sample)")
        skips = _integers("band_params['skip']", band_params["skip"], B)
        bad = np.nonzero((skips < 1) | (skips > width))[0]
        if bad.size:
            raise ValueError(f"band_params['skip'][{int(bad[0])}] = {int(skips[bad[0]])} outside [1, skip_connection = {width}]")
        distinct = list(dict.fromkeys(int(s) for s in skips))          # in order of first appearance
        tables = np.stack([skip_table(T, s, width) for s in distinct])
        bos = np.array([distinct.index(int(s)) for s in skips], dtype=np.int32)
        return np.ascontiguousarray(tables), bos
    sets = []
    for j, tab in enumerate(band_sets):
        a = np.asarray(tab.detach().cpu().numpy() if torch.is_tensor(tab) else tab, dtype=np.float32)
        if a.shape != (T, width):
            raise ValueError(f"band_sets[{j}] has shape {tuple(a.shape)}, the instance's band table has (T, skip_connection) = {(T, width)}")
        read = np.arange(width)[None, :] < np.minimum(np.arange(T), width)[:, None]          # the entries an operator reads
        bad = np.argwhere(read & ~np.isfinite(a))
        if bad.size:
            raise ValueError(f"band_sets[{j}][{int(bad[0][0])}][{int(bad[0][1])}] is not finite")
        sets.append(a)
    if not sets:
        raise ValueError("band_sets is empty")
    if band_of_sample is None:
        raise ValueError("band_sets needs band_of_sample (the set of every sample)")
    bos = _integers("band_of_sample", band_of_sample, B)
    bad = np.nonzero((bos < 0) | (bos >= len(sets)))[0]
    if bad.size:
        raise ValueError(f"band_of_sample[{int(bad[0])}] = {int(bos[bad[0]])} out of range for {len(sets)} band sets")
    return np.ascontiguousarray(np.stack(sets)), np.ascontiguousarray(bos, dtype=np.int32)
