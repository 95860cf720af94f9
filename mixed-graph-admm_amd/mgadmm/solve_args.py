"""What a solve is given beyond ``y`` and ``mask`` -- ``sample_params``, ``graph_params`` / ``graph_sets`` / ``graph_of_sample``,
``param_schedule`` / ``schedule_start``, ``adaptive_rho`` / ``adaptive_start``, ``band_params`` / ``band_sets`` /
``band_of_sample`` (their checks: ``band_args.py``) -- checked before the library is touched, and
set on a solver for the solves of one ``with`` block.  No GPU work here; ``ADMM.py`` is the caller.

Order of refusals, a contract like the one of ``csrc/solve_gate.h``: ``parse_solve_args`` raises the first that is due of
  1. ``sample_params``;
  2. ``param_schedule``: not a dict, ``schedule_start``, then per entry in the dict's order: unknown key, given in
     ``sample_params`` too, shape, the shape of the entries before it, not finite, sign;
  3. the graph arguments: ``graph_of_sample`` without sets, ``graph_params`` with ``graph_sets``, a line graph, then
     ``graph_params`` (which builds the tables of every distinct pair here) or ``graph_sets`` and ``graph_of_sample``;
  4. ``adaptive_rho`` and ``adaptive_start``;
  5. ``adaptive_rho`` together with ``param_schedule``;
  6. the band arguments (``band_args.check_band_args``).
``y`` and ``mask`` are checked after all of these, ``warm_start`` inside the scope, after the set calls.

Order of set and clear calls: ``solve_scope`` sets the sample table, the graph table (its device graphs created first), the
schedule, the adaptive penalties and the band table, and clears them in the reverse order with the return codes ignored.  A set call that
refuses raises ``MgadmmError`` and is not cleared, what was set before it is; the graph table alone is cleared whenever it
was entered -- also when a graph could not be created or its set call refused -- and its graphs are closed after that.
"""
import collections
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib
from .band_args import check_band_args

SAMPLE_PARAM_NAMES = ("rho", "rho_u", "rho_d", "mu_u", "mu_d1", "mu_d2")
GRAPH_PARAM_NAMES = ("u_sigma", "d_sigma")
ADAPTIVE_RHO_KEYS = ("every", "mu", "tau", "until", "rho_min", "rho_max")


def _float64(vals):
    """A tensor or a sequence as a float64 array."""
    return np.asarray(vals.detach().cpu().numpy() if torch.is_tensor(vals) else vals, dtype=np.float64)


def _need_dict(arg, d, keys):
    if not hasattr(d, "items"):
        raise ValueError(f"{arg} must be a dict with keys out of {keys}, got {type(d).__name__}")


def _need_key(arg, key, keys):
    if key not in keys:
        raise ValueError(f"{arg}: unknown key {key!r} (expected some of {keys})")


def _check_arrays(arg, d, keys, B, rows=False, twice=()):
    """The dict-of-arrays arguments: ``d`` as ``(dict name -> contiguous float64 array, shape of the entries)``.  Every entry has
    shape (B,), or with ``rows`` (K,) / (K, B), K >= 1, the same for all; rho* > 0, mu* >= 0, *_sigma > 0, all finite; no name
    out of ``twice``.  ValueError names the first entry, and the first element by index, that breaks a rule."""
    _need_dict(arg, d, keys)
    out, shape = {}, None
    for name, vals in d.items():
        _need_key(arg, name, keys)
        if name in twice:
            raise ValueError(f"{arg}[{name!r}] is given twice: in {arg} and in sample_params")
        v = _float64(vals)
        v = np.ascontiguousarray(v) if v.ndim or not rows else v          # (which turns a scalar into (1,): kept for `rows`)
        if rows:
            if v.ndim not in (1, 2) or v.shape[0] < 1 or (v.ndim == 2 and v.shape[1] != B):
                raise ValueError(f"{arg}[{name!r}] must have shape (K,) or (K, B = {B}) with K >= 1, got shape {tuple(v.shape)}")
            if shape is not None and v.shape != shape:
                raise ValueError(f"{arg}[{name!r}] has shape {tuple(v.shape)}, the entries before it {tuple(shape)}: "
                                 "one number of rows and one form (shared or per-sample) for all")
        elif v.ndim != 1 or v.shape[0] != B:
            raise ValueError(f"{arg}[{name!r}] must be 1-D of length B = {B}, got shape {tuple(v.shape)}")
        shape = v.shape
        at = lambda idx: "".join(f"[{int(i)}]" for i in idx)
        if not np.isfinite(v).all():
            raise ValueError(f"{arg}[{name!r}]{at(np.argwhere(~np.isfinite(v))[0])} is not finite")
        positive = name in GRAPH_PARAM_NAMES or name.startswith("rho")
        bad = np.argwhere(v <= 0 if positive else v < 0)
        if bad.size:
            raise ValueError(f"{arg}[{name!r}]{at(bad[0])} = {v[tuple(bad[0])]}: "
                             + ("u_sigma and d_sigma must be > 0" if name in GRAPH_PARAM_NAMES else
                                "rho, rho_u and rho_d must be > 0" if positive else "mu_u, mu_d1 and mu_d2 must be >= 0"))
        out[name] = v
    return out, shape


def _check_sample_params(sample_params, B):
    """``sample_params`` of ``solve``: dict name -> 1-D sequence / tensor of length B, as a dict name -> float64 array.
    Raises ValueError for an unknown name, a wrong length, a value that is not finite, rho* <= 0 or mu* < 0 (what
    ``mgadmm_solver_set_sample_params`` refuses, found before the library is touched)."""
    return _check_arrays("sample_params", sample_params, SAMPLE_PARAM_NAMES, B)[0]


def _check_param_schedule(param_schedule, B, schedule_start=0, sample_params=None):
    """``param_schedule`` of ``solve``: dict name -> array of shape (K,) (shared form) or (K, B) (per-sample form), the same K
    and the same form for every name, as ``(dict name -> float64 array, K, 0 or B)``.  Raises ValueError for an unknown name,
    a wrong shape, a value that is not finite, rho* <= 0 or mu* < 0 (named by [row][b]), a name that ``sample_params`` gives
    too, or a negative ``schedule_start`` (what ``mgadmm_solver_set_param_schedule`` refuses, found before the library is
    touched)."""
    _need_dict("param_schedule", param_schedule, SAMPLE_PARAM_NAMES)
    if int(schedule_start) != schedule_start or schedule_start < 0:
        raise ValueError(f"schedule_start must be an integer >= 0, got {schedule_start!r}")
    out, shape = _check_arrays("param_schedule", param_schedule, SAMPLE_PARAM_NAMES, B, rows=True, twice=sample_params or ())
    if shape is None:
        return out, 0, 0
    return out, int(shape[0]), (int(shape[1]) if len(shape) == 2 else 0)


def _check_adaptive_rho(adaptive_rho, adaptive_start=0):
    """``adaptive_rho`` of ``solve``: dict with ``every`` (1 ... 16), ``mu`` > 1 (default 10), ``tau`` > 1 (default 2), ``until``
    (None: no limit), ``rho_min`` / ``rho_max`` (a number for all three penalties, or three in the order rho, rho_u, rho_d, or a
    dict by name; defaults 1e-6 / 1e6) -> the ``_lib.AdaptiveRho`` struct.  ValueError for what
    ``mgadmm_solver_set_adaptive_rho`` refuses, found before the library is touched."""
    _need_dict("adaptive_rho", adaptive_rho, ADAPTIVE_RHO_KEYS)
    for k2 in adaptive_rho:
        _need_key("adaptive_rho", k2, ADAPTIVE_RHO_KEYS)
    if adaptive_rho.get("every") is None:
        raise ValueError("adaptive_rho needs 'every' (iterations between two adaptation steps, 1 ... 16)")
    every, start = int(adaptive_rho["every"]), int(adaptive_start)
    until = adaptive_rho.get("until")
    until = 0 if until is None else int(until)
    mu, tau = float(adaptive_rho.get("mu", 10.0)), float(adaptive_rho.get("tau", 2.0))
    if not 1 <= every <= 16:
        raise ValueError(f"adaptive_rho: every = {every} outside [1, 16] (the iterations of one launch)")
    if not mu > 1.0 or not tau > 1.0:
        raise ValueError(f"adaptive_rho: mu = {mu} and tau = {tau} should both be > 1")
    if until < 0:
        raise ValueError(f"adaptive_rho: until = {until} is negative (None: no limit)")
    if start < 0 or start % every:
        raise ValueError(f"adaptive_start = {start} must be a non-negative multiple of every = {every}")

    def three(name, default):
        v = adaptive_rho.get(name)
        if v is None:
            return [default] * 3
        if hasattr(v, "items"):
            if set(v) - set(SAMPLE_PARAM_NAMES[:3]):
                raise ValueError(f"adaptive_rho[{name!r}]: unknown keys {sorted(set(v) - set(SAMPLE_PARAM_NAMES[:3]))}")
            return [float(v.get(nm, default)) for nm in SAMPLE_PARAM_NAMES[:3]]
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            return [float(a)] * 3
        if a.shape != (3,):
            raise ValueError(f"adaptive_rho[{name!r}] must be a number, three numbers (rho, rho_u, rho_d) or a dict by name")
        return [float(t) for t in a]
    lo, hi = three("rho_min", 1e-6), three("rho_max", 1e6)
    for nm, a, b in zip(SAMPLE_PARAM_NAMES[:3], lo, hi):
        if not (0.0 < a <= b < float("inf")):
            raise ValueError(f"adaptive_rho: rho_min[{nm}] = {a}, rho_max[{nm}] = {b}, should be 0 < rho_min <= rho_max (finite)")
    ar = _lib.AdaptiveRho(every=every, until=until, mu=mu, tau=tau)
    ar.rho_min[:], ar.rho_max[:] = lo, hi
    return ar, start


def geometric_ramp(v0, factor, n_rows, vmax=None):
    """Rows of a geometric schedule: ``v0 * factor ** row`` for row = 0 .. n_rows - 1 as a float64 array, capped at ``vmax``
    when given (``solve(param_schedule={'rho': geometric_ramp(rho, 1.1, 20)})``; the last row holds for the rest of a solve)."""
    if int(n_rows) != n_rows or n_rows < 1:
        raise ValueError(f"geometric_ramp: n_rows must be an integer >= 1, got {n_rows!r}")
    if not (np.isfinite(v0) and np.isfinite(factor) and v0 > 0 and factor > 0):
        raise ValueError(f"geometric_ramp: v0 and factor must be finite and > 0, got {v0!r}, {factor!r}")
    v = float(v0) * float(factor) ** np.arange(int(n_rows), dtype=np.float64)
    return v if vmax is None else np.minimum(v, float(vmax))


def _check_graph_sets(blk, graph_sets, graph_of_sample, graph_params, B):
    """The graph arguments of ``solve`` on the instance ``blk`` as ``(sets, set_of_sample)`` -- a list of (u_ew, d_ew) tables and
    an int32 array of length B -- or None without them.  ValueError for what can be refused before the library is touched."""
    if graph_params is None and graph_sets is None:
        if graph_of_sample is not None:
            raise ValueError("graph_of_sample needs graph_sets")
        return None
    if graph_params is not None and graph_sets is not None:
        raise ValueError("graph_params and graph_sets exclude each other (graph_params builds the sets itself)")
    if blk.use_line_graph:
        raise ValueError("graph_params / graph_sets: a line-graph instance has no spatial W_d tables to vary (use_line_graph=True)")
    if graph_params is not None:
        gp = _check_arrays("graph_params", graph_params, GRAPH_PARAM_NAMES, B)[0]
        if getattr(blk, "dist_list", None) is None:
            raise ValueError("graph_params: the instance was built without distances (dist_list), its tables cannot be rebuilt")
        cols = [gp[nm].tolist() if nm in gp else [getattr(blk, nm)] * B for nm in GRAPH_PARAM_NAMES]
        pairs, index = [], {}
        gos = np.zeros(B, dtype=np.int32)
        for b, pair in enumerate(zip(*cols)):
            if pair not in index:
                index[pair] = len(pairs)
                pairs.append(pair)
            gos[b] = index[pair]
        return [blk._weight_tables(us, ds)[:2] for us, ds in pairs], gos
    sets = []
    for j, pair in enumerate(graph_sets):
        if not isinstance(pair, (tuple, list)) or len(pair) != 2:
            raise ValueError(f"graph_sets[{j}] must be a pair (u_ew, d_ew)")
        u_ew, d_ew = (torch.as_tensor(t).float() for t in pair)
        for nm, t, own in (("u_ew", u_ew, blk.u_ew), ("d_ew", d_ew, blk.d_ew)):
            if tuple(t.shape) not in (tuple(own.shape), tuple(own.shape[-2:])):
                raise ValueError(f"graph_sets[{j}]: {nm} has shape {tuple(t.shape)}, the instance's has {tuple(own.shape)}")
        sets.append((u_ew, d_ew))
    if not sets:
        raise ValueError("graph_sets is empty")
    if graph_of_sample is None:
        raise ValueError("graph_sets needs graph_of_sample (the set of every sample)")
    gos = graph_of_sample.detach().cpu().numpy() if torch.is_tensor(graph_of_sample) else np.asarray(graph_of_sample)
    if gos.ndim != 1 or gos.shape[0] != B or gos.dtype.kind not in "iu":
        raise ValueError(f"graph_of_sample must be B = {B} integers, got shape {tuple(gos.shape)} of {gos.dtype}")
    bad = np.nonzero((gos < 0) | (gos >= len(sets)))[0]
    if bad.size:
        raise ValueError(f"graph_of_sample[{int(bad[0])}] = {int(gos[bad[0]])} out of range for {len(sets)} graph sets")
    return sets, np.ascontiguousarray(gos, dtype=np.int32)


# the checked arguments of one call: the outputs of the four checkers (None where the argument was not given) and the start values
SolveArgs = collections.namedtuple("SolveArgs", "sp sch gs ar schedule_start adaptive_start bs", defaults=(None,))


def parse_solve_args(blk, B, sample_params=None, graph_sets=None, graph_of_sample=None, graph_params=None, param_schedule=None,
                     schedule_start=0, adaptive_rho=None, adaptive_start=0, band_params=None, band_sets=None, band_of_sample=None):
    """``solve``'s keywords for a batch of B samples of the instance ``blk`` as ``SolveArgs``, in the module's order of refusals."""
    sp = _check_sample_params(sample_params, B) if sample_params is not None else None
    sch = _check_param_schedule(param_schedule, B, schedule_start, sp) if param_schedule is not None else None
    gs = blk._check_graph_sets(graph_sets, graph_of_sample, graph_params, B)
    ar = _check_adaptive_rho(adaptive_rho, adaptive_start) if adaptive_rho is not None else None
    if ar is not None and sch is not None:
        raise ValueError("adaptive_rho and param_schedule exclude each other (the adaptation writes the table a schedule would fill)")
    bs = check_band_args(blk, band_params, band_sets, band_of_sample, B)
    return SolveArgs(sp, sch, gs, ar, schedule_start, adaptive_start, bs)


@contextlib.contextmanager
def _scoped(setter, set_args, clear_args):
    """``setter(*set_args)`` with its return code checked, the block, then ``setter(*clear_args)`` with its return code ignored."""
    _lib.check(setter(*set_args))
    try:
        yield
    finally:
        setter(*clear_args)


@contextlib.contextmanager
def _graph_table(blk, h, Cn, gs, B):
    """Per-sample graph weights (``_check_graph_sets`` output) set on solver ``h`` for the solves inside the block: a device
    graph per set, closed when the block ends, where the table is cleared as well."""
    sets, gos = gs
    graphs = []
    try:
        for u_ew, d_ew in sets:
            graphs.append(blk._make_graph(Cn, u_ew, d_ew))
        handles = (C.c_void_p * len(graphs))(*[g.handle for g in graphs])
        _lib.check(_lib.lib.mgadmm_solver_set_sample_graphs(h, len(graphs), handles, gos.ctypes.data_as(C.POINTER(C.c_int32)), B))
        yield
    finally:
        _lib.lib.mgadmm_solver_set_sample_graphs(h, 0, None, None, 0)
        for g in graphs:
            g.close()


def _table(arrays):
    t = _lib.SampleParams()             # (_lib.ParamSchedule is the same struct)
    for nm, v in arrays.items():
        setattr(t, nm, v.ctypes.data_as(C.POINTER(C.c_double)))
    return t


@contextlib.contextmanager
def solve_scope(blk, h, Cn, B, args):
    """``args`` (``SolveArgs``) set on solver ``h`` for the solves inside the block and cleared after it -- the next solve of the
    instance is an ordinary one -- in the module's order of set and clear calls."""
    lib = _lib.lib
    with contextlib.ExitStack() as scope:
        if args.sp:
            scope.enter_context(_scoped(lib.mgadmm_solver_set_sample_params, (h, C.byref(_table(args.sp)), B), (h, None, 0)))
        if args.gs is not None:
            scope.enter_context(_graph_table(blk, h, Cn, args.gs, B))
        if args.sch is not None and args.sch[0]:
            arrays, n_rows, cols = args.sch
            scope.enter_context(_scoped(lib.mgadmm_solver_set_param_schedule,
                                        (h, C.byref(_table(arrays)), n_rows, cols, int(args.schedule_start)), (h, None, 0, 0, 0)))
        if args.ar is not None:
            scope.enter_context(_scoped(lib.mgadmm_solver_set_adaptive_rho, (h, C.byref(args.ar[0]), int(args.adaptive_start)), (h, None, 0)))
        if args.bs is not None:
            tables, bos = args.bs
            scope.enter_context(_scoped(lib.mgadmm_solver_set_sample_bands,
                                        (h, len(tables), tables.ctypes.data_as(C.POINTER(C.c_float)), bos.ctypes.data_as(C.POINTER(C.c_int32)), B),
                                        (h, 0, None, None, 0)))
        yield
