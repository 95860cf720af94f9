"""Weight tables that vary over time (``ADMM_algorithm(time_varying=True)``): which tables take the per-slice path, and their
slices.  The reference's operators broadcast ``u_ew`` of shape (T, N, k) and ``d_ew`` of shape (T-1, N, k+1) slice by slice
(ADMM.py:147, 171, 200, 214); its constructor stores repeats of one slice, which the one-slice device graph serves."""
import os


def keep_slices():
    """``MGADMM_TV_KEEP=1`` (a test hook): tables of equal slices keep the per-slice path instead of collapsing to one slice."""
    return os.environ.get("MGADMM_TV_KEEP") == "1"


def table_slices(tab, name, n_slices):
    """``tab`` as its ``n_slices`` slices (a list of (N, k) tables), or None where the one-slice graph serves: a 2-D table, a
    single slice, or equal slices -- unless ``keep_slices()``.  ValueError for another leading size, naming the table and both
    shapes."""
    keep = keep_slices()
    if tab.dim() != 3 or tab.shape[0] == 1:
        return [tab.reshape(tab.shape[-2:])] * n_slices if keep else None
    if tab.shape[0] != n_slices:
        raise ValueError(f"{name} has shape {tuple(tab.shape)}, a time-varying table of this instance has shape "
                         f"{(n_slices,) + tuple(tab.shape[1:])}")
    if not keep and bool((tab == tab[0:1]).all()):
        return None
    return list(tab)
