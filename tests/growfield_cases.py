"""Helpers shared by tests/test_growfield_cpu.py and tests/test_gpu_growfield.py: the host form of carrying a tracked field across a
growth of the sample set (include/mpfmt.h, "growing the sample set", TRACKED FIELDS)."""
import numpy as np


def changed_columns(cp_old, rv_old, cp_new, rv_new):
    """bool[N'] over the grown set: every new column, every old column that lost an entry to the radius rule (it keeps fewer rows below
    n_old than it had) or gained one (it holds a row >= n_old).  0-based colptr / rowval of the old and the grown graph."""
    n_old, n_all = len(cp_old) - 1, len(cp_new) - 1
    col = np.repeat(np.arange(n_all), np.diff(cp_new))
    is_new_row = np.asarray(rv_new) >= n_old
    gained = np.bincount(col[is_new_row], minlength=n_all)[:n_old]
    kept = np.bincount(col[~is_new_row], minlength=n_all)[:n_old]
    dirty = np.ones(n_all, dtype=bool)
    dirty[:n_old] = (gained > 0) | (kept < np.diff(cp_old))
    return dirty


def padded_field(C, A, n_all):
    """The old field over the grown set: +Inf and no parent for the new samples."""
    n_add = n_all - len(C)
    return np.concatenate([C, np.full(n_add, np.inf)]), np.concatenate([A, np.zeros(n_add, dtype=np.int64)])


def ball_of_targets(X, center_idx0, radius):
    """1-based samples within `radius` of sample center_idx0: a ball of targets."""
    d = np.sqrt(((X - X[center_idx0]) ** 2).sum(axis=1))
    return np.flatnonzero(d <= radius).astype(np.int64) + 1
