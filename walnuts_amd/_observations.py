"""``data=`` / ``datasets=`` of ``DeviceEngine`` and ``walnuts_device`` as the library takes them: one wn_observations
(include/walnuts_hip.h) and the arrays it points into."""
from __future__ import annotations

import numpy as np

from . import _ffi


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _is_grouped(data) -> bool:
    """data is an (x, y, group) triple rather than an (x, y) pair"""
    try:
        return len(data) == 3
    except TypeError:
        return False


def _block(data, num_params: int, cols: int):
    """One block of observations as contiguous arrays (x, y, group, J).  A pair (x, y): x (num_obs, cols) float64, y
    (num_obs,) float64, group None, J 0.  A triple (x, y, group) of a grouped model (kUsesGroups): x (num_obs, P), group
    (num_obs,) int32 and J = num_params - P - 1 (the engine checks J >= 1, P >= 1 and the range)."""
    grouped = _is_grouped(data)
    if grouped:
        x, y, group = data
    else:
        try:
            x, y = data
        except (TypeError, ValueError):
            raise ValueError("data must be a pair (x, y)") from None
    x, y = _f64(x), _f64(y)
    if grouped and x.ndim != 2:
        raise ValueError(f"data x must have shape (num_obs, P), got {x.shape}")
    if not grouped and (x.ndim != 2 or x.shape[1] != cols):
        raise ValueError(f"data x must have shape (num_obs, {cols}), got {x.shape}")
    if y.ndim != 1 or y.shape[0] != x.shape[0]:
        raise ValueError(f"data y must have shape ({x.shape[0]},), got {y.shape}")
    if x.shape[0] < 1:
        raise ValueError("data needs at least one observation")
    if not grouped:
        return x, y, None, 0
    g = np.asarray(group)
    if g.shape != y.shape:
        raise ValueError(f"data group must have shape ({x.shape[0]},), got {g.shape}")
    if g.dtype.kind not in "iu":
        raise ValueError(f"data group must hold integers, got dtype {g.dtype}")
    if g.size and (g.min() < np.iinfo(np.int32).min or g.max() > np.iinfo(np.int32).max):
        raise ValueError("every group must be in [0, num_groups)")
    return x, y, np.ascontiguousarray(g, dtype=np.int32), num_params - x.shape[1] - 1


def _blocks(datasets, num_params: int, cols: int):
    """Several datasets [(x0, y0), ...] or [(x0, y0, group0), ...] as one block, stacked in order: (x, y, group, J) as
    _block gives them, and int64 offsets [G + 1] (dataset g = rows offsets[g] .. offsets[g + 1])."""
    try:
        items = list(datasets)
    except TypeError:
        raise ValueError("datasets must be a sequence of (x, y) pairs or (x, y, group) triples") from None
    if not items:
        raise ValueError("datasets needs at least one (x, y) pair")
    grouped = _is_grouped(items[0])
    if any(_is_grouped(d) != grouped for d in items):
        raise ValueError("datasets must be all (x, y) pairs or all (x, y, group) triples")
    try:
        parts = [_block(d, num_params, cols) for d in items]
    except TypeError:
        if grouped:
            raise
        raise ValueError("datasets must be a sequence of (x, y) pairs") from None
    if grouped and len({p[0].shape[1] for p in parts}) != 1:
        raise ValueError("every dataset's x must have the same number of columns")
    offsets = np.zeros(len(parts) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([p[1].size for p in parts])
    x = np.ascontiguousarray(np.concatenate([p[0] for p in parts], axis=0))
    y = np.ascontiguousarray(np.concatenate([p[1] for p in parts]))
    group = np.ascontiguousarray(np.concatenate([p[2] for p in parts])) if grouped else None
    return x, y, group, parts[0][3], offsets


def observations(lib, model: int, num_params: int, data=None, datasets=None):
    """The wn_observations of `data=(x, y[, group])` or `datasets=[(x0, y0[, group0]), ...]`, or None without either.
    The struct keeps the arrays it points into alive (`.arrays`); pass it with ctypes.byref."""
    if data is not None and datasets is not None:
        raise ValueError("data and datasets are mutually exclusive")
    if data is None and datasets is None:
        return None
    # columns of x of a flat data model (wn_model_data_columns): num_params, or num_params - 1 for a model with a scale
    # parameter.  An id that holds no flat data model gives num_params, and the engine then refuses the model (or the
    # pair (x, y) for a grouped model) with its own message.
    cols = int(lib.wn_model_data_columns(int(model), int(num_params), 0))
    cols = cols if cols >= 0 else int(num_params)
    obs = _ffi.Observations()
    if datasets is not None:
        x, y, group, J, offsets = _blocks(datasets, num_params, cols)
        obs.obs_offsets, obs.num_datasets = offsets.ctypes.data_as(_ffi._i64p), offsets.size - 1
    else:
        x, y, group, J = _block(data, num_params, cols)
        offsets = None
        obs.num_obs = y.size
    obs.x, obs.y = x.ctypes.data_as(_ffi._dp), y.ctypes.data_as(_ffi._dp)
    if group is not None:
        obs.group, obs.num_groups = group.ctypes.data_as(_ffi._i32p), J
    obs.arrays = (x, y, group, offsets)
    return obs
