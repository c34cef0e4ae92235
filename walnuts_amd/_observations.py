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


def _block(data, num_params: int, cols: int, varying: int = 1, scales: int = 0):
    """One block of observations as contiguous arrays (x, y, group, J).  A pair (x, y): x (num_obs, cols) float64, y
    (num_obs,) float64, group None, J 0.  A triple (x, y, group) of a grouped model (kUsesGroups): x (num_obs, P), group
    (num_obs,) int32 and J = (num_params - P - scales) / varying - 1, varying = Q the number of coefficients that vary by
    group (kVaryingSlopes; 1: J = num_params - P - 1 - scales) and scales = wn_model_num_scale_params(model), the
    trailing log scales of the likelihood (0 or 1); a remainder is refused here, and the engine checks J >= 1, P >= 1,
    Q - 1 <= P and the range."""
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
    rest = num_params - x.shape[1] - scales
    if rest % varying != 0:
        minus, plus = (f" - {scales}", f" + {scales}") if scales else ("", "")
        raise ValueError(f"num_params - P{minus} must be a multiple of varying (num_params == P + varying * (J + 1){plus}), "
                         f"got num_params {num_params}, P {x.shape[1]}, varying {varying}")
    return x, y, np.ascontiguousarray(g, dtype=np.int32), rest // varying - 1


def _blocks(datasets, num_params: int, cols: int, varying: int = 1, scales: int = 0):
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
        parts = [_block(d, num_params, cols, varying, scales) for d in items]
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


def _row_terms(name: str, value, sizes, several: bool):
    """`offset=` / `weights=` as one float64 array over all rows, or None.  With `data=`: an array of shape (num_obs,).
    With `datasets=`: a sequence with one entry per dataset, each an array of that dataset's (num_obs,) or None (offset
    0 / weight 1 there); all None gives None."""
    if value is None:
        return None
    fill = 1.0 if name == "weights" else 0.0
    if not several:
        a = _f64(value)
        if a.shape != (sizes[0],):
            raise ValueError(f"{name} must have shape ({sizes[0]},), got {a.shape}")
        return a
    try:
        items = list(value)
    except TypeError:
        raise ValueError(f"{name} must be a sequence with one array (or None) per dataset") from None
    if len(items) != len(sizes):
        raise ValueError(f"{name} must have one entry per dataset ({len(sizes)}), got {len(items)}")
    if all(v is None for v in items):
        return None
    parts = []
    for g, (v, n) in enumerate(zip(items, sizes)):
        a = np.full(n, fill) if v is None else _f64(v)
        if a.shape != (n,):
            raise ValueError(f"{name} of dataset {g} must have shape ({n},), got {a.shape}")
        parts.append(a)
    return np.ascontiguousarray(np.concatenate(parts))


def observations(lib, model: int, num_params: int, data=None, datasets=None, offset=None, weights=None,
                 weight_sets=None, varying: int = 1):
    """The wn_observations of `data=(x, y[, group])` or `datasets=[(x0, y0[, group0]), ...]`, or None without either,
    with the per-row `offset=` and `weights=` (one array, or one per dataset) and `weight_sets=` ((W, num_obs), with
    `data=` only) and `varying=` (Q >= 1 coefficients that vary by group, for a model with kVaryingSlopes: it says how
    num_params splits into P, J and Q, and travels as wn_observations::num_varying).  The struct keeps the arrays it points into alive (`.arrays`); pass it with ctypes.byref."""
    if data is not None and datasets is not None:
        raise ValueError("data and datasets are mutually exclusive")
    varying = int(varying)
    if varying < 1:
        raise ValueError(f"varying must be at least 1 (the intercept), got {varying}")
    if data is None and datasets is None:
        if offset is not None or weights is not None or weight_sets is not None:
            raise ValueError("offset, weights and weight_sets need data or datasets")
        return None
    if weight_sets is not None and datasets is not None:
        raise ValueError("weight_sets is available with data only (the sets share one block of rows)")
    if weight_sets is not None and weights is not None:
        raise ValueError("weights and weight_sets are mutually exclusive")
    # columns of x of a flat data model (wn_model_data_columns): num_params, or num_params - 1 for a model with a scale
    # parameter.  An id that holds no flat data model gives num_params, and the engine then refuses the model (or the
    # pair (x, y) for a grouped model) with its own message.
    cols = int(lib.wn_model_data_columns(int(model), int(num_params), 0))
    cols = cols if cols >= 0 else int(num_params)
    # a grouped model's trailing log scales of the likelihood (hier_scale_glm.h): they say how num_params splits into P, J
    scales = max(0, int(lib.wn_model_num_scale_params(int(model))))
    obs = _ffi.Observations()
    if datasets is not None:
        x, y, group, J, offsets = _blocks(datasets, num_params, cols, varying, scales)
        obs.obs_offsets, obs.num_datasets = offsets.ctypes.data_as(_ffi._i64p), offsets.size - 1
    else:
        x, y, group, J = _block(data, num_params, cols, varying, scales)
        offsets = None
        obs.num_obs = y.size
    obs.num_varying = varying   # (the engine refuses varying > 1 for a model without varying slopes)
    obs.x, obs.y = x.ctypes.data_as(_ffi._dp), y.ctypes.data_as(_ffi._dp)
    if group is not None:
        obs.group, obs.num_groups = group.ctypes.data_as(_ffi._i32p), J
    sizes = [y.size] if offsets is None else list(np.diff(offsets))
    off = _row_terms("offset", offset, sizes, offsets is not None)
    wts = _row_terms("weights", weights, sizes, offsets is not None)
    if weight_sets is not None:
        wts = _f64(weight_sets)
        if wts.ndim != 2 or wts.shape[1] != y.size or wts.shape[0] < 1:
            raise ValueError(f"weight_sets must have shape (W, {y.size}), got {wts.shape}")
        obs.num_weight_sets = wts.shape[0]
    if off is not None:
        obs.offset = off.ctypes.data_as(_ffi._dp)
    if wts is not None:
        obs.weight = wts.ctypes.data_as(_ffi._dp)
    obs.arrays = (x, y, group, offsets, off, wts)
    return obs
