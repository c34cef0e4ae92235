"""Simulated replicates and posterior predictive checks from draws that stay on the device.

``replicate_draws`` hands y_rep ~ p(y | theta, x_n), one value per draw and row, back as ``MarkovChains`` of one dimension
per row (wn_engine_replicate_chains): ``.quantiles([0.05, 0.95])`` is a predictive interval of an OBSERVATION, not of its
mean.  ``posterior_predictive_check`` folds six statistics of every draw's replicate, and of the observations under the
same draw, where the draws live (wn_engine_replicate_check; walnuts_amd/csrc/wn_replicate.h states the reduction,
wn_devrand.h the samplers and their counter streams): no [draws, rows] matrix exists at any time."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import _ffi
from .engine import DeviceEngine
from .pointwise import _ones
from .predict import _rows_of
from .summary import MarkovChains

STATISTICS = ("sum", "sumsq", "min", "max", "zeros", "pearson")


@dataclass
class PredictiveCheck:
    """Per draw, arrays of shape [chains, max_len] (NaN beyond a chain's length): ``rep[name]`` of the replicate,
    ``obs[name]`` of the observations, for name in sum, sumsq, min, max, zeros, pearson and the derived mean and var (of
    the live rows, from the sums).  ``p_value[name]``: the share of valid draws with rep >= obs, one entry per dataset /
    weight set; ``invalid``: the draws per dataset / weight set left out because their replicate was not finite."""
    rep: Dict[str, np.ndarray]
    obs: Dict[str, np.ndarray]
    p_value: Dict[str, np.ndarray]
    invalid: np.ndarray


def _derived(stats, n):
    """mean and var over the n live rows (n [chains, 1]) from the sums"""
    with np.errstate(all="ignore"):
        mean = stats["sum"] / n
        var = np.where(n > 1, (stats["sumsq"] - stats["sum"] * mean) / (n - 1), np.nan)
    return mean, var


def _engine(lib, model, num_params, data, datasets, offset, weight_sets, cfg, lib_path, varying=1):
    ws = None if weight_sets is None else np.asarray(weight_sets, dtype=np.float64)
    if ws is not None and ws.ndim != 2:
        raise ValueError(f"weight_sets must have shape (W, num_obs), got {ws.shape}")
    G = ws.shape[0] if ws is not None else (len(datasets) if datasets is not None else 1)
    e = DeviceEngine(model, num_params, G, cfg=cfg, params=_ones(num_params), lib_path=lib_path, data=data,
                     datasets=datasets, offset=offset, weight_sets=None if ws is None or G == 1 else np.ones_like(ws),
                     varying=varying)
    return e, G, ws


def replicate_draws(model: int, chains, *, num_params: int, seed: int, data=None, datasets=None, offset=None,
                    weight_sets=None, block: int = 0, cfg=None, lib_path: Optional[str] = None,
                    varying: int = 1) -> MarkovChains:
    """y_rep per draw and row as MarkovChains on the device: k chains with the source chains' lengths and one dimension
    per row.  `data`, `datasets`, `offset`, `weight_sets`, `block` as for ``predict_draws`` (y is never read); a replicate
    depends on (seed, chain, draw, row) alone."""
    lib = _ffi.load_library(lib_path)
    if not isinstance(chains, MarkovChains):
        raise ValueError("chains must be a MarkovChains")
    if data is not None:
        data = _rows_of(lib, model, num_params, data)
    if datasets is not None:
        datasets = [_rows_of(lib, model, num_params, d) for d in datasets]
    e, _, _ = _engine(lib, model, num_params, data, datasets, offset, weight_sets, cfg, lib_path, varying)
    try:
        return e.replicate_chains(chains, seed, block=block)
    finally:
        e.close()


def posterior_predictive_check(model: int, chains, *, num_params: int, seed: int, data=None, datasets=None, offset=None,
                               weight_sets=None, rows=None, cfg=None, lib_path: Optional[str] = None,
                               varying: int = 1) -> PredictiveCheck:
    """Posterior predictive checks of a fit: `data=(x, y[, group])` (or `datasets=`) are the observations the check
    compares with, `chains` one MarkovChains of G * k chains (block g meets dataset / weight set g), `rows` a mask shaped
    as for ``predict`` of the rows that enter the statistics (default: all).  Weights are never applied."""
    lib = _ffi.load_library(lib_path)
    if not isinstance(chains, MarkovChains):
        raise ValueError("chains must be a MarkovChains")
    e, G, ws = _engine(lib, model, num_params, data, datasets, offset, weight_sets, cfg, lib_path, varying)
    try:
        mask = None if rows is None else np.asarray(rows) != 0
        if mask is not None and G == 1 and ws is not None:
            mask = mask.reshape(-1)
        rep, obs = e.replicate_check(chains, seed, mask)
        sizes = e._row_sizes
        shared = ws is not None
    finally:
        e.close()
    C = rep.shape[1]
    k = C // G
    # live rows per block
    if mask is None:
        live = [sizes[0] if shared else sizes[g] for g in range(G)]
    elif shared:
        live = [int(m.sum()) for m in mask.reshape(G, -1)]
    else:
        first = np.concatenate([[0], np.cumsum(sizes)])
        live = [int(mask[first[g]:first[g + 1]].sum()) for g in range(G)]
    n = np.repeat(np.asarray(live, dtype=np.float64), k)[:, None]
    out = []
    for stats in (rep, obs):
        d = {name: stats[s] for s, name in enumerate(STATISTICS)}
        d["mean"], d["var"] = _derived(d, n)
        out.append(d)
    rep_d, obs_d = out
    valid = ~np.isnan(rep_d["sum"])
    drawn = ~np.isnan(obs_d["sum"])   # (entries within the chains' lengths)
    p_value = {}
    for name in rep_d:
        p = np.full(G, np.nan)
        for g in range(G):
            v = valid[g * k:(g + 1) * k]
            if v.any():
                p[g] = float(np.mean(rep_d[name][g * k:(g + 1) * k][v] >= obs_d[name][g * k:(g + 1) * k][v]))
        p_value[name] = p
    invalid = np.array([int((drawn[g * k:(g + 1) * k] & ~valid[g * k:(g + 1) * k]).sum()) for g in range(G)])
    return PredictiveCheck(rep_d, obs_d, p_value, invalid)
