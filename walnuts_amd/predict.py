"""What a fit predicts: the linear predictor, the expected response and the predictive variance of new rows from draws
that stay on the device.

``predict`` folds (eta, E[y | theta, x_n], Var[y | theta, x_n]) of a data model over the draws of ``MarkovChains``
(wn_engine_predict_fold; walnuts_amd/csrc/wn_predict.h states the values and the fold); ``predict_draws`` hands the
per-draw values back as ``MarkovChains`` of one dimension per row, so credible bands, R-hat, ESS and MCSE of a prediction
are the summaries' (wn_engine_predict_chains).  The draws of ``walnuts_device(..., keep_on_device=True)`` never reach the
host."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _ffi
from .engine import DeviceEngine
from .pointwise import _ones
from .summary import MarkovChains


@dataclass
class Prediction:
    """Per row, over the draws: eta_mean / eta_var = mean and sample variance of the linear predictor, mean / mean_var =
    those of E[y | theta, x_n], noise_var = the mean of Var[y | theta, x_n], count = draws.  Rows that were not evaluated
    (masked out) hold NaN and count 0."""
    eta_mean: np.ndarray
    eta_var: np.ndarray
    mean: np.ndarray
    mean_var: np.ndarray
    noise_var: np.ndarray
    count: np.ndarray

    @property
    def var(self) -> np.ndarray:
        """The predictive variance of a new observation: E Var[y | theta] + Var E[y | theta] (the law of total variance)."""
        return self.noise_var + self.mean_var

    @property
    def sd(self) -> np.ndarray:
        return np.sqrt(self.var)

    @property
    def evaluated(self) -> np.ndarray:
        return self.count > 0


def _is_grouped_model(lib, model: int, num_params: int) -> bool:
    return lib.wn_model_data_columns(int(model), int(num_params), 0) < 0 <= lib.wn_model_data_columns(int(model), int(num_params), 1)


def _rows_of(lib, model: int, num_params: int, data):
    """`data` as DeviceEngine takes it: x_new, (x_new,), (x_new, group) for a grouped model, or the fit's own
    (x, y[, group]) pass; where y is absent it is zeros (which pass every model's data check; y is never read)."""
    if isinstance(data, np.ndarray) or not isinstance(data, (tuple, list)):
        data = (data,)
    parts = tuple(data)
    grouped = _is_grouped_model(lib, model, num_params)
    if len(parts) == 1 or (len(parts) == 2 and grouped):
        x = np.asarray(parts[0], dtype=np.float64)
        y = np.zeros(x.shape[0] if x.ndim >= 1 else 0)
        return (x, y) + parts[1:]
    return parts


def _as_blocks(chains):
    if isinstance(chains, MarkovChains):
        return None
    blocks = list(chains)
    if not blocks or not all(isinstance(b, MarkovChains) for b in blocks):
        raise ValueError("chains must be a MarkovChains or a sequence of MarkovChains (one per block)")
    return blocks


def predict(model: int, chains, *, num_params: int, data=None, datasets=None, offset=None, weight_sets=None, rows=None,
            cfg=None, lib_path: Optional[str] = None, varying: int = 1) -> Prediction:
    """Predict rows from draws: per row the moments of the linear predictor and of the expected response, and the mean
    noise variance (Prediction; `.var` / `.sd` are the predictive variance and standard deviation of a new observation).

    `data`: x_new, (x_new,), (x_new, group) for a grouped model, or the fit's own (x, y[, group]) -- y is never read.
    `chains`: one MarkovChains of G * k chains -- block g predicts dataset g (`datasets=`), or the shared rows as weight
    set g (`weight_sets=`, which only says how many blocks meet the rows: weights are never applied), or all chains
    `data=` -- or a sequence of G MarkovChains, one per block (the views of ``chain_blocks``).  `rows`: a mask shaped like
    the output ([total rows]; [W, N] with weight sets) of the rows to evaluate, default every row.  `varying` as for
    DeviceEngine.  Model parameters are not needed."""
    lib = _ffi.load_library(lib_path)
    blocks = _as_blocks(chains)
    if data is not None:
        data = _rows_of(lib, model, num_params, data)
    if datasets is not None:
        datasets = [_rows_of(lib, model, num_params, d) for d in datasets]
    ws = None
    if weight_sets is not None:
        ws = np.asarray(weight_sets, dtype=np.float64)
        if ws.ndim != 2:
            raise ValueError(f"weight_sets must have shape (W, num_obs), got {ws.shape}")
    G = ws.shape[0] if ws is not None else (len(datasets) if datasets is not None else 1)
    mask = None if rows is None else np.asarray(rows) != 0
    common = dict(cfg=cfg, params=_ones(num_params), lib_path=lib_path, varying=varying)
    if blocks is None:
        e = DeviceEngine(model, num_params, G, data=data, datasets=datasets, offset=offset,
                         weight_sets=None if ws is None or G == 1 else np.ones_like(ws), **common)
        try:
            if mask is not None and G == 1 and ws is not None:
                mask = mask.reshape(-1)
            out = e.predict_fold(chains, mask)
        finally:
            e.close()
        if ws is not None and G == 1:
            out = tuple(a.reshape(1, -1) for a in out)
        return Prediction(*out)
    if len(blocks) != G:
        raise ValueError(f"{len(blocks)} blocks of chains for {G} datasets / weight sets")
    parts = []
    if datasets is not None:
        offs = [None] * G if offset is None else list(offset)
        sizes = [np.asarray(d[1]).shape[0] for d in datasets]
        first = np.concatenate([[0], np.cumsum(sizes)])
        if mask is not None and mask.shape != (first[-1],):
            raise ValueError(f"rows must have shape ({first[-1]},), got {mask.shape}")
        for g in range(G):
            e = DeviceEngine(model, num_params, 1, data=datasets[g], offset=offs[g], **common)
            try:
                parts.append(e.predict_fold(blocks[g], None if mask is None else mask[first[g]:first[g + 1]]))
            finally:
                e.close()
        return Prediction(*(np.concatenate([p[i] for p in parts]) for i in range(6)))
    e = DeviceEngine(model, num_params, 1, data=data, offset=offset, **common)   # the shared rows, once
    try:
        if mask is not None and ws is not None and mask.shape != ws.shape:
            raise ValueError(f"rows must have shape {ws.shape}, got {mask.shape}")
        for g in range(G):
            parts.append(e.predict_fold(blocks[g], None if mask is None else (mask[g] if ws is not None else mask)))
    finally:
        e.close()
    if ws is None:
        return Prediction(*parts[0])
    return Prediction(*(np.stack([p[i] for p in parts]) for i in range(6)))


def predict_draws(model: int, chains, *, num_params: int, data=None, datasets=None, offset=None, weight_sets=None,
                  what: str = "mean", block: int = 0, cfg=None, lib_path: Optional[str] = None,
                  varying: int = 1) -> MarkovChains:
    """The predictions per draw as MarkovChains on the device: k chains with the source chains' lengths and one dimension
    per row, holding E[y | theta, x_n] (`what="mean"`) or the linear predictor (`what="eta"`) -- `.quantiles([0.05, 0.5,
    0.95])` is a credible band of the prediction, `.r_hat()`, `.effective_sample_size()` and
    `.monte_carlo_standard_error()` its diagnostics.  `data` as for ``predict``; `chains` one MarkovChains; with
    `datasets=` or `weight_sets=` it holds G * k chains and `block` selects the k chains (and rows) of one of them."""
    lib = _ffi.load_library(lib_path)
    if not isinstance(chains, MarkovChains):
        raise ValueError("chains must be a MarkovChains")
    if data is not None:
        data = _rows_of(lib, model, num_params, data)
    if datasets is not None:
        datasets = [_rows_of(lib, model, num_params, d) for d in datasets]
    ws = None if weight_sets is None else np.asarray(weight_sets, dtype=np.float64)
    G = ws.shape[0] if ws is not None else (len(datasets) if datasets is not None else 1)
    e = DeviceEngine(model, num_params, G, cfg=cfg, params=_ones(num_params), lib_path=lib_path, data=data,
                     datasets=datasets, offset=offset, weight_sets=None if ws is None or G == 1 else np.ones_like(ws),
                     varying=varying)
    try:
        return e.predict_chains(chains, block=block, what=what)
    finally:
        e.close()
