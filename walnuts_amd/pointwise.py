"""Scoring a fit: the log pointwise predictive density, WAIC and K-fold elpd from draws that stay on the device.

``log_predictive`` folds the pointwise log-likelihood l_n(theta) of a data model over the draws of ``MarkovChains``
(wn_engine_log_predictive; walnuts_amd/csrc/wn_pointwise.h states the fold) -- the draws of
``walnuts_device(..., keep_on_device=True)`` never reach the host.  ``kfold_elpd`` scores the K refits of
``walnuts_device(..., weight_sets=...)``: every row by the one fold that held it out."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from .engine import DeviceEngine
from .summary import MarkovChains


@dataclass
class PointwisePredictive:
    """Per row: lpd = log mean_t exp l_n(theta_t), mean and var = mean and sample variance of l_n(theta_t) over the
    draws, count = draws.  Rows that were not evaluated (masked out) hold NaN, NaN, NaN, 0 and take no part below."""
    lpd: np.ndarray
    mean: np.ndarray
    var: np.ndarray
    count: np.ndarray

    @property
    def evaluated(self) -> np.ndarray:
        return self.count > 0

    @property
    def elpd(self) -> float:
        """Sum of lpd over the evaluated rows: the log pointwise predictive density (held-out rows: the elpd)."""
        return float(np.sum(self.lpd[self.evaluated]))

    @property
    def se(self) -> float:
        """Standard error of elpd: sqrt(n * sample variance of lpd over the n evaluated rows)."""
        v = self.lpd[self.evaluated]
        return float(np.sqrt(v.size * np.var(v, ddof=1))) if v.size > 1 else float("nan")

    @property
    def p_waic(self) -> float:
        """Effective number of parameters of WAIC: the sum over rows of the variance of l_n over the draws."""
        return float(np.sum(self.var[self.evaluated]))

    @property
    def waic(self) -> float:
        """-2 (elpd - p_waic), on the deviance scale (meaningful when the rows were part of the fit)."""
        return -2.0 * (self.elpd - self.p_waic)


def _ones(num_params: int) -> np.ndarray:
    return np.ones(int(num_params))   # the likelihood does not read the prior


def log_predictive(model: int, chains, *, num_params: int, data=None, datasets=None, offset=None, weight_sets=None,
                   held_out=None, cfg=None, lib_path: Optional[str] = None, varying: int = 1) -> PointwisePredictive:
    """Score draws on rows: lpd, mean, var and count per row (PointwisePredictive).

    `chains`: one MarkovChains of G * k chains -- block g is scored on dataset g (`datasets=`), or on the shared rows as
    weight set g (`weight_sets=`), or all chains on `data=` -- or a sequence of G MarkovChains, one per block (the views
    of ``chain_blocks``).  The rows are given as for DeviceEngine (`data=`, `datasets=`, `offset=`); weights are never
    applied, `weight_sets=` (W, N) only says which block meets which rows.  `held_out`: a mask shaped like the output
    ([total rows]; [W, N] with weight sets) of the rows to evaluate; default every row, with `weight_sets=` the rows of
    weight 0 (`weight_sets == 0`: each fold scored on what it did not see).  `varying` as for DeviceEngine.  Model
    parameters are not needed."""
    if isinstance(chains, MarkovChains):
        blocks = None
    else:
        blocks = list(chains)
        if not blocks or not all(isinstance(b, MarkovChains) for b in blocks):
            raise ValueError("chains must be a MarkovChains or a sequence of MarkovChains (one per block)")
    if weight_sets is not None:
        ws = np.asarray(weight_sets, dtype=np.float64)
        if ws.ndim != 2:
            raise ValueError(f"weight_sets must have shape (W, num_obs), got {ws.shape}")
        if held_out is None:
            held_out = ws == 0
    G = ws.shape[0] if weight_sets is not None else (len(list(datasets)) if datasets is not None else 1)
    mask = None if held_out is None else np.asarray(held_out) != 0
    common = dict(cfg=cfg, params=_ones(num_params), lib_path=lib_path, varying=varying)
    if blocks is None:
        e = DeviceEngine(model, num_params, G, data=data, datasets=datasets, offset=offset,
                         weight_sets=None if weight_sets is None or G == 1 else np.ones_like(ws), **common)
        try:
            if mask is not None and G == 1 and weight_sets is not None:
                mask = mask.reshape(-1)
            out = e.log_predictive(chains, mask)
        finally:
            e.close()
        if weight_sets is not None and G == 1:
            out = tuple(a.reshape(1, -1) for a in out)
        return PointwisePredictive(*out)
    if len(blocks) != G:
        raise ValueError(f"{len(blocks)} blocks of chains for {G} datasets / weight sets")
    parts = []
    if datasets is not None:
        items = list(datasets)
        offs = [None] * G if offset is None else list(offset)
        sizes = [np.asarray(d[1]).shape[0] for d in items]
        first = np.concatenate([[0], np.cumsum(sizes)])
        if mask is not None and mask.shape != (first[-1],):
            raise ValueError(f"held_out must have shape ({first[-1]},), got {mask.shape}")
        for g in range(G):
            e = DeviceEngine(model, num_params, 1, data=items[g], offset=offs[g], **common)
            try:
                parts.append(e.log_predictive(blocks[g], None if mask is None else mask[first[g]:first[g + 1]]))
            finally:
                e.close()
        return PointwisePredictive(*(np.concatenate([p[i] for p in parts]) for i in range(4)))
    e = DeviceEngine(model, num_params, 1, data=data, offset=offset, **common)   # the shared rows, once
    try:
        if mask is not None and weight_sets is not None and mask.shape != ws.shape:
            raise ValueError(f"held_out must have shape {ws.shape}, got {mask.shape}")
        for g in range(G):
            m = None if mask is None else (mask[g] if weight_sets is not None else mask)
            parts.append(e.log_predictive(blocks[g], m))
    finally:
        e.close()
    if weight_sets is None:
        return PointwisePredictive(*parts[0])
    return PointwisePredictive(*(np.stack([p[i] for p in parts]) for i in range(4)))


def kfold_elpd(model: int, views, *, num_params: int, data, weight_sets, offset=None, cfg=None,
               lib_path: Optional[str] = None, varying: int = 1) -> PointwisePredictive:
    """K-fold cross-validation from the K refits of ``walnuts_device(..., weight_sets=weight_sets)``: `views` are the
    fits' draws (one MarkovChains of K * k chains, or the K views of ``chain_blocks``), and every row takes its lpd,
    mean, var and count from the ONE set that held it out (weight 0).  -> PointwisePredictive with [N] arrays; `.elpd`
    is the K-fold estimate of the expected log predictive density, `.se` its standard error.  ValueError unless every
    row is held out by exactly one set."""
    ws = np.asarray(weight_sets, dtype=np.float64)
    if ws.ndim != 2:
        raise ValueError(f"weight_sets must have shape (K, num_obs), got {ws.shape}")
    held = ws == 0
    times = held.sum(axis=0)
    if np.any(times != 1):
        bad = int(np.flatnonzero(times != 1)[0])
        raise ValueError(f"every row must be held out by exactly one weight set: row {bad} is held out by {int(times[bad])}")
    res = log_predictive(model, views, num_params=num_params, data=data, offset=offset, weight_sets=ws, held_out=held,
                         cfg=cfg, lib_path=lib_path, varying=varying)
    fold = np.argmax(held, axis=0)
    cols = np.arange(ws.shape[1])
    return PointwisePredictive(res.lpd[fold, cols], res.mean[fold, cols], res.var[fold, cols], res.count[fold, cols])


@dataclass
class PsisLoo:
    """Per row: elpd_loo = the PSIS estimate of log p(y_n | y_-n), pareto_k = the shape of the generalised Pareto fitted
    to the row's largest importance ratios (+inf: no tail could be fitted), ess = 1 / sum of the squared normalised
    weights -- draws are counted as independent: there is NO autocorrelation (r_eff) correction --, lpd = log mean
    exp l_n over the draws, count = draws.  Rows that were not evaluated (masked out) hold NaN and count 0 and take no
    part below."""
    elpd_loo: np.ndarray
    pareto_k: np.ndarray
    ess: np.ndarray
    lpd: np.ndarray
    count: np.ndarray

    @property
    def evaluated(self) -> np.ndarray:
        return self.count > 0

    @property
    def elpd(self) -> float:
        """Sum of elpd_loo over the evaluated rows: the expected log pointwise predictive density."""
        return float(np.sum(self.elpd_loo[self.evaluated]))

    @property
    def se(self) -> float:
        """Standard error of elpd: sqrt(n * sample variance of elpd_loo over the n evaluated rows)."""
        v = self.elpd_loo[self.evaluated]
        return float(np.sqrt(v.size * np.var(v, ddof=1))) if v.size > 1 else float("nan")

    @property
    def p_loo(self) -> float:
        """Effective number of parameters: the sum over rows of lpd - elpd_loo."""
        on = self.evaluated
        return float(np.sum(self.lpd[on] - self.elpd_loo[on]))

    @property
    def looic(self) -> float:
        """-2 elpd, on the deviance scale."""
        return -2.0 * self.elpd

    @property
    def num_bad(self) -> int:
        """Rows with pareto_k > 0.7: their elpd_loo is not to be trusted (refit without the row, or K-fold)."""
        return int(np.sum(self.pareto_k[self.evaluated] > 0.7))


def psis_loo(model: int, chains, *, num_params: int, data=None, datasets=None, offset=None, cfg=None,
             lib_path: Optional[str] = None, varying: int = 1, weight_sets=None) -> PsisLoo:
    """PSIS-LOO of a fit from draws that stay on the device: elpd_loo, pareto_k, ess, lpd and count per row (PsisLoo).

    `chains`, `data=`, `datasets=`, `offset=` and `varying` as for ``log_predictive``: one MarkovChains of G * k chains,
    block g scored on dataset g, or a sequence of G MarkovChains.  `weight_sets=` is refused: the weights of a weighted
    fit are not part of a row's importance ratio (for K refits use ``kfold_elpd``).  Model parameters are not needed."""
    if weight_sets is not None:
        raise ValueError("psis_loo takes no weight_sets: the weights of a weighted fit are not part of a row's importance "
                         "ratio, so the draws of such a fit cannot be reweighted to leave a row out (kfold_elpd scores K "
                         "refits)")
    if isinstance(chains, MarkovChains):
        blocks = None
    else:
        blocks = list(chains)
        if not blocks or not all(isinstance(b, MarkovChains) for b in blocks):
            raise ValueError("chains must be a MarkovChains or a sequence of MarkovChains (one per block)")
    G = len(list(datasets)) if datasets is not None else 1
    common = dict(cfg=cfg, params=_ones(num_params), lib_path=lib_path, varying=varying)
    if blocks is None:
        e = DeviceEngine(model, num_params, G, data=data, datasets=datasets, offset=offset, **common)
        try:
            return PsisLoo(*e.psis_loo(chains))
        finally:
            e.close()
    if len(blocks) != G:
        raise ValueError(f"{len(blocks)} blocks of chains for {G} datasets")
    items = [data] if datasets is None else list(datasets)
    offs = [offset] if datasets is None else ([None] * G if offset is None else list(offset))
    parts = []
    for g in range(G):
        e = DeviceEngine(model, num_params, 1, data=items[g], offset=offs[g], **common)
        try:
            parts.append(e.psis_loo(blocks[g]))
        finally:
            e.close()
    return PsisLoo(*(np.concatenate([p[i] for p in parts]) for i in range(5)))
