"""Batched engine handle: the per-transition verbs of include/walnuts_hip.h.

``DeviceEngine`` advances ALL chains by one transition per call; its methods are named after the reference
objects they batch: ``warmup_step`` = ``AdaptiveWalnuts::operator()`` (adaptive_walnuts.hpp:234-251),
``freeze`` = ``AdaptiveWalnuts::sampler()`` (:263-271), ``sample_step`` = ``WalnutsSampler::operator()``
(walnuts.hpp:682-692); the init methods follow ``InitConfigBuilder`` (config.hpp:195-484).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _ffi
from ._observations import _f64, observations
from .summary import MarkovChains

MODEL_STD_NORMAL, MODEL_DIAG_NORMAL, MODEL_FUNNEL, MODEL_RW1 = 0, 1, 2, 3
# models conditioned on data (walnuts_amd/csrc/models/glm.h): params = the prior variances, data = (x, y)
MODEL_LINEAR_REGRESSION, MODEL_LOGISTIC_REGRESSION = 4, 5
# hierarchical regression with varying intercepts by group (walnuts_amd/csrc/models/hier_glm.h): theta = [beta (P) |
# group effects (J) | log tau], params = [prior variances of beta (P) | 1 (J, reserved) | sigma_tau], data = (x, y, group)
# with x of P = num_params - J - 1 columns and group in [0, J); non-centered (u = z) and centered (u = a)
# (ids 6-14 stay free for models of one's own: the out-of-tree examples and tests take ids there)
MODEL_HIER_LINEAR_REGRESSION, MODEL_HIER_LOGISTIC_REGRESSION = 15, 16
MODEL_HIER_LINEAR_REGRESSION_CENTERED, MODEL_HIER_LOGISTIC_REGRESSION_CENTERED = 17, 18
# count models and an estimated noise level (walnuts_amd/csrc/models/glm.h, glm_scale.h), ids 24-28 (19-23 stay free as
# well).  poisson_regression: as the linear and logistic models.  neg_binomial_regression (NB2, overdispersion
# kappa = exp(s)) and linear_regression_sigma (noise sigma = exp(s)): theta = [beta (P) | s], params = [prior variances
# of beta (P) | sigma_0, the half-normal scale of exp(s)], data = (x, y) with x of P = num_params - 1 columns.
# hier_poisson_regression(_centered): as MODEL_HIER_*, with Poisson counts.
MODEL_POISSON_REGRESSION, MODEL_NEG_BINOMIAL_REGRESSION, MODEL_LINEAR_REGRESSION_SIGMA = 24, 25, 26
MODEL_HIER_POISSON_REGRESSION, MODEL_HIER_POISSON_REGRESSION_CENTERED = 27, 28
# hierarchical regression with varying intercepts and slopes by group, non-centered
# (walnuts_amd/csrc/models/hier_slopes_glm.h): `varying=Q` coefficients vary by group, the intercept and the slopes of
# the first Q - 1 columns of x, with independent scales.  theta = [beta (P) | u_0 (J) | .. | u_{Q-1} (J) | log tau_0 ..
# log tau_{Q-1}], params = [prior variances of beta (P) | 1 (Q J, reserved) | sigma_0 .. sigma_{Q-1}], data = (x, y,
# group) with P = num_params - Q (J + 1) columns; at varying=1 they are MODEL_HIER_*, bit for bit
# (ids 29-31 stay free: the tests place run-time models of their own there)
MODEL_HIER_LINEAR_REGRESSION_SLOPES, MODEL_HIER_LOGISTIC_REGRESSION_SLOPES = 32, 33
MODEL_HIER_POISSON_REGRESSION_SLOPES = 34
# hierarchical regression with varying intercepts by group and an estimated scale
# (walnuts_amd/csrc/models/hier_scale_glm.h): hier_linear_regression_sigma(_centered) is the multilevel normal model
# y ~ N(x . beta + a_g, sigma) with sigma = exp(s) unknown.  theta = [beta (P) | group effects (J) | log tau | s],
# params = [prior variances of beta (P) | 1 (J, reserved) | sigma_tau | sigma_0, the half-normal scale of exp(s)],
# data = (x, y, group) with x of P = num_params - J - 2 columns
MODEL_HIER_LINEAR_REGRESSION_SIGMA, MODEL_HIER_LINEAR_REGRESSION_SIGMA_CENTERED = 35, 36
# varying intercepts and slopes by group AND an estimated noise level, non-centered
# (walnuts_amd/csrc/models/hier_slopes_scale_glm.h): y ~ x + (1 + x_0 + .. | g) with sigma = exp(s) unknown, `varying=Q`
# as for MODEL_HIER_*_SLOPES.  theta = [beta (P) | u_0 (J) | .. | u_{Q-1} (J) | log tau_0 .. log tau_{Q-1} | s], params =
# [prior variances of beta (P) | 1 (Q J, reserved) | sigma_0 .. sigma_{Q-1} | sigma_0 of exp(s)], data = (x, y, group)
# with P = num_params - Q (J + 1) - 1 columns; at varying=1 it is MODEL_HIER_LINEAR_REGRESSION_SIGMA, bit for bit
# (ids 37 and 38 stay reserved for grouped negative binomial models, 39 stays free)
MODEL_HIER_LINEAR_REGRESSION_SLOPES_SIGMA = 40
_dp = _ffi._dp


def default_config(lib_path: Optional[str] = None, **overrides) -> _ffi.Config:
    cfg = _ffi.Config()
    _ffi.load_library(lib_path).wn_default_config(C.byref(cfg))
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def model_id(name: str, lib_path: Optional[str] = None) -> int:
    """Id of the device model registered under `name` (see walnuts_amd/csrc/wn_model_api.h); ValueError if none."""
    i = _ffi.load_library(lib_path).wn_model_id(name.encode())
    if i < 0:
        raise ValueError(f"no device model named {name!r} in this build of the library")
    return i


def stream_version(lib_path: Optional[str] = None) -> int:
    """Version of the library's counter-based random streams (wn_stream_version): same seed + same version = same run."""
    return int(_ffi.load_library(lib_path).wn_stream_version())


class DeviceEngine:
    def __init__(self, model: int, dim: int, num_chains: int, cfg: Optional[_ffi.Config] = None,
                 params: Optional[np.ndarray] = None, lib_path: Optional[str] = None, data=None, datasets=None,
                 offset=None, weights=None, weight_sets=None, varying: int = 1):
        """`data=(x, y)`: the observations of a model conditioned on data (wn_model_api.h kUsesData), x of shape
        (num_obs, dim) and y of shape (num_obs,); copied to the device once.  `data=(x, y, group)` for a grouped model
        (kUsesGroups: MODEL_HIER_*): x of shape (num_obs, P), y and the integer group of shape (num_obs,), groups in
        [0, J) with J = dim - P - 1 (J = dim - P - 2 for MODEL_HIER_LINEAR_REGRESSION_SIGMA*, whose theta ends with log tau
        and the log scale s).  `varying=Q` (MODEL_HIER_*_SLOPES, 1 <= Q <= 8, Q - 1 <= P): the intercept and
        the slopes of the first Q - 1 columns of x vary by group, J = (dim - P) / Q - 1 (J = (dim - P - 1) / Q - 1 for
        MODEL_HIER_LINEAR_REGRESSION_SLOPES_SIGMA, whose theta ends with the log scale s).  A model with a scale parameter
        (MODEL_NEG_BINOMIAL_REGRESSION, MODEL_LINEAR_REGRESSION_SIGMA) takes x of shape (num_obs, dim - 1): its last
        coordinate is s, not a column of x.  The count models (MODEL_POISSON_REGRESSION, MODEL_NEG_BINOMIAL_REGRESSION,
        MODEL_HIER_POISSON_REGRESSION*) need every y to be a finite non-negative integer.

        `datasets=[(x0, y0), (x1, y1), ...]` instead: G datasets of the same model and prior (sizes may differ), fitted
        side by side (wn_observations::obs_offsets).  num_chains must be a multiple k of G; chains [g*k, (g+1)*k)
        are conditioned on dataset g and evolve exactly as chains 0..k-1 of an engine built with data=(xg, yg) and
        seeded with chain_offset = g*k.  Per-dataset statistics: rhat_per_dataset(), warmup_spread_per_dataset();
        init_masses_from_grad(average=True) averages over each dataset's chains.  A grouped model takes triples
        [(x0, y0, g0), ...] with the same number of columns in every x.

        `offset=` and `weights=` (every built-in data model): per-row terms of shape (num_obs,), eta_n = x_n . beta +
        offset_n and logp = prior + sum_n weights_n * ll_n -- the exposure log E of a count model; frequency or
        importance weights >= 0; binomial counts as weights=m, y=k/m (with weights the logistic models take y in
        [0, 1]).  A row of weight 0 contributes exactly nothing.  With `datasets=` each is a sequence with one array (or
        None) per dataset.  An engine that carries weights evaluates EVERY dataset in the weighted order of operations:
        a dataset whose entry is None gets weights of 1 and gives the bits of a standalone engine built with
        weights=np.ones(num_obs), which differ in the last place from those of an engine built without weights.

        `weight_sets=` (with `data=` only): a (W, num_obs) array, W weight vectors over the one shared block of rows
        -- K-fold refits, the bootstrap.  num_chains must be a multiple k of W; chains [g*k, (g+1)*k) use set g and
        evolve exactly as chains 0..k-1 of an engine built with weights=weight_sets[g] and seeded with chain_offset =
        g*k.  The sets are the engine's datasets: num_datasets == W and the per-dataset statistics are per set.  W == 1
        is one weight vector, the same engine as weights=weight_sets[0] (num_datasets == 1)."""
        self.lib = _ffi.load_library(lib_path)
        self.cfg = cfg if cfg is not None else default_config(lib_path)
        self.C, self.D = int(num_chains), int(dim)
        p = None if params is None else _f64(params)
        if p is not None and p.size != dim:
            raise ValueError("model params must have num_params entries")
        h, err = C.c_void_p(), C.c_void_p()
        pp = None if p is None else p.ctypes.data_as(_dp)
        obs = observations(self.lib, model, self.D, data, datasets, offset, weights, weight_sets, varying)
        # (one weight set is one weight vector: such an engine holds no datasets)
        self._several = datasets is not None or (obs is not None and obs.num_weight_sets > 1)
        # rows per dataset (the pointwise entry points size their outputs with them)
        self._row_sizes = None if obs is None else (
            [int(obs.num_obs)] if datasets is None else [int(n) for n in np.diff(obs.arrays[3])])
        self._weight_sets = obs is not None and obs.num_weight_sets > 1
        if obs is None:
            rc = self.lib.wn_engine_create(C.byref(h), model, dim, pp, num_chains, C.byref(self.cfg), C.byref(err))
        else:
            rc = self.lib.wn_engine_create_observed(C.byref(h), model, dim, pp, C.byref(obs), num_chains,
                                                    C.byref(self.cfg), C.byref(err))
        _ffi.check(self.lib, rc, err)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.wn_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, fn, *args):
        err = C.c_void_p()
        _ffi.check(self.lib, fn(self.h, *args, C.byref(err)), err)

    # ---- InitConfigBuilder
    def set_positions(self, pos):
        a = _f64(pos).reshape(self.C, self.D)
        self._call(self.lib.wn_engine_set_positions, a.ctypes.data_as(_dp))

    def set_masses(self, mass):
        a = _f64(mass).reshape(self.C, self.D)
        self._call(self.lib.wn_engine_set_masses, a.ctypes.data_as(_dp))

    def set_step_sizes(self, steps):
        a = _f64(np.broadcast_to(np.asarray(steps, dtype=np.float64), (self.C,)))
        self._call(self.lib.wn_engine_set_step_sizes, a.ctypes.data_as(_dp))

    def init_positions(self, seed: int, chain_offset: int, scale: float):
        self._call(self.lib.wn_engine_init_positions, seed, chain_offset, scale)

    def init_masses_from_grad(self, smoothing: float, average: bool = False):
        """InitConfigBuilder::masses(logp_grad, smoothing, average_masses) (config.hpp:360-382)."""
        self._call(self.lib.wn_engine_init_masses_from_grad, smoothing)
        if average:
            self.average_masses()

    def average_masses(self):
        """Every chain's masses become their geometric mean over the chains (config.hpp:371-380) -- over the chains of
        its own dataset on an engine built with `datasets=` (wn_engine_average_masses_datasets)."""
        self._call(self.lib.wn_engine_average_masses_datasets if self._several else self.lib.wn_engine_average_masses)

    def adapt_step(self, seed: int, chain_offset: int = 0):
        self._call(self.lib.wn_engine_adapt_step, seed, chain_offset)

    def adapt_step_with_normals(self, normals):
        a = _f64(normals).reshape(self.C, self.D)
        self._call(self.lib.wn_engine_adapt_step_with_normals, a.ctypes.data_as(_dp))

    def seed_chains(self, seed: int, chain_offset: int = 0):
        self._call(self.lib.wn_engine_seed, seed, chain_offset)

    def seed_reference_streams(self, seed: int):
        """Parity mode: the reference's mt19937_64(seed_seq{seed, m+1}) + libstdc++ distributions, generated on
        the host for every following transition (api.hpp:46-51, util.hpp:78-162)."""
        self._call(self.lib.wn_engine_seed_reference_streams, seed)

    def set_variates(self, normals, uniforms):
        z = _f64(normals).reshape(self.C, self.D)
        u = _f64(uniforms).reshape(self.C, -1)
        self._call(self.lib.wn_engine_set_variates, z.ctypes.data_as(_dp), u.ctypes.data_as(_dp), u.shape[1])

    # ---- transitions.  draws_ptr: integer device address (e.g. torch tensor .data_ptr()) or None
    def warmup_step(self, draws_ptr: Optional[int] = None, stride: int = 0):
        self._call(self.lib.wn_engine_warmup_step, C.c_void_p(draws_ptr), stride)

    def freeze(self):
        self._call(self.lib.wn_engine_freeze)

    def sample_step(self, draws_ptr: Optional[int] = None, stride: int = 0):
        self._call(self.lib.wn_engine_sample_step, C.c_void_p(draws_ptr), stride)

    def warmup_steps(self, transitions: int, draws_ptr: Optional[int] = None, stride: int = 0, transition_stride: int = 0):
        """`transitions` warmup transitions of every chain in one launch (same bits as as many warmup_step calls);
        chain c's k-th position at draws_ptr + c*stride + k*transition_stride doubles."""
        self._call(self.lib.wn_engine_warmup_steps, int(transitions), C.c_void_p(draws_ptr), stride, transition_stride)

    def sample_steps(self, transitions: int, draws_ptr: Optional[int] = None, stride: int = 0, transition_stride: int = 0):
        """`transitions` sampling transitions of every chain in one launch (same bits as as many sample_step calls)."""
        self._call(self.lib.wn_engine_sample_steps, int(transitions), C.c_void_p(draws_ptr), stride, transition_stride)

    def synchronize(self):
        self._call(self.lib.wn_engine_synchronize)

    def check(self):
        """Raise if any chain's last transition could not complete on the device."""
        self._call(self.lib.wn_engine_check)

    def logp_grad(self, theta):
        """The model's (log density [C], gradient [C, D]) at positions theta [C, D] (wn_engine_eval), in the engine's
        arithmetic mode; no chain state is read or changed."""
        th = _f64(theta).reshape(self.C, self.D)
        lp = np.empty(self.C)
        g = np.empty((self.C, self.D))
        self._call(self.lib.wn_engine_eval, th.ctypes.data_as(_dp), lp.ctypes.data_as(_dp), g.ctypes.data_as(_dp))
        return lp, g

    def _rows(self, dataset=None):
        """Rows of dataset `dataset`; None: of every output row (all datasets, or W * N with weight sets)."""
        sizes = self._row_sizes
        if sizes is None:   # an engine without data: the library refuses the call (a `config` error naming the model)
            return 1 if dataset is not None else (1,)
        if dataset is None:
            return (self.num_datasets * sizes[0],) if self._weight_sets else (int(sum(sizes)),)
        if not 0 <= dataset < (1 if self._weight_sets else len(sizes)):
            raise ValueError("weight sets share one block of rows: dataset must be 0" if self._weight_sets
                             else "dataset must be in [0, num_datasets)")
        return sizes[dataset]

    def log_lik(self, theta, dataset: int = 0):
        """The POINTWISE log-likelihood [T, N] of dataset `dataset` at positions theta [T, D] (wn_engine_log_lik): entry
        [t, n] is the full log density of row n under theta[t] -- constants included, the prior not, offsets and groups
        applied, weights IGNORED -- in the engine's arithmetic mode.  T is independent of the engine's num_chains; with
        weight sets the rows are the one shared block (dataset 0).  No chain state is read or changed."""
        th = _f64(theta).reshape(-1, self.D)
        out = np.empty((th.shape[0], self._rows(int(dataset))))
        self._call(self.lib.wn_engine_log_lik, th.ctypes.data_as(_dp), th.shape[0], int(dataset), out.ctypes.data_as(_dp))
        return out

    def log_predictive(self, chains, row_mask=None):
        """(lpd, mean, var, count) per row from draws that stay on the device (wn_engine_log_predictive): `chains` is a
        MarkovChains of G * k chains, G = num_datasets; block g is scored on dataset g's rows (weight sets: on the shared
        rows, as set g).  lpd = log mean exp l_n over the block's draws, mean / var the moments of l_n, count the draws.
        Arrays of shape [total rows], or [W, N] with weight sets; `row_mask` of that shape (nonzero = evaluate) or None:
        a masked row is not evaluated and gives NaN, NaN, NaN, 0.  walnuts_amd.log_predictive wraps this."""
        shape = self._rows() if not self._weight_sets else (self.num_datasets, self._row_sizes[0])
        mask = None
        if row_mask is not None:
            mask = np.ascontiguousarray(np.asarray(row_mask) != 0, dtype=np.uint8)
            if mask.shape != tuple(shape):
                raise ValueError(f"row_mask must have shape {tuple(shape)}, got {mask.shape}")
        lpd, mean, var = (np.empty(shape) for _ in range(3))
        count = np.empty(shape, dtype=np.int64)
        self._call(self.lib.wn_engine_log_predictive, chains._h,
                   None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), lpd.ctypes.data_as(_dp),
                   mean.ctypes.data_as(_dp), var.ctypes.data_as(_dp), count.ctypes.data_as(_ffi._i64p))
        return lpd, mean, var, count

    def psis_loo(self, chains, row_mask=None, *, workspace_bytes: int = 0):
        """(elpd_loo, pareto_k, ess, lpd, count) per row from draws that stay on the device (wn_engine_psis_loo):
        leave-one-out cross-validation by Pareto-smoothed importance sampling.  Blocks, shapes and `row_mask` as for
        log_predictive; a masked row gives NaN four times and count 0.  pareto_k is +inf where no tail could be fitted;
        ess is 1 / sum of the squared normalised weights, with no autocorrelation correction.  `workspace_bytes`: the
        device memory the rows-by-draws matrix may take at a time (0: 1 GiB); it changes no value.
        walnuts_amd.psis_loo wraps this."""
        shape = self._rows() if not self._weight_sets else (self.num_datasets, self._row_sizes[0])
        mask = None
        if row_mask is not None:
            mask = np.ascontiguousarray(np.asarray(row_mask) != 0, dtype=np.uint8)
            if mask.shape != tuple(shape):
                raise ValueError(f"row_mask must have shape {tuple(shape)}, got {mask.shape}")
        elpd, k, ess, lpd = (np.empty(shape) for _ in range(4))
        count = np.empty(shape, dtype=np.int64)
        self._call(self.lib.wn_engine_psis_loo, chains._h,
                   None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), int(workspace_bytes),
                   elpd.ctypes.data_as(_dp), k.ctypes.data_as(_dp), ess.ctypes.data_as(_dp), lpd.ctypes.data_as(_dp),
                   count.ctypes.data_as(_ffi._i64p))
        return elpd, k, ess, lpd, count

    def _psis_matrix(self, chains, num_draws: int, dataset: int = 0):
        """(tests) stage 1 of psis_loo alone: the [rows, num_draws] matrix of block `dataset`, whose chains hold
        num_draws draws (wn_internal_psis_matrix)"""
        out = np.empty((self._rows(int(dataset)), int(num_draws)))
        self._call(self.lib.wn_internal_psis_matrix, chains._h, int(dataset), int(num_draws), out.ctypes.data_as(_dp))
        return out

    def predict(self, theta, dataset: int = 0):
        """(eta, mean, var), each [T, N]: the linear predictor, E[y | theta, x_n] and Var[y | theta, x_n] of every row of
        dataset `dataset` at positions theta [T, D] (wn_engine_predict), in the engine's arithmetic mode.  eta is formed
        as the likelihood forms it (groups and offsets applied); y and weights are never read, so a logistic row with
        binomial weights is predicted per trial.  No chain state is read or changed."""
        th = _f64(theta).reshape(-1, self.D)
        eta, mean, var = (np.empty((th.shape[0], self._rows(int(dataset)))) for _ in range(3))
        self._call(self.lib.wn_engine_predict, th.ctypes.data_as(_dp), th.shape[0], int(dataset), eta.ctypes.data_as(_dp),
                   mean.ctypes.data_as(_dp), var.ctypes.data_as(_dp))
        return eta, mean, var

    def predict_fold(self, chains, row_mask=None):
        """(eta_mean, eta_var, mean, mean_var, noise_var, count) per row from draws that stay on the device
        (wn_engine_predict_fold): the moments of eta and of E[y | theta, x_n] over the draws of the row's block, the mean
        of Var[y | theta, x_n], and the number of draws.  Blocks, shapes and `row_mask` as for log_predictive; a masked
        row is not evaluated and gives NaN everywhere and count 0.  walnuts_amd.predict wraps this."""
        shape = self._rows() if not self._weight_sets else (self.num_datasets, self._row_sizes[0])
        mask = None
        if row_mask is not None:
            mask = np.ascontiguousarray(np.asarray(row_mask) != 0, dtype=np.uint8)
            if mask.shape != tuple(shape):
                raise ValueError(f"row_mask must have shape {tuple(shape)}, got {mask.shape}")
        out = tuple(np.empty(shape) for _ in range(5))
        count = np.empty(shape, dtype=np.int64)
        self._call(self.lib.wn_engine_predict_fold, chains._h,
                   None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                   *(a.ctypes.data_as(_dp) for a in out), count.ctypes.data_as(_ffi._i64p))
        return out + (count,)

    def predict_chains(self, chains, block: int = 0, what: str = "mean"):
        """The predictions of the k chains of dataset / weight set `block`, one value per draw and row, as MarkovChains
        of their own on the device (wn_engine_predict_chains): `what` is "eta" (the linear predictor) or "mean"
        (E[y | theta, x_n]); the result has one dimension per row and the source chains' lengths, so .quantiles(),
        .r_hat(), .effective_sample_size() and the rest give credible bands and diagnostics of a prediction."""
        codes = {"eta": 0, "mean": 1}
        if what not in codes:
            raise ValueError(f'what must be "eta" or "mean", got {what!r}')
        h = C.c_void_p()
        self._call(self.lib.wn_engine_predict_chains, chains._h, int(block), codes[what], C.byref(h))
        return MarkovChains(h, self.lib)

    def replicate(self, theta, seed: int, dataset: int = 0):
        """Simulated replicates y_rep [T, N] ~ p(y | theta[t], x_n) of every row of dataset `dataset` (wn_engine_replicate):
        what predict() describes, drawn on the device from counter streams keyed by (seed, t, row) -- position t is
        chain t, draw 0 of replicate_chains' layout.  The engine's own random streams and chain state are untouched."""
        th = _f64(theta).reshape(-1, self.D)
        out = np.empty((th.shape[0], self._rows(int(dataset))))
        self._call(self.lib.wn_engine_replicate, th.ctypes.data_as(_dp), th.shape[0], int(dataset), int(seed),
                   out.ctypes.data_as(_dp))
        return out

    def replicate_chains(self, chains, seed: int, block: int = 0):
        """One replicate per draw and row of the k chains of dataset / weight set `block`, as MarkovChains of their own on
        the device (wn_engine_replicate_chains): .quantiles() is a predictive interval of an OBSERVATION."""
        h = C.c_void_p()
        self._call(self.lib.wn_engine_replicate_chains, chains._h, int(block), int(seed), C.byref(h))
        return MarkovChains(h, self.lib)

    def replicate_check(self, chains, seed: int, row_mask=None):
        """(stat_rep, stat_obs), each [6, chains, max_len]: per draw the statistics sum, sum of squares, min, max, number
        of zeros and Pearson discrepancy over the live rows, of the draw's replicate and of the engine's observations
        (wn_engine_replicate_check); NaN beyond a chain's length.  `row_mask` as for predict_fold.
        walnuts_amd.posterior_predictive_check wraps this."""
        shape = self._rows() if not self._weight_sets else (self.num_datasets, self._row_sizes[0])
        mask = None
        if row_mask is not None:
            mask = np.ascontiguousarray(np.asarray(row_mask) != 0, dtype=np.uint8)
            if mask.shape != tuple(shape):
                raise ValueError(f"row_mask must have shape {tuple(shape)}, got {mask.shape}")
        out = tuple(np.full((6, chains.num_chains(), chains.max_chain_size()), np.nan) for _ in range(2))
        self._call(self.lib.wn_engine_replicate_check, chains._h,
                   None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_uint8)), int(seed),
                   *(a.ctypes.data_as(_dp) for a in out))
        return out

    # ---- state
    def _get(self, fn, shape, dtype=np.float64, ptr=_dp):
        out = np.empty(shape, dtype=dtype)
        self._call(fn, out.ctypes.data_as(ptr))
        return out

    def positions(self):
        return self._get(self.lib.wn_engine_get_positions, (self.C, self.D))

    def masses(self):
        return self._get(self.lib.wn_engine_get_masses, (self.C, self.D))

    def inv_mass(self):
        return self._get(self.lib.wn_engine_get_inv_mass, (self.C, self.D))

    def step_sizes(self):
        return self._get(self.lib.wn_engine_get_step_sizes, (self.C,))

    def logp(self):
        return self._get(self.lib.wn_engine_get_logp, (self.C,))

    def adam(self):
        return self._get(self.lib.wn_engine_get_adam, (self.C, 6))

    def min_micro(self):
        return self._get(self.lib.wn_engine_get_min_micro, (self.C,), np.int32, _ffi._i32p)

    def depths(self):
        return self._get(self.lib.wn_engine_get_depths, (self.C,), np.int32, _ffi._i32p)

    def grad_evals(self):
        return self._get(self.lib.wn_engine_get_grad_evals, (self.C,), np.int64, _ffi._i64p)

    def failed_extensions(self):
        """Per chain: 1 if an extension of the last transition failed (a leaf's energy error above the bound at every
        step size -- where a model returning non-finite values ends up; the device counterpart of the reference's
        on_logp_exception events, util.hpp:336-346 -- or a failed reversibility check)."""
        return self._get(self.lib.wn_engine_get_failed_extensions, (self.C,), np.int32, _ffi._i32p)

    def rng_draws(self):
        return self._get(self.lib.wn_engine_get_rng_draws, (self.C,), np.int32, _ffi._i32p)

    def estimator(self):
        dm, ds, sm, ss = (np.empty((self.C, self.D)) for _ in range(4))
        w = np.empty((self.C, 2))
        self._call(self.lib.wn_engine_get_estimator, *(x.ctypes.data_as(_dp) for x in (dm, ds, sm, ss, w)))
        return dict(draw_mean=dm, draw_ssd=ds, score_mean=sm, score_ssd=ss, weights=w)

    def total_grad_evals(self) -> int:
        v = C.c_int64()
        self._call(self.lib.wn_engine_total_grad_evals, C.byref(v))
        return v.value

    def last_kernel_ms(self) -> float:
        v = C.c_float()
        self._call(self.lib.wn_engine_last_kernel_ms, C.byref(v))
        return v.value

    def rhat(self) -> float:
        """R-hat of the log density over the sampling draws so far (sampler.hpp:132-145)."""
        v = C.c_double()
        self._call(self.lib.wn_engine_rhat, C.cast(C.byref(v), _dp))
        return v.value

    def lp_sums(self):
        """Stage 1 of R-hat for a multi-GPU driver: (sum of chain means, sum of chain sample variances, chains) of the
        log density -- all-reduce SUM."""
        out = np.zeros(3)
        self._call(self.lib.wn_engine_lp_sums, out.ctypes.data_as(_dp))
        return out

    def lp_sq_dev(self, mean_of_means: float) -> float:
        """Stage 2: sum over this engine's chains of (chain mean - mean of means)^2 -- all-reduce SUM."""
        v = C.c_double()
        self._call(self.lib.wn_engine_lp_sq_dev, mean_of_means, C.cast(C.byref(v), _dp))
        return v.value

    def warmup_spread(self):
        """(max rel. step-size distance, max rel. mass distance) from the chains' geometric means
        (adapt.hpp:193-221)."""
        a, b = C.c_double(), C.c_double()
        self._call(self.lib.wn_engine_warmup_spread, C.cast(C.byref(a), _dp), C.cast(C.byref(b), _dp))
        return a.value, b.value

    @property
    def num_datasets(self) -> int:
        """Datasets the engine holds (1 unless built with `datasets=`)."""
        return int(self.lib.wn_engine_num_datasets(self.h))

    def rhat_per_dataset(self) -> np.ndarray:
        """[G] R-hat of the log density per dataset: entry g is what rhat() returns on a standalone engine of dataset
        g's chains (wn_engine_rhat_datasets)."""
        return self._get(self.lib.wn_engine_rhat_datasets, (self.num_datasets,))

    def warmup_spread_per_dataset(self):
        """(step [G], mass [G]): warmup_spread() of each dataset's chains (wn_engine_warmup_spread_datasets)."""
        step, mass = np.empty(self.num_datasets), np.empty(self.num_datasets)
        self._call(self.lib.wn_engine_warmup_spread_datasets, step.ctypes.data_as(_dp), mass.ctypes.data_as(_dp))
        return step, mass

    def warmup_sums(self):
        """Stage 1 of the warmup statistic for a multi-GPU driver: (sum over this engine's chains of log step,
        [D] sums of log mass) -- all-reduce SUM these D+1 doubles."""
        s = C.c_double()
        col = np.zeros(self.D)
        self._call(self.lib.wn_engine_warmup_sums, C.cast(C.byref(s), _dp), col.ctypes.data_as(_dp))
        return s.value, col

    def warmup_max_rel(self, sum_log_step: float, colsum_log_mass, total_chains: int):
        """Stage 2: this engine's (max rel. step distance, max rel. mass distance) from the geometric means over
        ALL `total_chains` chains -- all-reduce MAX."""
        col = _f64(colsum_log_mass).reshape(self.D)
        a, b = C.c_double(), C.c_double()
        self._call(self.lib.wn_engine_warmup_max_rel, sum_log_step, col.ctypes.data_as(_dp), total_chains,
                   C.cast(C.byref(a), _dp), C.cast(C.byref(b), _dp))
        return a.value, b.value

    def region_begin(self):
        """Start of a timed region of launches (one pair of HIP events around all of them)."""
        self._call(self.lib.wn_engine_region_begin)

    def region_ms(self):
        """-> (elapsed ms since region_begin on the engine's stream, transition launches in between)."""
        ms, n = C.c_float(), C.c_int()
        self._call(self.lib.wn_engine_region_ms, C.byref(ms), C.byref(n))
        return float(ms.value), int(n.value)

    def timing_reset(self):
        self._call(self.lib.wn_engine_timing_reset)

    def kernel_times_ms(self, max_launches: int = 1 << 16) -> np.ndarray:
        buf = np.zeros(max_launches, dtype=np.float32)
        n = C.c_int()
        self._call(self.lib.wn_engine_kernel_times, buf.ctypes.data_as(C.POINTER(C.c_float)), max_launches,
                   C.byref(n))
        return buf[: min(n.value, max_launches)].astype(np.float64)

    def set_stream(self, stream_handle: int):
        self._call(self.lib.wn_engine_set_stream, C.c_void_p(stream_handle))

    def wait_stream(self, stream_handle: int):
        """The next transition launches wait for what the caller's stream holds now (wn_engine_wait_stream)."""
        self._call(self.lib.wn_engine_wait_stream, C.c_void_p(stream_handle))

    def release_stream(self, stream_handle: int):
        """The caller's stream waits for every transition launch made so far (wn_engine_release_stream)."""
        self._call(self.lib.wn_engine_release_stream, C.c_void_p(stream_handle))

    @property
    def lanes(self) -> int:
        return self.lib.wn_engine_lanes(self.h)

    @property
    def dim_padded(self) -> int:
        return self.lib.wn_engine_dim_padded(self.h)

    @property
    def streaming(self) -> bool:
        return bool(self.lib.wn_engine_is_streaming(self.h))

    @property
    def held_tiles(self) -> int:
        """Streaming kernels: 16-byte pairs per lane of the trajectory's moving end kept in registers (0: both ends of
        every micro step stream through HBM)."""
        return self.lib.wn_engine_held_tiles(self.h)

    @property
    def workgroups(self) -> int:
        return self.lib.wn_engine_workgroups(self.h)

    @property
    def chain_groups(self) -> int:
        """Kernels one transition launch consists of (wn_config::chain_groups): contiguous chain blocks, one stream each."""
        return self.lib.wn_engine_chain_groups(self.h)

    @property
    def lds_vectors(self) -> int:
        return self.lib.wn_engine_lds_vectors(self.h)

    @property
    def iteration(self) -> int:
        return self.lib.wn_engine_iteration(self.h)

    @property
    def stream(self) -> int:
        return self.lib.wn_engine_stream(self.h) or 0

    @property
    def positions_device_ptr(self) -> int:
        return self.lib.wn_engine_positions_device(self.h) or 0
