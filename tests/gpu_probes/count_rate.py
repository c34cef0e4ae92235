"""Probe (not a test): gradient-evaluation rate of the count models and the linear model with an estimated noise level
(models/glm.h LogLink, models/glm_scale.h) against logistic regression, on one GPU.

  python tests/gpu_probes/count_rate.py [--chains 16384] [--dim 100] [--obs 1000 100000] [--steps 4]

For each N and model: warm up, then time sampling launches with a device synchronise.  Prints grad-evals/s, the rate
relative to logistic regression at the same N, and the time per row of one chain's gradient evaluation (wall time /
grad evals * chains in flight is not measured here: ns_per_row_per_eval = 1e9 / (rate N)).  The models differ only in
the link of the row pass (glm.h step 2), so the ratio to logistic regression says what the link costs against the
row read and the dot products."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402


def data(model, N, D, rng):
    """(dim, x, y, params) with x's column 0 all ones"""
    scale = model in (wa.MODEL_NEG_BINOMIAL_REGRESSION, wa.MODEL_LINEAR_REGRESSION_SIGMA)
    P = D - 1 if scale else D
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    x[:, 0] = 1.0
    eta = x @ (0.3 * rng.normal(size=P))
    if model == wa.MODEL_LOGISTIC_REGRESSION:
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    elif model == wa.MODEL_POISSON_REGRESSION:
        y = rng.poisson(np.exp(eta)).astype(np.float64)
    elif model == wa.MODEL_NEG_BINOMIAL_REGRESSION:
        y = rng.negative_binomial(2.0, 2.0 / (2.0 + np.exp(eta))).astype(np.float64)
    else:
        y = eta + 0.5 * rng.normal(size=N)
    mp = np.full(D, 4.0)
    if scale:
        mp[-1] = 1.0
    return D, x, y, mp


MODELS = [("logistic", wa.MODEL_LOGISTIC_REGRESSION), ("poisson", wa.MODEL_POISSON_REGRESSION),
          ("neg_binomial", wa.MODEL_NEG_BINOMIAL_REGRESSION), ("linear_sigma", wa.MODEL_LINEAR_REGRESSION_SIGMA)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--obs", type=int, nargs="+", default=[1000, 100000])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", nargs="+", default=[m for m, _ in MODELS], choices=[m for m, _ in MODELS])
    a = ap.parse_args()
    C = a.chains
    for N in a.obs:
        base = None
        for name, model in MODELS:
            if name not in a.models:
                continue
            D, x, y, mp = data(model, N, a.dim, np.random.default_rng(N))
            e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=(x, y))
            e.init_positions(seed=1, chain_offset=0, scale=0.5)
            e.init_masses_from_grad(1e-5)
            e.adapt_step(seed=2)
            e.warmup_steps(a.warmup)
            e.freeze()
            e.sample_steps(1)
            e.synchronize()
            g0 = e.total_grad_evals()
            t0 = time.perf_counter()
            e.sample_steps(a.steps)
            e.synchronize()
            dt = time.perf_counter() - t0
            e.check()
            grads = e.total_grad_evals() - g0
            e.close()
            rate = grads / dt
            base = rate if name == "logistic" else base
            print(json.dumps(dict(model=name, chains=C, dim=D, obs=N, grad_evals=grads, wall_s=dt,
                                  grad_evals_per_s=rate, rate_vs_logistic=None if base is None else rate / base,
                                  ns_per_row_per_eval=1e9 / (rate * N), ms_per_transition=dt * 1e3 / a.steps)),
                  flush=True)


if __name__ == "__main__":
    main()
