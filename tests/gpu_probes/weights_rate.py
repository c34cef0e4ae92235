"""Probe (not a test): gradient-evaluation rate of logistic regression refitted under W sets of 0/1 fold weights, as
weight sets over ONE shared block of rows (wn_observations::num_weight_sets) against the same refits built as
`datasets=` with x duplicated once per refit, on one GPU.

  python tests/gpu_probes/weights_rate.py [--chains 16384] [--dim 100] [--obs 1000] [--sets 16 256 4096]

For each W: fold g leaves out rows n with n % W == g.  `weight_sets`: x stored once, weights [W][N].  `datasets`: W
copies of (x, y) with per-dataset weights, chains [g*k, (g+1)*k) on copy g.  For each: warm up, then time sampling
launches with a device synchronise.  Prints grad-evals/s, ms per transition and the x + weight bytes resident in HBM.
Kernel time alone: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402


def rate_of(e, warmup, steps):
    e.init_positions(seed=1, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=2)
    e.warmup_steps(warmup)
    e.freeze()
    e.sample_steps(warmup)
    e.synchronize()
    g0 = e.total_grad_evals()
    t0 = time.perf_counter()
    e.sample_steps(steps)
    e.synchronize()
    dt = time.perf_counter() - t0
    e.check()
    return (e.total_grad_evals() - g0) / dt, dt * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--sets", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    D, C, N = a.dim, a.chains, a.obs
    rng = np.random.default_rng(0)
    x = rng.normal(size=(N, D)) / np.sqrt(D)
    x[:, 0] = 1.0
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(x @ rng.normal(size=D))))).astype(np.float64)
    s2 = np.full(D, 4.0)
    for W in a.sets:
        folds = (np.arange(N)[None, :] % W != np.arange(W)[:, None]).astype(np.float64)
        for form in ("weight_sets", "datasets"):
            if form == "weight_sets":
                e = wa.DeviceEngine(wa.MODEL_LOGISTIC_REGRESSION, D, C, wa.default_config(), params=s2, data=(x, y),
                                    weight_sets=folds)
                blocks = 1
            else:
                e = wa.DeviceEngine(wa.MODEL_LOGISTIC_REGRESSION, D, C, wa.default_config(), params=s2,
                                    datasets=[(x, y)] * W, weights=list(folds))
                blocks = W
            Dp = e.dim_padded
            rate, ms = rate_of(e, a.warmup, a.steps)
            e.close()
            print(json.dumps(dict(form=form, chains=C, dim=D, obs=N, sets=W, chains_per_set=C // W,
                                  resident_mb=(blocks * N * Dp + W * N) * 8 / 1e6, grad_evals_per_s=rate,
                                  ms_per_transition=ms)), flush=True)


if __name__ == "__main__":
    main()
