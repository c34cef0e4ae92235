"""Probe (not a test): gradient-evaluation rate of hierarchical logistic regression (models/hier_glm.h, a group index
per observation) against the dense one-hot workaround (a flat MODEL_LOGISTIC_REGRESSION on x widened with the J group
indicators: D = P + J, every gradient evaluation reads 8 N Dp bytes of x instead of 8 N Dx + 4 N).

  python tests/gpu_probes/hier_rate.py [--chains 16384] [--p 10] [--obs 10000] [--groups 10 100 500] [--steps 4]

For each J: the non-centered and centered models and the dense workaround; warm up, then time sampling launches with a
device synchronise (wall) and with HIP events around every launch (kernel).  The three runs sample different
posteriors or parameterizations, so their trees differ: compare grad-evals/s, not ms per transition.  Kernel-trace
times: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402


def measure(model, D, C, mp, data, steps, warmup):
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=data)
    e.init_positions(seed=1, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=2)
    e.warmup_steps(warmup)
    e.freeze()
    e.sample_steps(1)
    e.synchronize()
    g0 = e.total_grad_evals()
    e.timing_reset()
    t0 = time.perf_counter()
    e.sample_steps(steps)
    e.synchronize()
    dt = time.perf_counter() - t0
    kernel_ms = float(e.kernel_times_ms().sum())
    e.check()
    grads = e.total_grad_evals() - g0
    out = dict(dim=D, dim_padded=e.dim_padded, grad_evals=int(grads), wall_s=dt, kernel_s=kernel_ms / 1e3,
               grad_evals_per_s_wall=grads / dt, grad_evals_per_s_kernel=grads / (kernel_ms / 1e3),
               ms_per_transition_wall=dt * 1e3 / steps)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--p", type=int, default=10)
    ap.add_argument("--obs", type=int, default=10000)
    ap.add_argument("--groups", type=int, nargs="+", default=[10, 100, 500])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    P, N, C = a.p, a.obs, a.chains
    for J in a.groups:
        x = rng.normal(size=(N, P)) / np.sqrt(P)
        group = rng.integers(0, J, size=N).astype(np.int32)
        eta = x @ rng.normal(size=P) + 0.7 * rng.normal(size=J)[group]
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        D = P + J + 1
        mp = np.concatenate([np.full(P, 4.0), np.ones(J), [1.0]])
        rows = {}
        for name, model in (("hier_noncentered", wa.MODEL_HIER_LOGISTIC_REGRESSION),
                            ("hier_centered", wa.MODEL_HIER_LOGISTIC_REGRESSION_CENTERED)):
            rows[name] = measure(model, D, C, mp, (x, y, group), a.steps, a.warmup)
        xw = np.concatenate([x, np.eye(J)[group]], axis=1)
        rows["dense_one_hot"] = measure(wa.MODEL_LOGISTIC_REGRESSION, P + J, C, np.full(P + J, 4.0), (xw, y),
                                        a.steps, a.warmup)
        for name, r in rows.items():
            x_bytes = 8.0 * N * (r["dim_padded"] if name == "dense_one_hot" else 128 * -(-P // 128)) + (
                0 if name == "dense_one_hot" else 4.0 * N)
            print(json.dumps(dict(run=name, chains=C, p=P, groups=J, obs=N, row_bytes_per_eval=x_bytes, **r,
                                  speedup_vs_dense_kernel=r["grad_evals_per_s_kernel"]
                                  / rows["dense_one_hot"]["grad_evals_per_s_kernel"])), flush=True)


if __name__ == "__main__":
    main()
