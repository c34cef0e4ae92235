"""Probe (not a test): what the predictive pass costs per draw against what wn_engine_eval costs per position, on one
GPU, same engine, same process.

  python tests/gpu_probes/pointwise_rate.py [--dim 100] [--obs 1000] [--chains 16384] [--draws 32] [--repeat 3]

Logistic regression, `chains` chains of `draws` resident draws each (uploaded once, a wn_chains block in HBM).
`log_predictive` folds all chains * draws draws over the N rows; `logp_grad` (wn_engine_eval, the kernel the sampler's
leapfrog steps are made of, unchanged by the pointwise work) evaluates `chains` positions.  Prints one JSON line: wall
milliseconds of each call (eval's includes its two host copies of [chains][dim] doubles), microseconds per draw / per
position, and the ratio.  Kernel time alone: run it under `rocprofv3 --kernel-trace --stats` (pointwise_kernel,
pointwise_combine_kernel against eval_kernel; collect no counters in the same run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402


def best_ms(fn, repeat):
    fn()  # (first call: allocations, code object load)
    best = float("inf")
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    D, N, C, S = a.dim, a.obs, a.chains, a.draws
    rng = np.random.default_rng(0)
    x = rng.normal(size=(N, D)) / np.sqrt(D)
    x[:, 0] = 1.0
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(x @ rng.normal(size=D))))).astype(np.float64)
    e = wa.DeviceEngine(wa.MODEL_LOGISTIC_REGRESSION, D, C, wa.default_config(), params=np.full(D, 4.0), data=(x, y))
    draws = rng.normal(size=(C * S, D)) * 0.3
    chains = wa.MarkovChains.from_host(draws, sizes=np.full(C, S))
    positions = np.ascontiguousarray(draws[::S])
    pred_ms = best_ms(lambda: e.log_predictive(chains), a.repeat)
    eval_ms = best_ms(lambda: e.logp_grad(positions), a.repeat)
    lpd = e.log_predictive(chains)[0]
    print(json.dumps(dict(dim=D, obs=N, chains=C, draws_per_chain=S, lanes=e.lanes, dim_padded=e.dim_padded,
                          log_predictive_ms=pred_ms, eval_ms=eval_ms, us_per_draw=pred_ms * 1e3 / (C * S),
                          us_per_position=eval_ms * 1e3 / C, ratio=(pred_ms / (C * S)) / (eval_ms / C),
                          elpd=float(np.sum(lpd)))))
    e.close()


if __name__ == "__main__":
    main()
