"""Probe (not a test): what PSIS-LOO costs against the predictive pass, on one GPU, same engine, same draws, same process.

  python tests/gpu_probes/psis_rate.py [--dims 100,1000] [--obs 1000] [--chains 16384] [--draws 32] [--repeat 5]

Logistic regression, `chains` chains of `draws` resident draws each (uploaded once, a wn_chains block in HBM).
`log_predictive` folds all chains * draws draws over the N rows in registers; `psis_loo` writes the same terms to the
rows-by-draws matrix (1 GiB of workspace at a time) and runs psis_row_kernel over every column.  Prints one JSON line per
dimension: wall milliseconds of each call (both end in a device synchronise and the copy of their per-row results) --
median, smallest and largest of `repeat` timed calls, the two calls alternating after one untimed call of each -- and
the ratio of the medians.
Kernel time alone: run it under `rocprofv3 --kernel-trace --stats` (pointwise_kernel and psis_row_kernel against
pointwise_kernel and pointwise_combine_kernel; collect no counters in the same run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402


def alternate_ms(fns, repeat):
    """[median, min, max] wall milliseconds per function, the functions taking turns"""
    for fn in fns:
        fn()  # (first call: allocations, code object load)
    times = [[] for _ in fns]
    for _ in range(repeat):
        for fn, t in zip(fns, times):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
    return [[float(np.median(t)), min(t), max(t)] for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="100,1000")
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    N, C, S = a.obs, a.chains, a.draws
    for D in (int(d) for d in a.dims.split(",")):
        rng = np.random.default_rng(0)
        x = rng.normal(size=(N, D)) / np.sqrt(D)
        x[:, 0] = 1.0
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(x @ rng.normal(size=D))))).astype(np.float64)
        e = wa.DeviceEngine(wa.MODEL_LOGISTIC_REGRESSION, D, 1, wa.default_config(), params=np.full(D, 4.0), data=(x, y))
        draws = rng.normal(size=(C * S, D)) * 0.3
        chains = wa.MarkovChains.from_host(draws, sizes=np.full(C, S))
        del draws
        pred_ms, psis_ms = alternate_ms([lambda: e.log_predictive(chains), lambda: e.psis_loo(chains)], a.repeat)
        elpd, k = e.psis_loo(chains)[:2]
        print(json.dumps(dict(dim=D, obs=N, chains=C, draws_per_chain=S, lanes=e.lanes, dim_padded=e.dim_padded,
                              repeat=a.repeat, log_predictive_ms=pred_ms, psis_loo_ms=psis_ms, ratio=psis_ms[0] / pred_ms[0],
                              elpd_loo=float(np.sum(elpd)), worst_pareto_k=float(np.max(k)))), flush=True)
        chains.close()
        e.close()


if __name__ == "__main__":
    main()
