"""Probe (not a test): what the prediction fold costs per draw and row against the predictive scoring pass, on one GPU,
same engine, same process, the two calls interleaved.

  python tests/gpu_probes/predict_rate.py [--dim 100] [--obs 1000] [--chains 16384] [--draws 32] [--repeat 5]

pointwise_rate.py's workload: logistic regression, `chains` chains of `draws` resident draws each (uploaded once, a
wn_chains block in HBM).  `predict_fold` (predict_kernel + predict_combine_kernel, wn_predict.h) and `log_predictive`
(pointwise_kernel + pointwise_combine_kernel, wn_pointwise.h) each fold all chains * draws draws over the N rows; both
end with their host copies of [N] outputs (six arrays against four).  After one warm-up call of each, the calls
alternate `repeat` times and the median wall time of each is reported.  Prints one JSON line: milliseconds per call,
picoseconds per draw and row, and the ratio predict_fold / log_predictive.  Kernel time alone: run it under
`rocprofv3 --kernel-trace --stats` (collect no counters in the same run)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    D, N, C, S = a.dim, a.obs, a.chains, a.draws
    rng = np.random.default_rng(0)
    x = rng.normal(size=(N, D)) / np.sqrt(D)
    x[:, 0] = 1.0
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(x @ rng.normal(size=D))))).astype(np.float64)
    e = wa.DeviceEngine(wa.MODEL_LOGISTIC_REGRESSION, D, 1, wa.default_config(), params=np.full(D, 4.0), data=(x, y))
    draws = rng.normal(size=(C * S, D)) * 0.3
    chains = wa.MarkovChains.from_host(draws, sizes=np.full(C, S))
    calls = {"predict_fold": lambda: e.predict_fold(chains), "log_predictive": lambda: e.log_predictive(chains)}
    for fn in calls.values():
        fn()  # (first call: allocations, code object load)
    times = {k: [] for k in calls}
    for _ in range(a.repeat):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    ms = {k: float(np.median(v)) for k, v in times.items()}
    per = {k: v * 1e9 / (C * S * N) for k, v in ms.items()}
    mean = e.predict_fold(chains)[2]
    print(json.dumps(dict(dim=D, obs=N, chains=C, draws_per_chain=S, lanes=e.lanes, dim_padded=e.dim_padded, repeat=a.repeat,
                          predict_fold_ms=ms["predict_fold"], log_predictive_ms=ms["log_predictive"],
                          predict_fold_ms_all=times["predict_fold"], log_predictive_ms_all=times["log_predictive"],
                          predict_ps_per_draw_row=per["predict_fold"], log_predictive_ps_per_draw_row=per["log_predictive"],
                          ratio=ms["predict_fold"] / ms["log_predictive"], mean_of_means=float(np.mean(mean)))))
    e.close()


if __name__ == "__main__":
    main()
