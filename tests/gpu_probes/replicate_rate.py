"""Probe (not a test): what the posterior predictive check costs per draw and row against the prediction fold, on one
GPU, same engine, same process, the two calls interleaved.

  python tests/gpu_probes/replicate_rate.py [--model logistic|poisson|negbin] [--dim 100] [--obs 1000] [--chains 16384]
                                            [--draws 32] [--repeat 9]

predict_rate.py's workload with the model as a choice: `chains` chains of `draws` resident draws each (uploaded once, a
wn_chains block in HBM), N rows.  `replicate_check` (replicate_kernel, wn_replicate.h: the row pass, one sampler call per
row, twelve accumulators, [6][chains][draws] outputs twice) and `predict_fold` (predict_kernel + predict_combine_kernel)
each visit all chains * draws draws over the N rows and end with their host copies.  poisson: the intercept puts mu
around 30 (the rejection sampler); negbin: the same with kappa = exp(-0.5).  After one warm-up call of each, the calls
alternate `repeat` times; the median wall time of each is reported.  The mean number of Philox calls per sample comes from
the sampler probe at the mu and scale of the first position.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402

MODELS = {"logistic": (wa.MODEL_LOGISTIC_REGRESSION, 1, 0), "poisson": (wa.MODEL_POISSON_REGRESSION, 2, 0),
          "negbin": (wa.MODEL_NEG_BINOMIAL_REGRESSION, 4, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=sorted(MODELS), default="logistic")
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--draws", type=int, default=32)
    ap.add_argument("--repeat", type=int, default=9)
    a = ap.parse_args()
    model, kind, extra = MODELS[a.model]
    P, N, Cn, S = a.dim, a.obs, a.chains, a.draws
    D = P + extra
    rng = np.random.default_rng(0)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    x[:, 0] = 1.0
    draws = rng.normal(size=(Cn * S, D)) * 0.3
    if a.model == "logistic":
        y = (rng.random(N) < 0.5).astype(np.float64)
    else:
        draws[:, 0] = np.log(30.0) + 0.1 * rng.normal(size=Cn * S)   # mu around 30
        y = rng.poisson(30.0, size=N).astype(np.float64)
    if extra:
        draws[:, -1] = -0.5
    e = wa.DeviceEngine(model, D, 1, wa.default_config(), params=np.full(D, 4.0), data=(x, y))
    chains = wa.MarkovChains.from_host(draws, sizes=np.full(Cn, S))
    calls = {"replicate_check": lambda: e.replicate_check(chains, 1), "predict_fold": lambda: e.predict_fold(chains)}
    for fn in calls.values():
        fn()  # (first call: allocations, code object load)
    times = {k: [] for k in calls}
    for _ in range(a.repeat):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t0) * 1e3)
    ms = {k: float(np.median(v)) for k, v in times.items()}
    per = {k: v * 1e9 / (Cn * S * N) for k, v in ms.items()}
    # Philox calls per sample at the first position's mu and scale
    _, mu, _ = e.predict(draws[:1])
    out, calls_out = np.empty(N), np.empty(N, dtype=np.intc)
    shape = np.full(N, np.exp(-0.5))
    dp = C.POINTER(C.c_double)
    rc = e.lib.wn_internal_sampler_probe(kind, mu[0].ctypes.data_as(dp), shape.ctypes.data_as(dp), 1, 0, 0, 0, N, 2,
                                         out.ctypes.data_as(dp), calls_out.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    rep, _ = e.replicate_check(chains, 1)
    print(json.dumps(dict(model=a.model, dim=D, obs=N, chains=Cn, draws_per_chain=S, lanes=e.lanes, dim_padded=e.dim_padded,
                          repeat=a.repeat, replicate_check_ms=ms["replicate_check"], predict_fold_ms=ms["predict_fold"],
                          replicate_check_ms_all=times["replicate_check"], predict_fold_ms_all=times["predict_fold"],
                          replicate_ps_per_draw_row=per["replicate_check"], predict_ps_per_draw_row=per["predict_fold"],
                          ratio=ms["replicate_check"] / ms["predict_fold"], philox_calls_per_sample=float(calls_out.mean()),
                          mean_mu=float(mu.mean()), invalid_draws=int(np.isnan(rep[0]).sum()))))
    e.close()


if __name__ == "__main__":
    main()
