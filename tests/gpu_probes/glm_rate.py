"""Probe (not a test): gradient-evaluation rate of the logistic-regression model (models/glm.h) on one GPU.

  python tests/gpu_probes/glm_rate.py [--chains 16384] [--dim 100] [--obs 1000 100000] [--steps 16]

For each N: warm up, then time sampling launches with a device synchronise.  Prints grad-evals/s, ms per transition
of all chains, x bytes per second (8 N D per gradient evaluation: every chain reads the whole block) and fp64 flops
(~4 N D per gradient evaluation) against the guide's figures, and the rate of a NumPy batched gradient on the host
for context.  Kernel time alone: run it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402

L2_SHARED_TBS = (16.8, 18.8)   # MI355X_MICROARCH.md: rows shared by every workgroup, served from L2 / MALL
FP64_VECTOR_PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--obs", type=int, nargs="+", default=[1000, 100000])
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    D, C = a.dim, a.chains
    for N in a.obs:
        x = rng.normal(size=(N, D)) / np.sqrt(D)
        x[:, 0] = 1.0
        beta = rng.normal(size=D)
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(x @ beta)))).astype(np.float64)
        e = wa.DeviceEngine(wa.MODEL_LOGISTIC_REGRESSION, D, C, wa.default_config(), params=np.full(D, 4.0), data=(x, y))
        e.init_positions(seed=1, chain_offset=0, scale=0.5)
        e.init_masses_from_grad(1e-5)
        e.adapt_step(seed=2)
        e.warmup_steps(a.warmup)
        e.freeze()
        e.sample_steps(a.warmup)
        e.synchronize()
        g0 = e.total_grad_evals()
        t0 = time.perf_counter()
        e.sample_steps(a.steps)
        e.synchronize()
        dt = time.perf_counter() - t0
        e.check()
        grads = e.total_grad_evals() - g0
        rate = grads / dt
        x_bytes = rate * 8.0 * N * D
        flops = rate * 4.0 * N * D
        e.close()
        theta = rng.normal(size=(min(C, 1024), D))
        t1 = time.perf_counter()
        eta = theta @ x.T
        _ = (y - 1.0 / (1.0 + np.exp(-eta))) @ x
        host_rate = theta.shape[0] / (time.perf_counter() - t1)
        print(json.dumps(dict(
            chains=C, dim=D, obs=N, x_mib=N * D * 8 / 2**20, grad_evals_per_s=rate,
            ms_per_transition=dt * 1e3 / a.steps, x_tb_per_s=x_bytes / 1e12,
            x_frac_of_shared_row_rate=[x_bytes / 1e12 / r for r in L2_SHARED_TBS],
            fp64_tflops=flops / 1e12, fp64_frac_of_vector_peak=flops / 1e12 / FP64_VECTOR_PEAK_TFLOPS,
            numpy_host_grad_evals_per_s=host_rate)), flush=True)


if __name__ == "__main__":
    main()
