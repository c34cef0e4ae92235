"""Probe (not a test): gradient-evaluation rate of logistic regression with many datasets in one engine
(wn_observations::obs_offsets) against one shared block, on one GPU.

  python tests/gpu_probes/datasets_rate.py [--chains 16384] [--dim 100] [--obs 1000] [--datasets 0 16 256 4096]

`--datasets 0` is the shared-data engine (every chain reads one block).  G > 0: G datasets of `obs` rows each, chains
[g*k, (g+1)*k) on dataset g, so the engine reads G times as many distinct rows.  For each: warm up, then time sampling
launches with a device synchronise.  Prints grad-evals/s, ms per transition, the distinct x bytes resident in HBM and
the x bytes the gradients read per second (8 N Dp per evaluation).  Kernel time alone: run it under
`rocprofv3 --kernel-trace --stats`."""
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
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--datasets", type=int, nargs="+", default=[0, 16, 256, 4096])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    D, C, N = a.dim, a.chains, a.obs
    for G in a.datasets:
        rng = np.random.default_rng(0)
        blocks = max(G, 1)
        x = rng.normal(size=(blocks * N, D)) / np.sqrt(D)
        x[:, 0] = 1.0
        beta = rng.normal(size=(blocks, D))
        eta = np.einsum("gnd,gd->gn", x.reshape(blocks, N, D), beta).reshape(-1)
        y = (rng.random(blocks * N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
        kw = dict(data=(x, y)) if G == 0 else dict(datasets=[(x[g * N:(g + 1) * N], y[g * N:(g + 1) * N])
                                                             for g in range(G)])
        e = wa.DeviceEngine(wa.MODEL_LOGISTIC_REGRESSION, D, C, wa.default_config(), params=np.full(D, 4.0), **kw)
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
        Dp = e.dim_padded
        e.close()
        print(json.dumps(dict(
            chains=C, dim=D, obs_per_dataset=N, datasets=G, chains_per_dataset=C // blocks,
            x_resident_mb=blocks * N * Dp * 8 / 1e6, grad_evals_per_s=rate, ms_per_transition=dt * 1e3 / a.steps,
            x_read_tb_per_s=rate * 8.0 * N * Dp / 1e12)), flush=True)


if __name__ == "__main__":
    main()
