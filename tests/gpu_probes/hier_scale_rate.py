"""Probe (not a test): gradient-evaluation rate of the grouped models with a scale parameter
(models/hier_scale_glm.h), N = 1 000 rows, J = 50 groups, against their nearest siblings of the same build.

  python tests/gpu_probes/hier_scale_rate.py [--p 100 wide] [--runs 9] [--steps 3] [--obs 1000] [--groups 50]

  hier_linear_regression_sigma(_centered)   against hier_linear_regression(_centered): the same block pass, the row term
                                            with 1 / sigma^2 and a d/ds partial, one more lane accumulator
P = 100 (16 384 chains; num_params = 152 for the new models, 151 for the hier siblings) and "wide" (2 048 chains;
num_params = 900 for every model, so P = 848 or 849).  All engines of one P are built and warmed up
first; the timed runs then ALTERNATE between them, `runs` rounds of `steps` sampling transitions each, timed with HIP
events around every launch.  The engines sample different posteriors, so their trees differ: compare grad-evals/s, not
ms per transition.  One JSON line per engine: the median and the range of its runs, and the ratio of its median to its
sibling's."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402

# name -> (model, trailing log scales after beta and the effects, the engine it is compared with)
ENGINES = {
    "hier_linear": (wa.MODEL_HIER_LINEAR_REGRESSION, 1, None),
    "hier_linear_sigma": (wa.MODEL_HIER_LINEAR_REGRESSION_SIGMA, 2, "hier_linear"),
    "hier_linear_c": (wa.MODEL_HIER_LINEAR_REGRESSION_CENTERED, 1, None),
    "hier_linear_sigma_c": (wa.MODEL_HIER_LINEAR_REGRESSION_SIGMA_CENTERED, 2, "hier_linear_c"),
}


def make(P, J, N, trailing, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    group = rng.integers(0, J, size=N).astype(np.int32)
    y = x @ rng.normal(size=P) + 0.7 * rng.normal(size=J)[group] + 0.8 * rng.normal(size=N)
    return (x, y, group), np.concatenate([np.full(P, 4.0), np.ones(J), np.ones(trailing)])


def ready(model, D, C, mp, data, warmup):
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=data)
    e.init_positions(seed=1, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=2)
    e.warmup_steps(warmup)
    e.freeze()
    e.sample_steps(2)   # (the first sampling launches are not timed)
    e.synchronize()
    return e


def timed(e, steps):
    g0 = e.total_grad_evals()
    e.timing_reset()
    e.sample_steps(steps)
    e.synchronize()
    return (e.total_grad_evals() - g0) / (float(e.kernel_times_ms().sum()) / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", nargs="+", default=["100", "wide"])
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    N, J = a.obs, a.groups
    for p in a.p:
        wide = p == "wide"
        C = 2048 if wide else 16384
        engines = []
        for name, (model, trailing, ref) in ENGINES.items():
            P = 900 - J - trailing if wide else int(p)   # wide: num_params = 900 for every model
            data, mp = make(P, J, N, trailing, seed=7)   # (the same x, group and noise for every model of one P)
            D = P + J + trailing
            engines.append((name, P, D, ready(model, D, C, mp, data, a.warmup), [], ref))
        for _ in range(a.runs):
            for item in engines:
                item[4].append(timed(item[3], a.steps))
        med = {name: float(np.median(r)) for name, _, _, _, r, _ in engines}
        for name, P, D, e, r, ref in engines:
            e.check()
            print(json.dumps(dict(run=name, p=P, groups=J, obs=N, chains=C, dim=D, dim_padded=e.dim_padded, steps=a.steps,
                                  grad_evals_per_s_kernel_median=med[name], grad_evals_per_s_kernel_min=min(r),
                                  grad_evals_per_s_kernel_max=max(r), runs=[float(v) for v in r],
                                  ratio_to=ref, ratio=None if ref is None else med[name] / med[ref])), flush=True)
            e.close()


if __name__ == "__main__":
    main()
