"""Probe (not a test): gradient-evaluation rate of hierarchical logistic regression with varying slopes
(models/hier_slopes_glm.h), N = 1 000 rows, J = 50 groups.

  python tests/gpu_probes/slopes_rate.py [--p 100 wide] [--runs 9] [--steps 3] [--obs 1000] [--groups 50]

  (a) the slopes model at Q = 1 against MODEL_HIER_LOGISTIC_REGRESSION of the same build on the same data -- the same
      arithmetic plus wave-uniform loop tests;
  (b) Q = 2, 4, 8 against Q = 1 -- what a varying slope costs beside the row's multiply-adds.
P = 100 (16 384 chains; num_params = 100 + 51 Q) and "wide", P = 900 - 51 Q (2 048 chains; num_params = 900 for every Q).
All engines of one P are built and warmed up first; the timed runs then ALTERNATE between them, `runs` rounds of `steps`
sampling transitions each, timed with HIP events around every launch.  The engines sample different posteriors, so
their trees differ: compare grad-evals/s, not ms per transition.  One JSON line per engine: the median and the range of
its runs, and the ratio of its median to the reference's (the hier model for Q = 1, Q = 1 for the others)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402


def make(P, J, Q, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    group = rng.integers(0, J, size=N).astype(np.int32)
    z = np.concatenate([np.ones((N, 1)), x[:, :Q - 1]], axis=1)
    u = 0.7 * rng.normal(size=(Q, J))
    eta = x @ rng.normal(size=P) + (u[:, group].T * z).sum(1)
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    mp = np.concatenate([np.full(P, 4.0), np.ones(Q * J), np.ones(Q)])
    return (x, y, group), mp


def ready(model, D, C, mp, data, warmup, **kw):
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=data, **kw)
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
        for name, Q in (("hier", 1), ("slopes_q1", 1), ("slopes_q2", 2), ("slopes_q4", 4), ("slopes_q8", 8)):
            P = 900 - Q * (J + 1) if wide else int(p)
            data, mp = make(P, J, Q, N, seed=7)   # (Q = 1: the same data for both models)
            D = P + Q * (J + 1)
            if name == "hier":
                e = ready(wa.MODEL_HIER_LOGISTIC_REGRESSION, D, C, mp, data, a.warmup)
            else:
                e = ready(wa.MODEL_HIER_LOGISTIC_REGRESSION_SLOPES, D, C, mp, data, a.warmup, varying=Q)
            engines.append((name, Q, P, D, e, []))
        for _ in range(a.runs):
            for item in engines:
                item[5].append(timed(item[4], a.steps))
        med = {name: float(np.median(r)) for name, _, _, _, _, r in engines}
        for name, Q, P, D, e, r in engines:
            e.check()
            ref = "hier" if name == "slopes_q1" else "slopes_q1"
            print(json.dumps(dict(run=name, varying=Q, p=P, groups=J, obs=N, chains=C, dim=D, dim_padded=e.dim_padded,
                                  steps=a.steps, grad_evals_per_s_kernel_median=med[name], grad_evals_per_s_kernel_min=min(r),
                                  grad_evals_per_s_kernel_max=max(r), runs=[float(v) for v in r], ratio_to=ref,
                                  ratio=med[name] / med[ref])), flush=True)
            e.close()


if __name__ == "__main__":
    main()
