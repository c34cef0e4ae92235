"""Probe (not a test): cost of hier_linear_regression_slopes_sigma (40, models/hier_slopes_scale_glm.h) against its two
siblings of the same build, hier_linear_regression_slopes (32, unit noise) at equal Q and hier_linear_regression_sigma
(35) at Q = 1.  N = 1 000 rows, J = 50 groups.

  python tests/gpu_probes/slopes_scale_rate.py [--sizes 150 900] [--q 1 2 4] [--runs 9] [--steps 3] [--evals 20]

num_params ~ 150 (16 384 chains; P = 100 columns, so num_params = 100 + 51 Q (+ 1)) and num_params = 900 (2 048 chains; P is
what is left).  All engines of one size are built and warmed up first; every measurement then ALTERNATES between them.

  (a) logp_grad at FIXED positions: the same theta (the shared coordinates; s = 0.1) is set into every engine, and `evals`
      launches of the gradient pass (wn_engine_init_masses_from_grad: one evaluation per chain and the mass write, no
      host copy) are timed with one pair of HIP events.  This rate does not depend on the posterior or on tree depths.
  (b) sampling transitions, `runs` rounds of `steps` each, timed with HIP events around every launch: grad-evals/s (the
      engines sample different posteriors, so their trees differ: the spread is reported).
One JSON line per engine and measurement: the median and the range of its runs, and the ratio of the medians to the
sibling's."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import walnuts_amd as wa  # noqa: E402

NEW, SLOPES, SIGMA = (wa.MODEL_HIER_LINEAR_REGRESSION_SLOPES_SIGMA, wa.MODEL_HIER_LINEAR_REGRESSION_SLOPES,
                      wa.MODEL_HIER_LINEAR_REGRESSION_SIGMA)


def make(P, J, Q, N, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(N, P)) / np.sqrt(P)
    group = rng.integers(0, J, size=N).astype(np.int32)
    z = np.concatenate([np.ones((N, 1)), x[:, :Q - 1]], axis=1)
    y = x @ rng.normal(size=P) + (0.7 * rng.normal(size=(Q, J))[:, group].T * z).sum(1) + 0.8 * rng.normal(size=N)
    return x, y, group


def ready(model, D, C, mp, data, Q, warmup):
    kw = dict(varying=Q) if model != SIGMA else {}
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=mp, data=data, **kw)
    e.init_positions(seed=1, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=2)
    e.warmup_steps(warmup)
    e.freeze()
    e.sample_steps(2)   # (the first sampling launches are not timed)
    e.synchronize()
    return e


def timed_transitions(e, steps):
    g0 = e.total_grad_evals()
    e.timing_reset()
    e.sample_steps(steps)
    e.synchronize()
    return (e.total_grad_evals() - g0) / (float(e.kernel_times_ms().sum()) / 1e3)


def timed_evals(e, evals):
    """gradient passes per second per chain-evaluation: C * evals / elapsed"""
    e.region_begin()
    for _ in range(evals):
        e.init_masses_from_grad(1e-5)
    ms, _ = e.region_ms()
    return e.C * evals / (ms / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[150, 900])
    ap.add_argument("--q", nargs="+", type=int, default=[1, 2, 4])
    ap.add_argument("--obs", type=int, default=1000)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    N, J = a.obs, a.groups
    for size in a.sizes:
        wide = size >= 512
        C = 2048 if wide else 16384
        for Q in a.q:
            P = size - Q * (J + 1) - 1 if wide else 100
            x, y, group = make(P, J, Q, N, seed=7)
            U = P + Q * J
            rng = np.random.default_rng(3)
            shared = np.concatenate([0.3 * rng.normal(size=(C, U)), rng.uniform(-0.5, 0.5, size=(C, Q))], axis=1)
            specs = [("slopes_sigma", NEW, 1)] + [("slopes", SLOPES, 0)] + ([("sigma", SIGMA, 1)] if Q == 1 else [])
            engines = []
            for name, model, scales in specs:
                D = U + Q + scales
                mp = np.concatenate([np.full(P, 4.0), np.ones(Q * J), np.ones(Q + scales)])
                e = ready(model, D, C, mp, (x, y, group), Q, a.warmup)
                theta = np.concatenate([shared, np.full((C, scales), 0.1)], axis=1)
                engines.append(dict(name=name, D=D, e=e, theta=theta, trans=[], evals=[]))
            for _ in range(a.runs):   # (b) first: the chains are where the warmup left them
                for it in engines:
                    it["trans"].append(timed_transitions(it["e"], a.steps))
            for it in engines:
                it["e"].check()
                it["e"].set_positions(it["theta"])
                timed_evals(it["e"], 2)   # (not timed)
            for _ in range(a.runs):
                for it in engines:
                    it["evals"].append(timed_evals(it["e"], a.evals))
            med = {it["name"]: (float(np.median(it["evals"])), float(np.median(it["trans"]))) for it in engines}
            for it in engines:
                for what, k, runs in (("logp_grad", 0, it["evals"]), ("transitions", 1, it["trans"])):
                    line = dict(run=it["name"], measure=what, q=Q, p=P, groups=J, obs=N, chains=C, dim=it["D"],
                                dim_padded=it["e"].dim_padded, evals_per_s_median=med[it["name"]][k],
                                evals_per_s_min=float(min(runs)), evals_per_s_max=float(max(runs)))
                    if it["name"] == "slopes_sigma":
                        for ref in med:
                            if ref != "slopes_sigma":
                                line["ratio_to_" + ref] = med["slopes_sigma"][k] / med[ref][k]
                    print(json.dumps(line), flush=True)
                it["e"].close()


if __name__ == "__main__":
    main()
