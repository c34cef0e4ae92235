"""GPU tier: models conditioned on data (walnuts_amd/csrc/models/glm.h) on the MI355X.

  * device = emulation, bit for bit: the same kernel source under tests/cpusim and on gfx950, same geometry asked of both;
  * (1, 8) -- eight elements per lane, the default for 257-512 parameters -- also against NumPy and for determinism;
  * the linear model against its closed-form posterior, the logistic model against its Laplace approximation;
  * the drop-in call with data, draws on the host and kept on the device;
  * the GLM edge matrix of test_data_models_sim.py (N around the block size, D at the padding boundary, saturated
    logits) at 2, 4, 8 and 16 elements per lane against the high-precision reference;
  * many chains (more than resident), fused transitions and two chain groups against emulated 8-chain slices at their
    chain offsets, bit for bit: the data models have no oracle, so the emulation of the same source stands in for it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "cpusim"))
import build as simbuild  # noqa: E402
import walnuts_amd as wa  # noqa: E402
from test_data_models_sim import LIN, LOG, check_glm_edges, edge_dims, make_data, numpy_logp_grad  # noqa: E402

pytestmark = pytest.mark.gpu


def run(lib, model, D, C, data, s2, geometry, fma, warm=6, samp=6):
    cfg = wa.default_config(lib, fused_multiply_add=fma, waves_per_chain=geometry[0], elems_per_lane=geometry[1])
    e = wa.DeviceEngine(model, D, C, cfg, params=s2, lib_path=lib, data=data)
    theta = np.random.default_rng(D).normal(size=(C, D)) * 0.3
    lp, g = e.logp_grad(theta)
    e.init_positions(seed=17, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=18)
    for _ in range(warm):
        e.warmup_step()
    e.freeze()
    for _ in range(samp):
        e.sample_step()
    e.check()
    out = dict(lp_eval=lp, g_eval=g, pos=e.positions(), logp=e.logp(), depth=e.depths(), grads=e.grad_evals(),
               steps=e.step_sizes(), inv_mass=e.inv_mass())
    e.close()
    return out


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("model", [LIN, LOG])
@pytest.mark.parametrize("D,N,geometry", [(5, 70, (1, 2)), (150, 130, (1, 4)), (1000, 60, (1, 16)),
                                          (1000, 7, (1, 16)), (150, 5, (1, 4)),  # (odd N at B = 2; N < B = 8)
                                          (300, 9, (1, 8)), (512, 5, (1, 8))])  # (N = 2 B + 1 and B + 1 at B = 4; no padding)
@pytest.mark.parametrize("fma", [0, 1])
def test_device_equals_emulation(gpu, model, D, N, geometry, fma):
    sim = simbuild.build()
    x, y, s2 = make_data(model, D, N, seed=D)
    C = 4 if D == 1000 else 8
    dev = run(None, model, D, C, (x, y), s2, geometry, fma)
    emu = run(sim, model, D, C, (x, y), s2, geometry, fma)
    for k in dev:
        assert np.array_equal(dev[k], emu[k]), k


@pytest.mark.timeout(600)
@pytest.mark.parametrize("model", [LIN, LOG])
def test_eight_per_lane_on_the_device(gpu, model):
    D, N = 400, 250
    x, y, s2 = make_data(model, D, N, seed=11)
    e = wa.DeviceEngine(model, D, 6, wa.default_config(), params=s2, data=(x, y))
    assert e.lanes == 64 and e.dim_padded == 512
    theta = np.random.default_rng(2).normal(size=(6, D)) * 0.2
    lp, g = e.logp_grad(theta)
    lp_ref, g_ref = numpy_logp_grad(model, x, y, s2, theta)
    assert np.all(np.abs(lp - lp_ref) <= 1e-12 * np.abs(lp_ref))
    for c in range(6):
        assert np.linalg.norm(g[c] - g_ref[c]) <= 1e-12 * np.linalg.norm(g_ref[c])
    a = run(None, model, D, 6, (x, y), s2, (1, 8), 1)
    b = run(None, model, D, 6, (x, y), s2, (1, 8), 1)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.all(np.isfinite(a["pos"]))


def lockstep_draws(model, D, C, x, y, s2, warm, samp, seed, start=None):
    """init -> adapt_step -> `warm` warmup transitions -> freeze -> `samp` sampling transitions, draws on the device
    (`start` [C, D]: initial positions instead of the generator's)."""
    import torch
    e = wa.DeviceEngine(model, D, C, wa.default_config(), params=s2, data=(x, y))
    if start is None:
        e.init_positions(seed=seed, chain_offset=0, scale=0.5)
    else:
        e.set_positions(start)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=seed + 1)
    e.warmup_steps(warm)
    e.freeze()
    draws = torch.empty((C, samp, D), dtype=torch.float64, device="cuda")
    e.sample_steps(samp, draws.data_ptr(), samp * D, D)
    e.synchronize()
    e.check()
    out = draws.cpu().numpy()
    e.close()
    return out


def rhat(d):  # [C, S] split-free Gelman-Rubin
    C, S = d.shape
    W = d.var(axis=1, ddof=1).mean()
    B = S * d.mean(axis=1).var(ddof=1)
    return np.sqrt(((S - 1) / S * W + B / S) / W)


def mcse_mean(z):  # [C, S]: per-chain means are independent; their spread gives the standard error
    m = z.mean(axis=1)
    return m.std(ddof=1) / np.sqrt(len(m))


@pytest.mark.timeout(1800)
def test_linear_regression_exact_posterior(gpu):
    D, N, C = 16, 400, 4096
    rng = np.random.default_rng(21)
    x = rng.normal(size=(N, D))
    x[:, 0] = 1.0
    y = x @ rng.normal(size=D) + rng.normal(size=N)
    s2 = np.full(D, 4.0)
    draws = lockstep_draws(LIN, D, C, x, y, s2, 200, 200, seed=5)
    prec = x.T @ x + np.diag(1.0 / s2)
    cov = np.linalg.inv(prec)
    mu = cov @ (x.T @ y)
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, (draws.reshape(-1, D) - mu).T).T.reshape(C, -1, D)
    for i in range(D):
        zi = z[:, :, i]
        assert abs(zi.mean()) <= 5 * mcse_mean(zi), i
        assert abs(zi.var() - 1.0) <= 0.03, (i, zi.var())
        assert rhat(zi) <= 1.01, i
    corr = np.corrcoef(z.reshape(-1, D).T)
    assert np.max(np.abs(corr - np.eye(D))) < 0.02


@pytest.mark.timeout(1800)
def test_logistic_regression_large_sample_limit(gpu):
    D, N, C = 6, 20000, 1024
    rng = np.random.default_rng(22)
    x = rng.normal(size=(N, D))
    x[:, 0] = 1.0
    beta = np.array([0.3, 1.0, -0.5, 0.25, 0.0, -1.0])
    y = (rng.random(N) < 1.0 / (1.0 + np.exp(-(x @ beta)))).astype(np.float64)
    s2 = np.full(D, 25.0)
    th = np.zeros(D)
    for _ in range(50):  # Newton on the log posterior
        p = 1.0 / (1.0 + np.exp(-(x @ th)))
        grad = x.T @ (y - p) - th / s2
        H = (x * (p * (1 - p))[:, None]).T @ x + np.diag(1.0 / s2)
        th = th + np.linalg.solve(H, grad)
    p = 1.0 / (1.0 + np.exp(-(x @ th)))
    H = (x * (p * (1 - p))[:, None]).T @ x + np.diag(1.0 / s2)
    laplace_sd = np.sqrt(np.diag(np.linalg.inv(H)))
    # 20 000 observations make the posterior ~50 times narrower than the generator's initial spread: the chains start
    # overdispersed around the mode (3 Laplace sds) instead, as a user with this much data would start them
    start = th + 3.0 * laplace_sd * rng.normal(size=(C, D))
    draws = lockstep_draws(LOG, D, C, x, y, s2, 300, 200, seed=8, start=start).reshape(-1, D)
    sd = draws.std(axis=0)
    assert np.all(np.abs(draws.mean(axis=0) - th) <= 0.05 * sd)
    assert np.all(np.abs(sd / laplace_sd - 1.0) <= 0.05)


@pytest.mark.timeout(900)
def test_drop_in_call_with_data_on_the_device(gpu):
    D, N = 6, 500
    x, y, s2 = make_data(LOG, D, N, seed=3)
    kw = dict(model_params=s2, num_params=D, num_chains=64, seed=4, min_warmup_iter=100, max_warmup_iter=100,
              min_sampling_iter=100, max_sampling_iter=100, data=(x, y))
    host = np.array([np.asarray(r) for r in wa.walnuts_device(LOG, **kw)])  # [C, S, D]
    kept, chains = wa.walnuts_device(LOG, keep_on_device=True, thin=1, **kw)
    assert np.array_equal(host, np.array([np.asarray(r) for r in kept]))
    flat = host.reshape(-1, D)
    assert np.allclose(chains.mean(), flat.mean(axis=0), rtol=1e-10, atol=1e-12)
    assert np.all(np.isfinite(chains.r_hat()))
    chains.close()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("epl", [2, 4, 8, 16])
@pytest.mark.parametrize("model", [LIN, LOG], ids=["linear", "logistic"])
def test_glm_edges_on_the_device(gpu, model, epl, fma, record_property):
    """The CPU tier's edge matrix on gfx950: N in 1, B - 1, B, B + 1 (and 7 at B = 2), D in 1, 64 EPL - 1, 64 EPL,
    saturated and exactly-zero logits, all-zero and duplicated rows, y all 0 / all 1, |y| ~ 1e6."""
    record_property("max_error_over_bound", max(check_glm_edges(None, model, epl, fma, D) for D in edge_dims(epl)))


def sliced_run(lib, C, offset, mode, x, y, s2, wg_per_cu=0):
    """logistic regression, C chains starting at chain `offset`: seed, init, adapt, then four warmup and four sampling
    transitions -- one launch each ("single"), in launches of four ("fused"), both in one chain group, or in launches of
    four split in two chain groups ("groups")."""
    D = x.shape[1]
    cfg = wa.default_config(lib, chain_groups=2 if mode == "groups" else 1, workgroups_per_cu=wg_per_cu)
    e = wa.DeviceEngine(LOG, D, C, cfg, params=s2, lib_path=lib, data=(x, y))
    if lib is None:
        assert e.workgroups < C, "the device run must hold more chains than are resident"
        assert e.chain_groups == (2 if mode == "groups" else 1)
    e.seed_chains(7, offset)
    e.init_positions(seed=3, chain_offset=offset, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=4, chain_offset=offset)
    if mode == "single":
        for _ in range(4):
            e.warmup_step()
        e.freeze()
        for _ in range(4):
            e.sample_step()
    else:
        e.warmup_steps(4)
        e.freeze()
        e.sample_steps(4)
    e.check()
    out = dict(pos=e.positions(), logp=e.logp(), steps=e.step_sizes(), inv_mass=e.inv_mass(), depths=e.depths(),
               grads=e.grad_evals())
    e.close()
    return out


@pytest.mark.timeout(1800)
def test_data_model_launches_against_emulated_slices(gpu):
    """3 000 chains of logistic regression (D = 20, N = 37) on the device, one workgroup per CU so that chains queue
    for the persistent workgroups, run as single transitions, fused launches and two chain groups: chains [0, 8),
    [1496, 1504) and [2992, 3000) of every run equal emulation runs of 8 chains at those chain offsets, bit for bit."""
    sim = simbuild.build()
    D, N, C = 20, 37, 3000
    rng = np.random.default_rng(1)
    x = rng.normal(size=(N, D))
    y = (rng.random(N) < 0.5).astype(np.float64)
    s2 = np.full(D, 2.0)
    slices = (0, 1496, 2992)
    emu = {o: sliced_run(sim, 8, o, "single", x, y, s2) for o in slices}
    for mode in ("single", "fused", "groups"):
        dev = sliced_run(None, C, 0, mode, x, y, s2, wg_per_cu=1)
        for o in slices:
            for k in emu[o]:
                assert np.array_equal(dev[k][o:o + 8], emu[o][k]), (mode, o, k)
