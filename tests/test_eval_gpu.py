"""GPU tier: wn_engine_eval (DeviceEngine.logp_grad) of the models without data, on every geometry the library builds,
against the high-precision references of tests/helpers/hp_reference.py, and the evaluation's agreement with what the
transitions store as logp.

  * eval_kernel at the 17 register geometries of wn_launch.h and eval_kernel_mem at the streaming NW in {2, 4, 8, 16},
    plus the held-moving-end default; D = the smallest size the model takes, Dp - 1 and Dp (streaming: and a ragged
    last tile of a longer vector), both arithmetic modes; one case with more chains than the grid (grid-stride loop);
  * logp() after init, adapt, three warmup and one sampling transition equals logp_grad(positions())[0], bit for bit,
    for every model and one geometry per kernel family."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import hp_reference as hp  # noqa: E402
import walnuts_amd as wa  # noqa: E402

pytestmark = pytest.mark.gpu

STD, DIAG, FUNNEL, RW1 = wa.MODEL_STD_NORMAL, wa.MODEL_DIAG_NORMAL, wa.MODEL_FUNNEL, wa.MODEL_RW1
LIN, LOG = wa.MODEL_LINEAR_REGRESSION, wa.MODEL_LOGISTIC_REGRESSION
MODELS = (STD, DIAG, FUNNEL, RW1)
NAMES = {STD: "std_normal", DIAG: "diag_normal", FUNNEL: "funnel", RW1: "rw1", LIN: "linear", LOG: "logistic"}
REGISTER = ((1, 2), (1, 4), (1, 8), (1, 16), (2, 2), (2, 4), (2, 8), (2, 16), (4, 2), (4, 4), (4, 8), (4, 16), (8, 2),
            (8, 4), (8, 8), (16, 4), (16, 8))  # WN_FOR_EACH_GEOMETRY of a full build
STREAMING = (2, 4, 8, 16)  # WN_FOR_EACH_MEM_GEOMETRY


def smallest_dim(model):
    return 2 if model == FUNNEL else 1


def theta_for(model, C, D, seed):
    rng = np.random.default_rng(seed)
    theta = rng.normal(size=(C, D))
    if model == FUNNEL:
        theta[:, 0] = rng.uniform(-3.0, 3.0, size=C)  # e^-v over three orders of magnitude either way
    return theta


def params_for(model, D, seed):
    return np.random.default_rng(seed + 1).uniform(0.25, 4.0, size=D) if model == DIAG else None


def eval_case(model, D, C, cfg, seed):
    """logp_grad on the device against the reference; returns (error / bound, the engine's geometry)."""
    params = params_for(model, D, seed)
    theta = theta_for(model, C, D, seed)
    e = wa.DeviceEngine(model, D, C, cfg, params=params)
    geom = (e.lanes // 64, e.dim_padded, e.streaming, e.held_tiles)
    e.init_positions(seed=seed, chain_offset=0, scale=1.0)
    before = e.positions()
    lp, g = e.logp_grad(theta)
    assert np.array_equal(e.positions(), before), "logp_grad must leave the chains' state alone"
    e.close()
    nw, dp = geom[0], geom[1]
    ref = hp.simple_case(model, theta, params, dp // (64 * nw), nw)
    ratio = hp.error_ratio(lp, g, ref)
    assert ratio <= 1.0, (NAMES[model], D, geom, ratio)
    return ratio, geom


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("geometry", REGISTER, ids=lambda g: f"nw{g[0]}_epl{g[1]}")
@pytest.mark.parametrize("model", MODELS, ids=lambda m: NAMES[m])
def test_eval_register_geometries(gpu, model, geometry, fma, record_property):
    nw, epl = geometry
    dp = 64 * nw * epl
    worst = 0.0
    for D in (smallest_dim(model), dp - 1, dp):
        cfg = wa.default_config(fused_multiply_add=fma, waves_per_chain=nw, elems_per_lane=epl)
        ratio, geom = eval_case(model, D, 3, cfg, seed=D + 7 * nw + epl)
        assert geom[:3] == (nw, dp, False)
        worst = max(worst, ratio)
    record_property("max_error_over_bound", worst)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("nw", STREAMING)
@pytest.mark.parametrize("model", MODELS, ids=lambda m: NAMES[m])
def test_eval_streaming_geometries(gpu, model, nw, fma, record_property):
    tile = 2 * 64 * nw
    worst = 0.0
    for D in (smallest_dim(model), tile - 1, tile, 2 * tile + 3):  # (2 * tile + 3: three tiles, the last one ragged)
        cfg = wa.default_config(fused_multiply_add=fma, waves_per_chain=nw, elems_per_lane=-1)
        ratio, geom = eval_case(model, D, 3, cfg, seed=D + nw)
        assert geom[0] == nw and geom[2] and geom[1] == -(-D // tile) * tile
        worst = max(worst, ratio)
    record_property("max_error_over_bound", worst)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("model", MODELS, ids=lambda m: NAMES[m])
def test_eval_held_streaming_default(gpu, model, fma, record_property):
    """The default geometry past the register kernels' limit: eight wavefronts streaming, the moving end held where the
    model has such kernels (the evaluation itself streams both)."""
    D = 9000 if model == FUNNEL else 5000
    ratio, geom = eval_case(model, D, 3, wa.default_config(fused_multiply_add=fma), seed=D)
    assert geom[0] == 8 and geom[2]
    record_property("held_tiles", geom[3])
    record_property("max_error_over_bound", ratio)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("model", MODELS, ids=lambda m: NAMES[m])
def test_eval_grid_stride(gpu, model, record_property):
    """More chains than eval_kernel's grid (num_cus * 8): every workgroup takes several chains in turn."""
    import torch

    C = max(5000, torch.cuda.get_device_properties(0).multi_processor_count * 8 + 123)
    ratio, _ = eval_case(model, 6, C, wa.default_config(), seed=11)
    record_property("max_error_over_bound", ratio)


def transitions_then_logp(model, D, C, cfg, data=None, params=None):
    e = wa.DeviceEngine(model, D, C, cfg, params=params, data=data)
    e.init_positions(seed=31, chain_offset=0, scale=0.5)
    e.init_masses_from_grad(1e-5)
    e.adapt_step(seed=32)
    for _ in range(3):
        e.warmup_step()
    e.freeze()
    e.sample_step()
    e.check()
    lp_stored, pos, streaming, held = e.logp(), e.positions(), e.streaming, e.held_tiles
    lp_eval = e.logp_grad(pos)[0]
    e.close()
    return lp_stored, lp_eval, streaming, held


# one geometry per kernel family: register NW = 1, register NW > 1, streaming, held streaming (the default past the
# register kernels' limit)
FAMILIES = {"register_nw1": (1000, dict(waves_per_chain=1, elems_per_lane=16)),
            "register_nw4": (2000, dict(waves_per_chain=4, elems_per_lane=8)),
            "streaming_nw4": (300, dict(waves_per_chain=4, elems_per_lane=-1)),
            "held_streaming": (5000, {})}


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("model", MODELS, ids=lambda m: NAMES[m])
def test_eval_equals_transition_logp(gpu, model, family, fma):
    """wn_init.h: eval evaluates "the same expressions a transition evaluates" -- so at the positions the chains hold,
    the density it returns is the one the last transition stored, bit for bit."""
    D, kw = FAMILIES[family]
    if family == "held_streaming" and model == FUNNEL:
        D = 9000  # (the funnel's register kernels serve up to 8 192 by default)
    cfg = wa.default_config(fused_multiply_add=fma, **kw)
    lp_stored, lp_eval, streaming, held = transitions_then_logp(model, D, 16, cfg, params=params_for(model, D, 3))
    assert streaming == ("streaming" in family)
    assert np.all(np.isfinite(lp_stored))
    assert np.array_equal(lp_stored, lp_eval), (np.abs(lp_stored - lp_eval) / np.abs(lp_stored)).max()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fma", [0, 1])
@pytest.mark.parametrize("model", [LIN, LOG], ids=lambda m: NAMES[m])
def test_eval_equals_transition_logp_data_models(gpu, model, fma):
    """The same for the data models (register kernels, one wavefront per chain: the only family they run on)."""
    from test_data_models_sim import make_data

    for D, N in ((20, 37), (1000, 33)):
        x, y, s2 = make_data(model, D, N, seed=D + N)
        lp_stored, lp_eval, _, _ = transitions_then_logp(model, D, 16, wa.default_config(fused_multiply_add=fma),
                                                         data=(x, y), params=s2)
        assert np.all(np.isfinite(lp_stored))
        assert np.array_equal(lp_stored, lp_eval), (D, N)
