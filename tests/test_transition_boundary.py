"""The register kernels' transition boundary and turn-around (wn_chip.h: the top-level U-turn test's operands stay in
set 1 for a turn-around of the next doubling): bit for bit against the device-order oracle, on the CPU emulation and --
the same cases, -m gpu -- on the device.

Every case runs the oracle ONCE (single steps, traced) and the engine once per way of cutting the same sampling
transitions into launches; the oracle's trace says how often the paths under test were taken, and the cases assert that
they were."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpusim"))
import build as simbuild  # noqa: E402
import parity  # noqa: E402

SAMPLING = 9
TIERS = ["sim", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture(scope="module")
def sim_lib(oracle):
    return simbuild.build()


@pytest.fixture(params=TIERS)
def lib(request):
    """-> the library the engine is built from: the emulation's path, or None = the HIP library on the GPU."""
    if request.param == "sim":
        return request.getfixturevalue("sim_lib")
    request.getfixturevalue("gpu")
    return None


def tiered(cases):
    """[(tier or None = both, case...)] -> parameters (lib, case...); the device's cases carry the gpu mark"""
    out = []
    for tier, *case in cases:
        for t in ("sim", "gpu"):
            if tier in (None, t):
                out.append(pytest.param(t, *case, marks=[pytest.mark.gpu] if t == "gpu" else []))
    return out


@pytest.fixture
def lib_of(request):
    def get(tier):
        if tier == "sim":
            return request.getfixturevalue("sim_lib")
        request.getfixturevalue("gpu")
        return None
    return get


class Snapshot:
    """What parity.assert_same_state reads of an oracle, kept from one of its transitions."""

    def __init__(self, orc):
        self._v = dict(positions=orc.positions(), logp=orc.logp(), depths=orc.depths(), grad_evals=orc.grad_evals(),
                       rng_draws=orc.rng_draws())

    def __getattr__(self, name):
        return lambda: self._v[name]


def tree_events(trace):
    """Events of one chain-transition from the oracle's macro-step trace (one record per attempt: [0] forward, [6] within
    the energy bound, [7] reversible).  Leaves are the accepted attempts; doubling d is the next 2^(d-1) of them (the
    last doubling may be cut short), and its direction is its first attempt's.
    -> (turn-arounds, turn-around directly after the first doubling, doublings begun)"""
    # (a doubling opens at its first attempt and closes when it has all its leaves; dirs: one direction per doubling)
    dirs, have, want, open_ = [], 0, 1, False
    for r in trace:
        if not open_:
            dirs.append(r[0] > 0.5)
            open_, have = True, 0
        if r[6] > 0.5 and r[7] > 0.5:
            have += 1
            if have == want:
                open_, want = False, want * 2
    turns = sum(1 for a, b in zip(dirs, dirs[1:]) if a != b)
    return turns, len(dirs) >= 2 and dirs[0] != dirs[1], len(dirs)


def setup(dev_or_orc_pair, C, D, seed, step, warmup):
    dev, orc = dev_or_orc_pair
    pos = np.random.default_rng(seed).normal(0.0, 2.0, size=(C, D))
    for x in (dev, orc):
        x.set_positions(pos)
        x.init_masses_from_grad(1e-5)
        x.set_step_sizes(1.0 if step is None else step)
    if step is None:
        dev.adapt_step(seed, 11)
        orc.adapt_step(seed, 11)
    for x in (dev, orc):
        x.seed_chains(seed + 1, 3)
    for _ in range(warmup):     # (adaptive transitions: the frozen inverse mass is not the unit one)
        dev.warmup_step()
        orc.warmup_step(8)
    parity.assert_same_state(dev, orc, "warmup", warm=True)
    dev.freeze()
    orc.freeze()


_ORACLE_RUNS = {}


def oracle_run(key, orc):
    """The oracle's SAMPLING single steps of a case, run once: per-transition snapshots and event counts."""
    if key in _ORACLE_RUNS:
        return _ORACLE_RUNS[key]
    orc.enable_trace(True)
    snaps = []
    ev = dict(turned=0, turned_after_first=0, turned_selection_other=0, depth_one=0)
    for _ in range(SAMPLING):
        before = orc.positions()
        orc.sample_step(8)
        snaps.append(Snapshot(orc))
        after = orc.positions()
        for c in range(orc.C):
            turns, after_first, begun = tree_events(orc.trace(c))
            ev["turned"] += turns >= 1
            ev["turned_after_first"] += after_first
            # the selection is the initial point at the end, so it was at every turn-around: a selection that moved
            # never comes back to the span's other end
            ev["turned_selection_other"] += turns >= 1 and np.array_equal(before[c], after[c])
            ev["depth_one"] += begun == 1
    _ORACLE_RUNS[key] = (snaps, ev)
    return snaps, ev


def run(lib, model, D, C, geometry, *, tpl, seed=1234, step=None, warmup=2, fma=1, **cfg):
    ocfg = {k: v for k, v in cfg.items() if k not in ("workgroups_per_cu", "chain_groups")}
    key = (model, D, C, geometry, seed, step, warmup, fma, tuple(sorted(ocfg.items())))
    dev, orc = parity.make_pair(model, D, C, lib, geometry, fused_multiply_add=fma, **cfg)
    setup((dev, orc), C, D, seed, step, warmup)
    snaps, ev = oracle_run(key, orc)
    it = 0
    while it < SAMPLING:
        n = min(tpl, SAMPLING - it)
        if lib is None:
            import torch

            rows = torch.full((n, C, D), float("nan"), dtype=torch.float64, device="cuda")
            dev.sample_steps(n, rows.data_ptr(), D, C * D)
            dev.synchronize()
            rows = rows.cpu().numpy()
        else:
            rows = np.full((n, C, D), np.nan)
            dev.sample_steps(n, rows.ctypes.data, D, C * D)
            dev.synchronize()
        for k in range(n):   # every transition's draw, also inside a launch
            assert np.array_equal(rows[k], snaps[it + k].positions()), f"draw of transition {it + k} (launch of {n})"
        it += n
        parity.assert_same_state(dev, snaps[it - 1], f"{model} D={D} launches of {tpl}, after transition {it - 1}",
                                 warm=False)
    return dev, ev


# ---- the launch boundary: 9 x 1, 4 x 2 + 1, 3 x 3, 8 + 1 --------------------------------------------------------------
# (first column: the tier that runs the row -- the emulation is built with a cross-section of the geometries, (1, 8),
# (1, 16) and (2, 8) among them -- or None for both)
GEOMETRIES = tiered([
    (None, "std_normal", 1024, (1, 16), 1),    # the headline kernel: the other end parked in accumulator registers
    (None, "std_normal", 1024, (1, 16), 0),
    (None, "diag_normal", 1024, (1, 16), 1),   # config #2's kernel
    (None, "diag_normal", 1024, (1, 16), 0),
    ("gpu", "std_normal", 512, (1, 8), 1),     # two wavefronts per SIMD, still parked
    ("gpu", "diag_normal", 2048, (2, 16), 1),  # two wavefronts per chain: barriers around the top-level reduction
    (None, "diag_normal", 1024, (2, 8), 1),    # ... with 8 elements per lane
    (None, "std_normal", 1000, (1, 16), 1),    # padding lanes: their momentum is zero
    (None, "diag_normal", 1000, (1, 16), 0),
    ("sim", "std_normal", 512, (1, 8), 1),     # (the emulated half of the (1, 8) row above)
])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tpl", [1, 2, 3, 8])
@pytest.mark.parametrize("tier,model,D,geometry,fma", GEOMETRIES)
def test_launch_boundaries_and_turn_arounds(lib_of, tier, model, D, geometry, fma, tpl):
    """The same 9 sampling transitions cut into launches of 1, 2, 3 and 8 (the last launch short): every draw, and the
    scalars after every launch, are the oracle's -- so the four are each other's.  The trees turn around, also directly
    after the first doubling."""
    _, ev = run(lib_of(tier), model, D, 8, geometry, tpl=tpl, fma=fma)
    print(ev)
    assert ev["turned"] >= 5 and ev["turned_after_first"] >= 5, ev


# ---- turn-arounds with the selection still on the other end; trees that end at depth 1 ---------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("tpl", [1, 8])
@pytest.mark.parametrize("max_depth,event", [(2, "turned_selection_other"), (1, "depth_one"), (3, "turned_selection_other")])
def test_short_trees(lib, max_depth, event, tpl):
    """max_trajectory_doublings 1: the tree ends after the first doubling and the selection may be the parked initial
    point; 2 and 3: a turn-around directly after the first doubling, often with the selection still the other end's
    (it then gets a pool buffer from set 1).  A larger step than the adapted one: more rejected proposals."""
    _, ev = run(lib, "std_normal", 1024, 64, (1, 16), tpl=tpl, seed=77, step=0.45, max_trajectory_doublings=max_depth)
    print(ev)
    assert ev[event] >= 5, ev
    if max_depth > 1:
        assert ev["turned_after_first"] >= 5, ev


# ---- chains handed over inside a launch -------------------------------------------------------------------------------
@pytest.mark.timeout(900)
@pytest.mark.parametrize("chain_groups", [1, 2])
def test_chain_hand_over(lib, chain_groups):
    """Every workgroup runs several chains per launch, each for all of the launch's transitions: nothing of a chain's
    last transition reaches the next chain's first one."""
    C = 40 if lib is not None else 4096
    dev, ev = run(lib, "std_normal", 1024, C, (1, 16), tpl=3, seed=5, workgroups_per_cu=1, chain_groups=chain_groups)
    assert C >= 3 * dev.workgroups, (C, dev.workgroups)
    assert ev["turned"] >= 5, ev


# ---- rare paths: halvings, the reversibility check, failed extensions ---------------------------------------------------
@pytest.mark.timeout(900)
def test_halvings_and_failed_extensions(lib):
    """A step far too large: leaves halve their step, run the reversibility check and fail -- an extension that fails
    ends the tree while set 1 carries the span's other end."""
    parity.run_case("std_normal", 64, 64, warmup=0, sampling=6, step=2.9, max_trajectory_doublings=4, check_every=3,
                    lib_path=lib)
    dev, _ = parity.run_case("std_normal", 1024, 8, warmup=0, sampling=6, step=1.9, max_trajectory_doublings=4,
                             check_every=3, lib_path=lib, geometry=(1, 16), fused=3)
    assert dev.grad_evals().sum() > 0


# ---- host-fed variates: one transition per launch -----------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_host_fed_variates(lib):
    dev, orc = parity.make_pair("std_normal", 1024, 6, lib, (1, 16))
    rng = np.random.default_rng(5)
    pos = rng.normal(size=(6, 1024))
    for x in (dev, orc):
        x.set_positions(pos)
        x.set_step_sizes(0.25)
        x.seed_chains(1, 0)
        x.freeze()
    for it in range(4):
        z, u = rng.normal(size=(6, 1024)), rng.uniform(size=(6, 64))
        for x in (dev, orc):
            x.set_variates(z, u)
            x.sample_step()
        parity.assert_same_state(dev, orc, f"variates sampling {it}", warm=False)
    for _ in range(2):      # and back to the counter-based stream, fused
        dev.sample_steps(3)
        for _ in range(3):
            orc.sample_step()
    parity.assert_same_state(dev, orc, "fused launches after host-fed transitions", warm=False)


# ---- warmup kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_warmup_kernel(lib):
    parity.run_pending_observation_case("std_normal", 1024, 6, lib_path=lib, geometry=(1, 16))
