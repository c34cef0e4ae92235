"""The register kernels' merge path between two leaf pairs (wn_chip.h: the pool-side U-turn test with both operand halves
in flight, the pop split around its loads, the merge's decision taken in front of the test's branch with the draw looked
at and not yet taken): bit for bit against the device-order oracle, on the CPU emulation and -- the same cases, -m gpu --
on the device.

Every case runs the oracle ONCE (single steps, traced) and the engine once per way of cutting the same sampling
transitions into launches.  The oracle's trace, its draw counts and its depths say how often the paths under test were
taken -- cascades of two and more pool-side merges, pool-side tests that turned, top-level tests that turned -- and every
case asserts that they were."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpusim"))
import build as simbuild  # noqa: E402
import parity  # noqa: E402

CHAINS = 8
SAMPLING = 9
MAX_DEPTH = 5   # max_trajectory_doublings of every case (the default)
MIN_EVENTS = 5


@pytest.fixture(scope="module")
def sim_lib(oracle):
    return simbuild.build()


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


def trailing_zeros(k):
    return (k & -k).bit_length() - 1


def merge_events(trace, draws, depth):
    """Events of one chain-transition from the oracle's macro-step trace (one record per attempt: [6] within the energy
    bound, [7] reversible; leaves are the accepted attempts, doubling d is the next 2^(d-1) of them), the number of tree
    draws the transition took and its depth (the doubling the tree stopped in, MAX_DEPTH + 1 if it never did).

    Draws: one per doubling (its direction), one per merge inside the new span (k leaves in popcount(k) spans took
    k - popcount(k) merges) and one per finished extension (the Metropolis draw of the top-level merge).  A last
    extension whose last leaf was accepted and that took no Metropolis draw was ended by a U-turn test inside it: that
    test's span ends at leaf k and spans 2^L leaves (L = 1 rides in the leaf pair, L >= 2 is a pool-side test); the
    merges of levels L and above at leaf k -- and their draws -- did not happen, so the draw count gives L.
    Worked example: leaves per doubling [1, 2, 4, 8], last leaf accepted, 20 draws.  Doublings 1-3 finished: 2 + 3 + 5 =
    10 draws.  The fourth has all of its k = 8 leaves, but 10 draws are not the k + 1 = 9 of a finished extension, so a
    test inside it turned.  Its direction took 1 draw, so 9 merges drew; 8 leaves without a turn merge 8 - 1 = 7 times
    ... no more than 7 can be missing: here 1 + 7 - 10 = -2 is impossible and the asserts below fail.  With 7 draws
    instead: missing = 1 + 7 - 7 = 1 merge, trailing_zeros(8) = 3 levels end at leaf 8, so the test of level
    L = 3 + 1 - 1 = 3 (the whole new span, a pool-side test) turned after the merges of levels 1 and 2: one pool-side
    merge done in that cascade, one pool-side test that turned.
    -> (cascades with two or more pool-side merges, pool-side tests that turned, top-level tests that turned)"""
    leaves = []   # accepted leaves per doubling
    have, want, open_ = 0, 1, False
    for r in trace:
        if not open_:
            open_, have = True, 0
        if r[6] > 0.5 and r[7] > 0.5:
            have += 1
            if have == want:
                leaves.append(have)
                open_, want = False, want * 2
    if open_:
        leaves.append(have)
    last_leaf_ok = trace[-1][6] > 0.5 and trace[-1][7] > 0.5
    cascades = pool_turned = 0
    finished = True   # the last extension
    taken = 0
    for d, k in enumerate(leaves):
        merges = k - bin(k).count("1")
        turned_level = 0   # the level of the test that ended this extension (0: none did)
        if d < len(leaves) - 1 or (k == 1 << d and draws - taken == k + 1):
            taken += 1 + merges + 1
        elif not last_leaf_ok:   # a leaf failed
            finished = False
            taken += 1 + merges
        else:
            finished = False
            assert k >= 2 and k % 2 == 0, (leaves, draws)
            missing = 1 + merges - (draws - taken)
            turned_level = trailing_zeros(k) + 1 - missing
            assert 1 <= turned_level <= trailing_zeros(k), (leaves, draws, turned_level)
            taken = draws
            pool_turned += turned_level >= 2
        for m in range(8, k + 1, 8):   # the cascade behind leaf m: pool-side merges of levels 2 .. trailing_zeros(m)
            done = trailing_zeros(m) - 1
            if m == k and turned_level:
                done = turned_level - 2
            cascades += done >= 2
    assert taken == draws, (leaves, draws, taken)
    assert depth == (len(leaves) if not finished or depth <= MAX_DEPTH else MAX_DEPTH + 1), (leaves, depth)
    # the tree stopped growing behind a finished extension: the top-level test turned (from the second doubling on it is
    # the test of the top-level merge; the first doubling's rides in its single leaf)
    top_turned = int(finished and depth == len(leaves) >= 2)
    return cascades, pool_turned, top_turned


def setup(dev, orc, C, D, seed, step, warmup):
    pos = np.random.default_rng(seed).normal(0.0, 2.0, size=(C, D))
    for x in (dev, orc):
        x.set_positions(pos)
        x.init_masses_from_grad(1e-5)
        x.set_step_sizes(step)
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
    ev = dict(cascades=0, pool_turned=0, top_turned=0, deep=0)
    for _ in range(SAMPLING):
        orc.sample_step(8)
        snaps.append(Snapshot(orc))
        draws, depths = orc.rng_draws(), orc.depths()
        for c in range(orc.C):
            cas, pool, top = merge_events(orc.trace(c), int(draws[c]), int(depths[c]))
            ev["cascades"] += cas
            ev["pool_turned"] += pool
            ev["top_turned"] += top
        ev["deep"] += int(np.sum(orc.depths() >= 4))
    _ORACLE_RUNS[key] = (snaps, ev)
    return snaps, ev


def run(lib, model, D, geometry, fma, lds_vectors, step, seed, tpl):
    cfg = {} if lds_vectors is None else dict(lds_vectors=lds_vectors)
    key = (model, D, geometry, fma, step, seed)   # (where the pool's vectors live changes no result)
    dev, orc = parity.make_pair(model, D, CHAINS, lib, geometry, fused_multiply_add=fma, **cfg)
    setup(dev, orc, CHAINS, D, seed, step, warmup=2)
    # (the oracle is set up and warmed up with the engine every time -- the warmup is compared --; only its SAMPLING steps
    # are run once per key and shared, also between the tiers and the pool's tiers)
    snaps, ev = oracle_run(key, orc)
    it = 0
    while it < SAMPLING:
        n = min(tpl, SAMPLING - it)
        if lib is None:
            import torch

            rows = torch.full((n, CHAINS, D), float("nan"), dtype=torch.float64, device="cuda")
            dev.sample_steps(n, rows.data_ptr(), D, CHAINS * D)
            dev.synchronize()
            rows = rows.cpu().numpy()
        else:
            rows = np.full((n, CHAINS, D), np.nan)
            dev.sample_steps(n, rows.ctypes.data, D, CHAINS * D)
            dev.synchronize()
        for k in range(n):   # every transition's draw, also inside a launch
            assert np.array_equal(rows[k], snaps[it + k].positions()), f"draw of transition {it + k} (launch of {n})"
        it += n
        # positions, log densities, depths, gradient evaluations and the number of draws taken: a draw looked at and
        # taken by a test that turned would show in the last
        parity.assert_same_state(dev, snaps[it - 1], f"{model} D={D} launches of {tpl}, after transition {it - 1}",
                                 warm=False)
    return ev


# (model, dimensions, geometry or None = the engine's choice, fused multiply-add, lds_vectors or None = the default,
#  initial step size, seed).  Pool-side tests that turn are rare in these models (a new span is never longer than the
# tree it is added to, whose top-level test did not turn): steps and seeds were searched for on the oracle alone until
# it showed EVERY event at least MIN_EVENTS times over the 8 chains x 9 transitions, and are frozen.
CASES = [
    # the headline kernel (the span's other end parked in accumulator registers), both arithmetic modes
    ("std_normal", 1024, (1, 16), 1, 4, 0.1, 389),
    ("std_normal", 1024, (1, 16), 0, 4, 0.1, 389),
    # padding lanes
    ("std_normal", 1000, (1, 16), 1, 4, 0.1, 194),
    ("std_normal", 1000, (1, 16), 0, 4, 0.1, 194),
    # two wavefronts per chain, 8 elements per lane: one half, the sums go through the cross-wave reduction
    ("std_normal", 1024, (2, 8), 1, 4, 0.1, 389),
    ("std_normal", 1024, (2, 8), 0, 4, 0.1, 389),
    # 8 elements per lane, one wavefront: the operands are one half -- the shape that did not change
    ("std_normal", 512, (1, 8), 1, 4, 0.1, 10),
    ("std_normal", 512, (1, 8), 0, 4, 0.1, 10),
    # the pool's other tier: one LDS vector (operands mixed), none (every operand from the arena)
    ("std_normal", 1024, (1, 16), 1, 1, 0.1, 389),
    ("std_normal", 1024, (1, 16), 1, 0, 0.1, 389),
    # a model with parameters, and one that keeps its gradient (the top-level test is a pool-side test there)
    ("diag_normal", 1024, (1, 16), 1, 4, 0.12, 155),
    ("funnel", 128, None, 1, None, 0.05, 15),
]


def cases():
    out = []
    for tier in ("sim", "gpu"):
        for case in CASES:
            out.append(pytest.param(tier, *case, marks=[pytest.mark.gpu] if tier == "gpu" else []))
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tpl", [1, 8])
@pytest.mark.parametrize("tier,model,D,geometry,fma,lds_vectors,step,seed", cases())
def test_merge_path(lib_of, tier, model, D, geometry, fma, lds_vectors, step, seed, tpl):
    """9 sampling transitions of 8 chains in launches of 1 and of 8 (+ 1): every draw, and positions, log densities,
    depths, gradient evaluations and draw counts after every launch, are the oracle's.  Most trees reach depth 4-5, so
    cascades merge two and more levels; pool-side and top-level tests turn -- the oracle's trace says how often, and
    fewer than MIN_EVENTS of any is a failure of the case."""
    ev = run(lib_of(tier), model, D, geometry, fma, lds_vectors, step, seed, tpl)
    print(ev)
    assert ev["cascades"] >= MIN_EVENTS, ev
    assert ev["pool_turned"] >= MIN_EVENTS, ev
    assert ev["top_turned"] >= MIN_EVENTS, ev
    assert ev["deep"] >= CHAINS * SAMPLING // 2, ev
