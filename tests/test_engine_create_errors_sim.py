"""CPU tier: the refusals of wn_engine_create / wn_engine_create_observed, through the C ABI itself (the Python layer
checks shapes of its own first and would hide most of them).  Every refusal is a `config` error with a fixed text; where
two checks would both fire, the first in the documented order wins.  The host source is the same for the HIP build.

What test_data_models_sim.py, test_datasets_sim.py, test_weights_sim.py and test_hier_models_sim.py already pin with
their full text (the weight-set and obs_offsets checks, non-finite x / y / offset / weight, "reads no data", the
"dataset g: " prefix, "one wavefront per chain") is not repeated here.  Not reachable with the in-tree models: "reads no
offsets or weights" (every data model declares kUsesRowTerms)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "cpusim"))
import build as simbuild  # noqa: E402
import walnuts_amd as wa  # noqa: E402

STD, DIAG, FUNNEL = wa.MODEL_STD_NORMAL, wa.MODEL_DIAG_NORMAL, wa.MODEL_FUNNEL
LIN, LOG, SIGMA = wa.MODEL_LINEAR_REGRESSION, wa.MODEL_LOGISTIC_REGRESSION, wa.MODEL_LINEAR_REGRESSION_SIGMA
HLIN = wa.MODEL_HIER_LINEAR_REGRESSION
CONFIG = 1  # WalnutpyErrorType: config
D, N, J = 5, 4, 2  # parameters, observations, groups (a grouped model's x then has P = D - J - 1 = 2 columns)
NULL = object()  # a null pointer where the default would be an array


@pytest.fixture(scope="module")
def sim():
    return simbuild.build()


@pytest.fixture(scope="module")
def create(sim):
    """create(model, ...) -> None if the engine was built (and destroyed again), else (error type, message)."""
    lib = wa._ffi.load_library(sim)
    dp, i32p, i64p = wa._ffi._dp, wa._ffi._i32p, wa._ffi._i64p

    def run(model, num_params=D, chains=2, params=None, observed=True, cfg=None, null_out=False, null_cfg=False,
            x=None, y=None, num_obs=N, group=None, num_groups=0, obs_offsets=None, num_datasets=0, offset=None,
            weight=None, num_weight_sets=0):
        keep = []

        def ptr(a, dtype, ctype):
            if a is None or a is NULL:
                return None
            keep.append(np.ascontiguousarray(a, dtype=dtype))
            return keep[-1].ctypes.data_as(ctype)

        h, err = C.c_void_p(), C.c_void_p()
        config = wa.default_config(sim, **(cfg or {}))
        out = None if null_out else C.byref(h)
        cfgp = None if null_cfg else C.byref(config)
        pp = ptr(np.ones(max(num_params, 1)) if params is None else params, np.float64, dp)
        if observed is True:
            obs = wa._ffi.Observations(
                x=ptr(np.zeros((N, D)) if x is None else x, np.float64, dp), y=ptr(np.zeros(N) if y is None else y, np.float64, dp),
                num_obs=num_obs, group=ptr(group, np.int32, i32p), num_groups=num_groups,
                obs_offsets=ptr(obs_offsets, np.int64, i64p), num_datasets=num_datasets, offset=ptr(offset, np.float64, dp),
                weight=ptr(weight, np.float64, dp), num_weight_sets=num_weight_sets)
            rc = lib.wn_engine_create_observed(out, model, num_params, pp, C.byref(obs), chains, cfgp, C.byref(err))
        elif observed is NULL:
            rc = lib.wn_engine_create_observed(out, model, num_params, pp, None, chains, cfgp, C.byref(err))
        else:
            rc = lib.wn_engine_create(out, model, num_params, pp, chains, cfgp, C.byref(err))
        if rc == 0:
            lib.wn_engine_destroy(h)
            return None
        assert not h.value  # a refusal hands no engine out
        msg = lib.walnutpie_get_error_message(err).decode()
        kind = lib.walnutpie_get_error_type(err)
        lib.walnutpie_destroy_error(err)
        return kind, msg

    return run


GROUPS = [0, 1, 1, 0]
GROUPED_NEEDS = ("a grouped model needs num_params == P + num_groups + 1 with P >= 1 and num_groups >= 1, got num_params "
                 "{}, num_groups {}")

# (arguments of create(), the message)
CASES = [
    # ---- the entry points' own arguments
    (dict(model=STD, observed=False, null_out=True), "null argument"),
    (dict(model=STD, observed=False, null_cfg=True), "null argument"),
    (dict(model=LIN, null_out=True), "null argument"),
    (dict(model=LIN, null_cfg=True), "null argument"),
    (dict(model=LIN, observed=NULL), "null argument"),
    # ---- sizes, the model id, the configuration
    (dict(model=STD, observed=False, num_params=0), "num_params must be positive"),
    (dict(model=STD, observed=False, num_params=-3), "num_params must be positive"),
    (dict(model=STD, observed=False, chains=0), "num_chains must be positive"),
    (dict(model=63, observed=False), "unknown device model id"),
    (dict(model=-1, observed=False), "unknown device model id"),
    (dict(model=64, observed=False), "unknown device model id"),
    (dict(model=STD, observed=False, cfg=dict(max_trajectory_doublings=0)), "max_nuts_depth must be positive"),
    (dict(model=STD, observed=False, cfg=dict(max_trajectory_doublings=18)),
     "max_trajectory_doublings exceeds the device span stack"),
    (dict(model=STD, observed=False, cfg=dict(max_step_halvings=0)), "max_step_halvings must be positive"),
    (dict(model=STD, observed=False, cfg=dict(min_micro_steps=0)), "min_micro_steps must be positive"),
    (dict(model=STD, observed=False, cfg=dict(max_hamiltonian_error=0.0)),
     "max_hamiltonian_error must be positive and finite"),
    (dict(model=STD, observed=False, cfg=dict(max_hamiltonian_error=float("inf"))),
     "max_hamiltonian_error must be positive and finite"),
    (dict(model=STD, observed=False, cfg=dict(max_hamiltonian_error=float("nan"))),
     "max_hamiltonian_error must be positive and finite"),
    # ---- what the model asks for
    (dict(model=DIAG, observed=False, params=NULL), "diag_normal model needs a parameter vector of num_params doubles"),
    (dict(model=FUNNEL, observed=False, num_params=1), "funnel needs num_params >= 2"),
    (dict(model=LOG, observed=False),
     "logistic_regression model is conditioned on data: create it with wn_engine_create_observed (x [num_obs]"
     "[num_params], y [num_obs])"),
    (dict(model=SIGMA, observed=False),
     "linear_regression_sigma model is conditioned on data: create it with wn_engine_create_observed (x [num_obs]"
     "[num_params - 1], y [num_obs])"),
    (dict(model=HLIN),
     "hier_linear_regression model reads a group per observation: create it with wn_engine_create_observed (x [num_obs]"
     "[num_params - num_groups - 1], y, group [num_obs] in [0, num_groups))"),
    (dict(model=LIN, group=GROUPS, num_groups=J), "linear_regression model reads no groups (it does not declare kUsesGroups)"),
    # ---- a grouped model's sizes
    (dict(model=HLIN, group=GROUPS, num_groups=0), GROUPED_NEEDS.format(5, 0)),
    (dict(model=HLIN, group=GROUPS, num_groups=-1), GROUPED_NEEDS.format(5, -1)),
    (dict(model=HLIN, group=GROUPS, num_groups=4), GROUPED_NEEDS.format(5, 4)),
    # ---- the observation block
    (dict(model=LIN, num_obs=0), "num_obs must be positive"),
    (dict(model=LIN, num_obs=-2), "num_obs must be positive"),
    (dict(model=LIN, obs_offsets=[0, 1 << 31], num_datasets=1), "a dataset holds more than 2^31 - 1 observations"),
    (dict(model=LIN, obs_offsets=[0, 2, (1 << 31) + 2], num_datasets=2), "a dataset holds more than 2^31 - 1 observations"),
    (dict(model=LIN, x=NULL), "null data argument"),
    (dict(model=LIN, y=NULL), "null data argument"),
    (dict(model=LIN, x=NULL, obs_offsets=[0, 2, 4], num_datasets=2), "null data argument"),
    (dict(model=HLIN, group=[0, 1, 1, 2], num_groups=J), "every group must be in [0, num_groups), observation 3 has 2"),
    (dict(model=HLIN, group=[0, -1, 1, 0], num_groups=J), "every group must be in [0, num_groups), observation 1 has -1"),
    (dict(model=HLIN, group=[0, 1, 7, 0], num_groups=J, obs_offsets=[0, 2, 4], num_datasets=2),
     "every group must be in [0, num_groups), observation 2 has 7"),
]

X_INF = np.zeros((N, D))
X_INF[2, 1] = np.inf
W_NAN = np.ones(N)
W_NAN[0] = np.nan
# Two checks would both fire: the one that comes first in build_engine's order gives the message
ORDER_CASES = [
    # the configuration before the model's needs
    (dict(model=LOG, observed=False, cfg=dict(max_step_halvings=0)), "max_step_halvings must be positive"),
    # the sizes before the registry's model lookup
    (dict(model=63, observed=False, num_params=0), "num_params must be positive"),
    # data the model does not read, before a group it does not read either
    (dict(model=STD, group=GROUPS, num_groups=J), "std_normal model reads no data (it does not declare kUsesData)"),
    # weight sets: the sign, then the missing weights, then obs_offsets, then the chain count
    (dict(model=LIN, num_weight_sets=-1, num_obs=0), "num_weight_sets must not be negative"),
    (dict(model=LIN, num_weight_sets=2, obs_offsets=[0, 2, 4], num_datasets=2),
     "num_weight_sets > 1 needs weight [num_weight_sets][num_obs]"),
    (dict(model=LIN, num_weight_sets=2, weight=np.ones((2, N)), obs_offsets=[0, 2, 4], num_datasets=2, chains=3),
     "weight sets share one block of rows: not with obs_offsets (several datasets)"),
    # the weight sets before a grouped model's sizes, those before the row counts, those before the null pointers
    (dict(model=HLIN, group=GROUPS, num_groups=0, num_weight_sets=-1), "num_weight_sets must not be negative"),
    (dict(model=HLIN, group=GROUPS, num_groups=0, num_obs=0), GROUPED_NEEDS.format(5, 0)),
    (dict(model=LIN, num_obs=0, x=NULL), "num_obs must be positive"),
    # x before the groups before the weights
    (dict(model=HLIN, x=X_INF[:, :2], group=[0, 1, 1, 2], num_groups=J), "data x must be finite"),
    (dict(model=HLIN, group=[0, 1, 1, 2], num_groups=J, weight=W_NAN),
     "every group must be in [0, num_groups), observation 3 has 2"),
    # every element-wise check before the model's own look at the data
    (dict(model=LOG, y=[0.0, 0.5, 1.0, 0.0], weight=W_NAN), "every weight must be finite and >= 0, observation 0 has nan"),
]


@pytest.mark.parametrize("kw,msg", CASES + ORDER_CASES, ids=lambda v: None if isinstance(v, dict) else v[:60])
def test_create_refusal(create, kw, msg):
    assert create(**kw) == (CONFIG, msg)


def test_failed_registration_is_reported_by_create(sim, create):
    """A device model that failed to register (wn_plugin_register_model) is reported by the next engine, whatever its
    model, ahead of the model lookup and of every configuration check; clearing the error lifts it."""
    lib = wa._ffi.load_library(sim)
    assert lib.wn_plugin_register_model(None, None) == -1
    try:
        text = lib.wn_model_error().decode()
        assert "compiled against other headers than this library" in text
        assert create(model=STD, observed=False) == (CONFIG, text)
        assert create(model=63, observed=False, cfg=dict(max_step_halvings=0)) == (CONFIG, text)
        assert create(model=STD, observed=False, chains=0) == (CONFIG, "num_chains must be positive")
    finally:
        lib.wn_model_clear_error()
    assert create(model=STD, observed=False) is None


def test_the_smallest_valid_inputs_are_accepted(create):
    """The inputs the refusals above start from are themselves valid: every case differs from these in what it names."""
    assert create(model=STD, observed=False) is None
    assert create(model=LIN) is None
    assert create(model=LIN, obs_offsets=[0, 2, 4], num_datasets=2) is None
    assert create(model=LIN, weight=np.ones((2, N)), num_weight_sets=2) is None
    assert create(model=HLIN, x=np.zeros((N, 2)), group=GROUPS, num_groups=J) is None
