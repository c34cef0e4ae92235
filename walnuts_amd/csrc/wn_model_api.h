// wn_model_api.h -- the interface a device model implements.
//
// The reference's model contract is `logp_grad(theta) -> (logp, grad)` (LogpGrad, concepts.hpp:258-262; C form
// LOGP_CFUNC, python/src/walnutpie/walnutpy.cpp:131-132).  A host function cannot be called from a GPU-resident
// trajectory, so here the model is a struct of static device functions that the kernels are instantiated with.  One
// workgroup of L = 64 * NW lanes evaluates one chain; lane `tid` holds EPL coordinates of every vector, slot j of it
// being coordinate cx.index(j) (pairs of consecutive coordinates, pair m = k * L + tid).
//
//   struct MyModel {
//     static constexpr bool kUsesParams;      // a parameter vector of num_params doubles exists (arrives as `mp`,
//                                             //   padded with 1.0); wn_engine_create requires it then
//     static constexpr bool kElementwise;     // grad[i] depends on theta[i] (and mp[i]) only: the streaming kernels (the
//                                             //   default above 4 096 parameters) then take ONE pass per micro step; needs grad()
//                                             //   below (other models: the optional streaming form further down)
//     static constexpr bool kCheapGrad;       // grad_elem() is one or two operations: the kernels then store no
//                                             //   gradient vector at all and call grad_elem() at each use
//     static constexpr bool kGradIsNegTheta;  // (informational) grad == -theta
//     static double grad_elem(double theta_i, double mp_i);     // used only when kCheapGrad
//     struct Aux { ... };                     // wave-uniform by-products of eval() that finish() wants
//
//     // Write the gradient of the lane's coordinates to g and ADD the lane's log-density terms, in slot order, to
//     // `acc`.  The kernels sum `acc` over the chain in a fixed order (lane partials, butterfly, wavefronts left to
//     // right) and hand the total to finish().  Padding slots (!cx.valid(j)) must leave g[j] = 0 and add nothing.
//     template <int EPL, class Cx>
//     static void eval(Cx& cx, const double (&theta)[EPL], double (&g)[EPL], const double (&mp)[EPL], Aux&, double& acc);
//     template <int EPL, class Cx>            // kElementwise only: the gradient alone, same expression as in eval()
//     static void grad(Cx& cx, const double (&theta)[EPL], double (&g)[EPL], const double (&mp)[EPL], Aux&);
//     static double finish(double sum, const Aux&, int num_params);   // -> logp
//
//     // optional -- "Streaming a model whose gradient is not element-wise": above 8 192 parameters (4 096 by default
//     // where the kernels that hold the trajectory's moving end in registers apply) the span pool lives in HBM and
//     // vectors are processed two coordinates at a time, so eval() (which sees the lane's whole share at once) cannot
//     // run.  A model states what its gradient needs beyond the coordinate itself, and gets two passes per micro step:
//     static constexpr bool kStreamable = true;
//     static constexpr int kStreamSums;       // 0..2 sums over ALL coordinates (funnel: sum x_i^2 and x_0)
//     static constexpr bool kStreamHalo;      // the gradient reads the neighbouring coordinates (rw1)
//     template <class Cx> static void stream_sums(Cx&, const double (&theta)[2], const double (&mp)[2], double (&sums)[N]);
//     template <class Tab> static void stream_aux(const double (&sums)[N], int num_params, const Tab&, Aux&);
//     template <class Cx> static void stream_grad(Cx&, const double (&theta)[2], const double (&prev)[2],
//                                                 const double (&next)[2], const double (&mp)[2], double (&g)[2], const Aux&);
//     template <class Cx> static void stream_logp(Cx&, theta, prev, next, mp, const Aux&, double& acc);  // adds the terms
//     // (prev[j] / next[j]: the values at coordinate index(j) - 1 / + 1, 0.0 beyond the ends; the same expressions as
//     // in eval() give the same bits.  wn_models.h: FunnelModel, models/rw1.h)
//
//     // optional, host side (wn_engine_create): check / transform the parameter vector before it is uploaded;
//     // check num_params.  Throw std::invalid_argument to reject (-> error type `config`).
//     static void host_params(double* params, int num_params);
//     static void validate(int num_params);
//     // optional: geometry hint -- elements per lane (2, 4, 8 or 16); the engine then takes the fewest wavefronts per
//     // chain that hold num_params at that width instead of its default policy (one wavefront up to 1 024
//     // dimensions).  A model whose evaluation exchanges data across lanes or keeps many live vectors may prefer
//     // more, narrower wavefronts (models/rw1.h); an explicit waves_per_chain / elems_per_lane request still wins.
//     static constexpr int kPreferredElemsPerLane;
//     // ... or, where the best width depends on the dimension, the same hint as a function (0 = the default policy there):
//     static constexpr int preferred_elems_per_lane(int num_params);
//
//     // optional -- a model CONDITIONED ON DATA: the engine keeps a read-only observation block in HBM (x: num_obs rows
//     // of num_params doubles, y: num_obs doubles; wn_engine_create_observed / walnutpie_sample_device_observed*), and
//     // eval() reads it through the cx calls below.  A data model runs one wavefront per chain on the register kernels
//     // (1 <= num_params <= 1024, any num_obs >= 1): it declares no streaming form, and wn_engine_create refuses other
//     // geometries, a data model without data and data for a model without this member (`config` errors).
//     static constexpr bool kUsesData = true;
//     static void host_data(const double* x, const double* y, int num_obs, int num_params);  // optional checks (throw)
//     // (... or with a fifth argument `bool weighted`: whether the engine carries per-row weights, for a model whose
//     // admissible y depends on it -- logistic_regression then takes proportions in [0, 1])
//     // ... and, on top of kUsesData, a GROUP per observation (int32 in [0, J), copied beside y; wn_observations::group,
//     // num_groups): x then has P = num_params - J - 1 columns, stored at the narrower row stride
//     // Dx = 128 * ceil(P / 128) (host_data's last argument is P).
//     // wn_engine_create refuses a grouped model without groups and groups for a model without this member.
//     static constexpr bool kUsesGroups = true;
//     // ... and, on top of kUsesGroups, VARYING SLOPES: Q = cx.num_varying() >= 1 coefficients vary by group
//     // (wn_observations::num_varying, 0 meaning 1; at most 8) -- the intercept and the slopes of the FIRST Q - 1
//     // columns of x -- so theta ends with Q blocks of J effects and Q scales and x has P = num_params - Q (J + 1)
//     // columns (Q - 1 <= P).  Such a model takes num_varying as host_params' third argument,
//     // host_params(params, num_params, num_varying), which is called in place of the two-argument form.
//     // wn_engine_create refuses num_varying > 1 for a model without this member.  models/hier_slopes_glm.h.
//     static constexpr bool kVaryingSlopes = true;
//     // ... or, on top of kUsesData, a SCALE PARAMETER as the last
//     // coordinate: x has P = num_params - 1 columns, stored at the flat stride Dp with column num_params - 1 zero, so
//     // the row pass never sees the scale (host_data's last argument is P).  models/glm_scale.h.  Together with
//     // kUsesGroups theta ends [.. | s_tau | s]: x has P = num_params - J - 2 columns at the grouped stride, so neither
//     // scale is ever a column (wn_model_num_scale_params tells a front end).  models/hier_scale_glm.h.  Together with
//     // kVaryingSlopes theta ends [.. | s_0 .. s_{Q-1} | s]: x has P = num_params - Q (J + 1) - 1 columns, and
//     // host_params(params, num_params, num_varying) sees Q + 1 trailing scales.  models/hier_slopes_scale_glm.h.
//     static constexpr bool kScaleParam = true;
//     // ... and, on top of kUsesData, per-row OFFSETS and WEIGHTS (wn_observations::offset / weight /
//     // num_weight_sets; each optional at run time): the model reads them through cx.has_offset() / obs_offset() /
//     // has_weight() / obs_weight() below.  wn_engine_create refuses offsets or weights for a model without this member,
//     // and a model without it compiles nothing of them.
//     static constexpr bool kUsesRowTerms = true;
//     // ... and, on top of kUsesData, the POINTWISE log-likelihood (wn_pointwise.h: wn_engine_log_lik,
//     // wn_engine_log_predictive -- held-out log predictive density, WAIC, K-fold scores from draws that stay on the
//     // device).  pointwise() returns, in lane k, the likelihood term of row n0 + k of a tile of 64 consecutive rows
//     // (n0 a multiple of 64, wave-uniform) for the lanes whose `live` is set -- the other lanes' rows are absent or
//     // masked out: read nothing of theirs, return anything.  The prior is NOT part of it and weights are NEVER
//     // applied (cx.has_weight() is false here).  The built-in models form eta in the order models/glm.h states, pack
//     // the eta of the 64 rows into the 64 lanes (pointwise_eta) and evaluate their link ONCE, with a zero running sum
//     // -- the expression of eval()'s weighted path, so the bits are eval()'s.  pointwise_const(y) is, on the HOST in
//     // long double, whatever constant of the row's full log density the term leaves out (0 if none); it is rounded
//     // once, kept in a device array beside y, and added by the kernel as its last operation.  An engine whose model
//     // lacks this member refuses the two entry points with a `config` error that names the model.
//     static constexpr bool kPointwise = true;
//     template <int EPL, class Cx>
//     static double pointwise(Cx& cx, const double (&theta)[EPL], int n0, bool live);
//     static long double pointwise_const(double y);
//     // ... and, on top of kUsesData, PREDICTIONS (wn_predict.h: wn_engine_predict, wn_engine_predict_fold,
//     // wn_engine_predict_chains -- the linear predictor, the expected response and its variance of new rows from draws
//     // that stay on the device).  predict() leaves, in lane k, the triple of row n0 + k of a tile of 64 consecutive rows
//     // (n0 a multiple of 64, wave-uniform; `live` as for pointwise()): eta, the linear predictor; mu = E[y | theta,
//     // x_n]; v = Var[y | theta, x_n].  It reads x, the group and the offset, NEVER y or the weights.  The built-in
//     // models form eta exactly as their pointwise() does and evaluate Link::response / Family::response -- the sibling
//     // of term() -- ONCE on the full wavefront (wn_predict.h holds the table of mu and v per family).  An engine whose
//     // model lacks this member refuses the three entry points with a `config` error that names the model.
//     static constexpr bool kPredict = true;
//     template <int EPL, class Cx>
//     static void predict(Cx& cx, const double (&theta)[EPL], int n0, bool live, double& eta, double& mu, double& v);
//     // ... and, on top of kPredict, SIMULATED REPLICATES (wn_replicate.h: wn_engine_replicate,
//     // wn_engine_replicate_chains, wn_engine_replicate_check -- y_rep ~ p(y | theta, x_n) and posterior predictive
//     // checks from draws that stay on the device).  replicate() leaves, in lane k, predict()'s triple of row n0 + k --
//     // formed by the very expression predict() uses -- and yrep, ONE draw from the row's distribution taken from `rng`,
//     // the lane's counter stream (wn::RepStream, wn_devrand.h: keyed by seed, row, draw and chain; the kernel sets it
//     // up, the model only draws).  The built-in models call Link::replicate / Family::replicate, the sibling of
//     // response(), once on the full wavefront: wn::sample_normal / sample_bernoulli / sample_poisson / sample_negbin.
//     // A sampler with a loop must keep the wavefront together (wn::WaveAny; wn_devrand.h says why); y and the weights
//     // are never read.  An engine whose model lacks this member refuses the three entry points with a `config`
//     // error that names the model.
//     static constexpr bool kReplicate = true;
//     template <int EPL, class Cx>
//     static void replicate(Cx& cx, const double (&theta)[EPL], int n0, bool live, wn::RepStream& rng, double& eta,
//                           double& mu, double& v, double& yrep);
//   };
//
// What `cx` offers (all of it collective: every lane of the chain's workgroup must make the same calls):
//   cx.index(j), cx.valid(j), cx.dim()        coordinate of slot j; whether it is < num_params; num_params
//   cx.sum1(x)                                sum of x over all lanes of the chain (fixed order), wave-uniform
//   cx.element0(x)                            the value slot 0 of lane 0 holds (coordinate 0), wave-uniform
//   cx.shift(v, prev, next)                   prev[j] = v at coordinate index(j) - 1, next[j] = v at index(j) + 1
//                                             (0.0 beyond either end of the padded vector)
//   cx.uniform_tab()                          tables for wnd::dexp / wnd::dlog of a wave-uniform argument
//   cx.gather_tab()                           the same tables for a per-lane argument (every lane takes part)
//   Cx::mad(a, b, c)                          a * b + c: one fused multiply-add when the engine was created with
//                                             wn_config::fused_multiply_add, a rounded product plus an add otherwise
// ... and, compiled in for data models only (kUsesData; one wavefront per chain, so Cx::L == 64).  They are relative to
// the CHAIN's dataset: the engine's one block, or -- an engine built with several datasets
// (wn_observations::obs_offsets) -- the block of the dataset the chain is conditioned on; the model cannot tell:
//   cx.num_obs()                              number of observations, wave-uniform
//   cx.load_row(n, x)                         double x[EPL] = the lane's slots of row n of x: slot j holds column
//                                             cx.index(j), zero beyond num_params (a row is laid out like theta and
//                                             loads with the same 16-byte pair loads); n wave-uniform, 0 <= n < num_obs
//   cx.obs_y(n)                               y[n] (0 <= n < num_obs)
// ... and for grouped data models only (kUsesGroups):
//   cx.num_groups()                           J, wave-uniform
//   cx.obs_group(n)                           the group of observation n, in [0, J) (0 <= n < num_obs)
//   cx.num_varying()                          Q of a model with kVaryingSlopes, wave-uniform (1 for other grouped models)
//   cx.obs_x(n, col)                          x[n][col], a per-lane load (0 <= n < num_obs, col below the row's stride)
//   (cx.load_row then fills slot pairs k < Dx / 128 -- columns [128 k, 128 k + 128) -- and zeros the rest without
//   loading them; a flat model's rows keep the stride Dp and its loads)
// ... and for data models that declare kUsesRowTerms (eta_n += offset_n; the row's likelihood term and residual times
// weight_n >= 0; models/glm.h states the order of operations every built-in model follows):
//   cx.has_offset(), cx.has_weight()          whether the engine holds offsets / weights, wave-uniform: test once per
//                                             evaluation or per block, never per element
//   cx.obs_offset(n), cx.obs_weight(n)        offset_n / weight_n (0 <= n < num_obs; only where has_*() is true) -- with
//                                             weight sets, of the set the chain is conditioned on; the model cannot tell
// (pointwise() receives the same calls over the block of rows being scored -- wn_pointwise.h, PointwiseCx -- with
// cx.has_weight() false; cx.sum1 / element0 / shift are not offered there; predict() and replicate() receive the same cx)
// The wavefront primitives of the platform layer (wave_sum_packed, lane_value, set_lane, uni, ...: wn_gfx950.h, with
// the same association order under the CPU emulation) are available to eval(); models/glm.h uses them to reduce two
// rows' dot products per butterfly.
// Arithmetic: the library is compiled with -ffp-contract=off; what you write is what is evaluated (Cx::mad is the one
// place where the engine's arithmetic mode shows), so a CPU restatement of the same expressions reproduces the device
// bit for bit (that is how the parity tests work).
//
// Registration is a five-line translation unit, wn_kernels_<name>.hip, that the Makefile picks up by its name:
//   #include "models/my_model.h"
//   #define WN_MODEL_ID 6                 // 0-5, 15-18, 24-28, 32-36 and 40 are taken (std_normal, diag_normal, funnel, rw1,
//                                         //   linear_regression, logistic_regression; hier_linear_regression,
//                                         //   hier_logistic_regression and their _centered forms; poisson_regression,
//                                         //   neg_binomial_regression, linear_regression_sigma,
//                                         //   hier_poisson_regression and its _centered form;
//                                         //   hier_linear_regression_slopes, hier_logistic_regression_slopes,
//                                         //   hier_poisson_regression_slopes at 32-34;
//                                         //   hier_linear_regression_sigma and its _centered form at 35, 36;
//                                         //   hier_linear_regression_slopes_sigma at 40); < 64
//   #define WN_MODEL_TAG my_model         // wn_model_id("my_model") finds it at run time
//   #define WN_MODEL_TYPE wn::MyModel
//   #include "wn_kernels.inc"
// models/rw1.h is a complete example (the reference's AR(1) density with a neighbour-coupled gradient); models/glm.h
// one of a model conditioned on data (Bayesian linear, logistic and Poisson regression); models/hier_glm.h one with a
// group channel (hierarchical regression with varying intercepts); models/hier_slopes_glm.h one with varying slopes on
// top of it (32-34); models/glm_scale.h one with a scale parameter
// (negative binomial regression, linear regression with an estimated noise level); models/hier_scale_glm.h one with
// groups and a scale parameter (hierarchical linear regression with an estimated noise level, 35 and 36);
// models/hier_slopes_scale_glm.h one with varying slopes and a scale parameter (40).
#pragma once

#include "wn_devmath.h"
#include "wn_hip.h"
