// models/glm.h -- Bayesian generalised linear models on an observation block the engine keeps in HBM (wn_model_api.h,
// kUsesData): linear regression (unit-variance normal noise), logistic regression and Poisson regression, one template
// over the link.
//
//   eta = X theta,  prior theta_i ~ normal(0, s_i^2)  (model_params: the prior variances s^2)
//   linear_regression:    logp = -1/2 sum_n (y_n - eta_n)^2             - 1/2 sum_i theta_i^2 / s_i^2
//                         grad = X^T (y - eta)                            - theta / s^2
//   logistic_regression:  logp = sum_n (y_n eta_n - softplus(eta_n))     - 1/2 sum_i theta_i^2 / s_i^2
//                         grad = X^T (y - sigmoid(eta))                   - theta / s^2
//   poisson_regression:   logp = sum_n (y_n eta_n - exp(eta_n))           - 1/2 sum_i theta_i^2 / s_i^2
//                         grad = X^T (y - exp(eta))                       - theta / s^2
// (constants dropped.  A linear model with an unknown noise level sigma, and the negative binomial: models/glm_scale.h.)
//
// One pass over X per gradient evaluation.  The chain's lane `tid` holds EPL coordinates of theta, and row n of X is
// laid out the same way, so a row is EPL / 2 16-byte loads per lane and its product with theta is EPL lane-local
// multiply-adds.  What costs is the reduction of that partial dot product over the wavefront and the link function,
// so the rows are taken in BLOCKS of B = max(2, 32 / EPL) (the block's rows stay in registers: 32 doubles per lane):
//   1. for each pair of rows (n0 + 2k, n0 + 2k + 1) of the block, in order: the lanes' partial dot products (slot
//      order 0..EPL-1, Cx::mad) go through ONE packed butterfly (wave_sum_packed: offsets 32, 1, 2, 4, 8, 16) and
//      eta of row n0 + k lands in lane k (set_lane);
//   2. lanes 0..B-1 evaluate the link of their row at once (one vector evaluation for B rows): the residual
//      r = y - mean(eta) and the row's log-likelihood term, which lane k adds to its own running sum;
//   3. the residuals are broadcast back one row at a time (lane_value) and g[j] += x_row[j] * r, rows in order.
// The log-likelihood terms of lane k (rows n = n0 + k of every block, blocks in order) are added to the lane's prior
// partial after the last block; the kernels' own reduction of `acc` then sums the lanes in its fixed order.  A last,
// partial block reads no row at or beyond num_obs: its missing rows are zeros and their residuals and terms are
// masked to 0.  The CPU emulation runs the same source with the same butterfly order, so the bits agree.
//
// Per-row offsets o_n and weights w_n >= 0 (kUsesRowTerms; either may be absent, a wave-uniform test per evaluation):
//   eta_n = x_n . theta + o_n,   logp = prior + sum_n w_n ll_n(eta_n, y_n),   r_n = w_n d ll_n / d eta_n
// in this order, shared by every data model (glm_scale.h, hier_glm.h):
//   offset: between steps 1 and 2, lanes 0..B-1 add their row's o_n to eta (one add per block; lanes without a row add
//           0.0) -- in hier_glm.h after the group effect was added;
//   weight: the link is evaluated with a ZERO running sum, t = Link::term(eta, y, r, 0.0), then
//           ll = Cx::mad(w, t, ll) and r = w * r (glm_scale.h: also ds = ds + w * ds_n, ds_n the row's own partial);
//   w_n == 0: the row is discarded by SELECT, exactly as a row at or beyond num_obs (ll unchanged, r = 0), so it adds
//           nothing even when its eta overflows the link (t, r inf or NaN).
// Without weights the link receives the running sum as before and without offsets no add is issued: such an engine
// computes what it computed before these fields existed, bit for bit.
//
// The POINTWISE hook (wn_model_api.h, kPointwise; wn_pointwise.h): pointwise() returns, in lane k, the likelihood term of
// row n0 + k of a tile of 64 rows -- eta formed in the order above (pointwise_eta: the rows are streamed pair by pair,
// nothing is kept for a gradient pass, eta of 64 rows is packed into the 64 lanes), then ONE evaluation of
// Link::term(eta, y, r, 0.0, tab) on the full wavefront, the weighted path's expression.  Weights are never applied.
// pointwise_const(y) is the constant the term drops, added by the kernel as its last operation:
//   identity: -1/2 log 2 pi;   logit: 0 (Bernoulli per trial, the same expression for a proportion);   log: -lgamma(y + 1)
//
// The PREDICT hook (wn_model_api.h, kPredict; wn_predict.h): predict() leaves in lane k the triple (eta, mu, v) of row
// n0 + k -- eta formed as pointwise() forms it (pointwise_eta, the offset), then ONE evaluation of Link::response on the
// full wavefront: mu = E y and v = Var y given eta (wn_predict.h holds the table).  y and the weights are never read.
//
// The REPLICATE hook (wn_model_api.h, kReplicate; wn_replicate.h): replicate() forms (eta, mu, v) by the very expression
// predict() uses and adds y_rep ~ p(y | theta, x_n), drawn by Link::replicate -- the sibling of response() -- ONCE on the
// full wavefront from the lane's counter stream (wn_devrand.h: a normal with unit noise, a Bernoulli per trial, a
// Poisson).  y and the weights are never read.
//
// Arithmetic: the prior variances arrive as reciprocals (host_params, as the diagonal normal's); the logistic mean is
// one true division per block-row evaluation, 1 / (1 + exp(-|eta|)), and softplus(eta) = max(eta, 0) +
// log(1 + exp(-|eta|)) never overflows.  exp / log are wnd::dexp / wnd::dlog with per-lane arguments (gather tables).
#pragma once

#include <cmath>
#include <stdexcept>
#include <string>

#include "../wn_devrand.h"
#include "../wn_model_api.h"

namespace wn {

// -1/2 log(2 pi), the normal density's constant (host side: rounded once where it is uploaded)
constexpr long double kHalfLog2Pi = -0.918938533204672741780329736405617639L;

struct IdentityLink {
  // r = y - eta; ll += -1/2 r^2
  template <class Cx, class Tab>
  __device__ __forceinline__ static double term(double eta, double y, double& r, double ll, const Tab&) {
    r = y - eta;
    return Cx::mad(-0.5 * r, r, ll);
  }
  // mean and variance of y given eta: unit noise
  template <class Cx, class Tab>
  __device__ __forceinline__ static void response(double eta, double& mu, double& v, const Tab&) {
    mu = eta;
    v = 1.0;
  }
  // y_rep ~ normal(mu, 1)
  template <class Tab>
  __device__ __forceinline__ static double replicate(double mu, RepStream& rng, const Tab& tab) {
    return sample_normal(mu, 1.0, rng, tab);
  }
  static void check_y(double, bool) {}
  static long double pointwise_const(double) { return kHalfLog2Pi; }
};

struct LogitLink {
  // r = y - sigmoid(eta); ll += y eta - softplus(eta)
  template <class Cx, class Tab>
  __device__ __forceinline__ static double term(double eta, double y, double& r, double ll, const Tab& tab) {
    const double a = __builtin_fabs(eta);
    const double e = wnd::dexp(-a, tab);  // in (0, 1]
    const double d = 1.0 / (1.0 + e);
    const double mu = eta >= 0.0 ? d : e * d;
    const double sp = (eta > 0.0 ? eta : 0.0) + wnd::dlog(1.0 + e, tab);
    r = y - mu;
    return Cx::mad(y, eta, ll) - sp;
  }
  // per trial: mu as term() computes it for its residual; v = mu (1 - mu) as (e * d) * d, without the cancellation
  template <class Cx, class Tab>
  __device__ __forceinline__ static void response(double eta, double& mu, double& v, const Tab& tab) {
    const double e = wnd::dexp(-__builtin_fabs(eta), tab);
    const double d = 1.0 / (1.0 + e);
    mu = eta >= 0.0 ? d : e * d;
    v = (e * d) * d;
  }
  // y_rep ~ Bernoulli(mu), per trial
  template <class Tab>
  __device__ __forceinline__ static double replicate(double mu, RepStream& rng, const Tab&) {
    return sample_bernoulli(mu, rng);
  }
  // (with weights y may be a proportion: k successes in m trials are weight m and y = k / m)
  static void check_y(double y, bool weighted) {
    if (weighted) {
      if (!(y >= 0.0 && y <= 1.0))
        throw std::invalid_argument("logistic_regression with weights needs every y in [0, 1], got " + std::to_string(y));
    } else if (!(y == 0.0 || y == 1.0)) {
      throw std::invalid_argument("logistic_regression needs every y in {0, 1}");
    }
  }
  static long double pointwise_const(double) { return 0.0L; }
};

struct LogLink {
  // Poisson: r = y - exp(eta); ll += y eta - exp(eta) (-lgamma(y + 1) dropped).  exp(eta) overflows to inf beyond
  // eta ~ 709.78: the term is then non-finite and the trajectory treats it as every non-finite energy.
  template <class Cx, class Tab>
  __device__ __forceinline__ static double term(double eta, double y, double& r, double ll, const Tab& tab) {
    const double mu = wnd::dexp(eta, tab);
    r = y - mu;
    return Cx::mad(y, eta, ll) - mu;
  }
  // Poisson: mean and variance are exp(eta) (inf where it overflows)
  template <class Cx, class Tab>
  __device__ __forceinline__ static void response(double eta, double& mu, double& v, const Tab& tab) {
    mu = wnd::dexp(eta, tab);
    v = mu;
  }
  // y_rep ~ Poisson(mu) (NaN where exp(eta) is not served: wn_devrand.h)
  template <class Tab>
  __device__ __forceinline__ static double replicate(double mu, RepStream& rng, const Tab& tab) {
    return sample_poisson(mu, rng, tab, WaveAny{});
  }
  static void check_y(double y, bool) { check_count(y, "Poisson regression"); }
  static long double pointwise_const(double y) { return -lgammal(static_cast<long double>(y) + 1.0L); }
  // a count: finite, >= 0 and integer-valued
  static void check_count(double y, const char* model) {
    if (!(std::isfinite(y) && y >= 0.0 && y == std::floor(y)))
      throw std::invalid_argument(std::string(model) + " needs every y to be a count (finite, >= 0, integer-valued), got " +
                                  std::to_string(y));
  }
};

// The weighted form of a block's link results (header comment): t, r are the link's with a zero running sum; lanes
// without a row hold w = 0.  -> the lane's running sum; r becomes the weighted residual.
template <class Cx>
__device__ __forceinline__ double weigh_row(double w, double t, double& r, double ll) {
  const bool live = w != 0.0;
  r = live ? w * r : 0.0;
  return live ? Cx::mad(w, t, ll) : ll;
}

// the value of coordinate c (wave-uniform) of a vector laid out like theta, in every lane (one wavefront)
template <int EPL>
__device__ __forceinline__ double coord_value(const double (&v)[EPL], int c) {
  const int slot = 2 * (c >> 7) + (c & 1);
  double mine = 0.0;
#pragma unroll
  for (int j = 0; j < EPL; ++j) mine = j == slot ? v[j] : mine;
  return lane_value(mine, (c >> 1) & 63);
}

// The pointwise hook's row pass (header comment): eta of rows n0 .. n0 + 63 of the block, row n0 + k in lane k, for the
// rows whose lane holds `live` (the others: 0, and a pair of rows that is off issues no load).  nx: the slot pairs that
// hold columns of x.  Rows pair up as in eval() -- (even, odd), the even row's sum in lanes 0-31 -- so the bits are its.
template <int EPL, class Cx>
__device__ __forceinline__ double pointwise_eta(Cx& cx, const double (&th)[EPL], int n0, bool live, int nx) {
  static_assert(Cx::L == 64, "data models run one wavefront per chain");
  const int liv = live ? 1 : 0;
  double eta = 0.0;
#pragma unroll 2
  for (int k = 0; k < 64; k += 2) {
    const bool la = lane_value(liv, k) != 0, lb = lane_value(liv, k + 1) != 0;
    if (!(la || lb)) continue;
    double xa[EPL], xb[EPL];
    if (la) {
      cx.load_row(n0 + k, xa);
    } else {
#pragma unroll
      for (int j = 0; j < EPL; ++j) xa[j] = 0.0;
    }
    if (lb) {
      cx.load_row(n0 + k + 1, xb);
    } else {
#pragma unroll
      for (int j = 0; j < EPL; ++j) xb[j] = 0.0;
    }
    double da = 0.0, db = 0.0;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      if ((j >> 1) < nx) {
        da = Cx::mad(xa[j], th[j], da);
        db = Cx::mad(xb[j], th[j], db);
      }
    }
    const double packed = wave_sum_packed(da, db);
    set_lane(eta, uni(packed), k);
    set_lane(eta, lane_value(packed, 32), k + 1);
  }
  return eta;
}

template <class Link>
struct GlmModel {
  static constexpr bool kUsesParams = true;  // prior variances s^2 [num_params]
  static constexpr bool kUsesData = true;
  static constexpr bool kUsesRowTerms = true;
  static constexpr bool kElementwise = false;
  static constexpr bool kGradIsNegTheta = false;
  static constexpr bool kCheapGrad = false;
  __device__ __forceinline__ static double grad_elem(double, double) { return 0.0; }
  struct Aux {};

  template <int EPL>
  static constexpr int kBlock = EPL >= 16 ? 2 : 32 / EPL;  // rows per block (registers: 32 doubles per lane)

  template <int EPL, class Cx>
  __device__ __forceinline__ static void eval(Cx& cx, const double (&th)[EPL], double (&g)[EPL],
                                              const double (&rs2)[EPL], Aux&, double& acc) {
    static_assert(Cx::L == 64, "data models run one wavefront per chain");
    constexpr int B = kBlock<EPL>;
    static_assert(B % 2 == 0 && B <= 64, "rows are reduced in pairs");
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      g[j] = -th[j] * rs2[j];
      acc = Cx::mad(-0.5 * th[j] * th[j], rs2[j], acc);
    }
    const int N = cx.num_obs();
    const int me = opaque_lane_id();
    const bool offs = cx.has_offset(), wts = cx.has_weight();
    double ll = 0.0;  // this lane's log-likelihood terms
    for (int n0 = 0; n0 < N; n0 += B) {
      double x[B][EPL];
      double eta = 0.0;
#pragma unroll
      for (int k = 0; k < B; ++k) {
        if (n0 + k < N) {
          cx.load_row(n0 + k, x[k]);
        } else {
#pragma unroll
          for (int j = 0; j < EPL; ++j) x[k][j] = 0.0;
        }
      }
#pragma unroll
      for (int k = 0; k < B; k += 2) {
        double da = 0.0, db = 0.0;
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
          da = Cx::mad(x[k][j], th[j], da);
          db = Cx::mad(x[k + 1][j], th[j], db);
        }
        const double packed = wave_sum_packed(da, db);  // row k's sum in lanes 0-31, row k + 1's in lanes 32-63
        set_lane(eta, uni(packed), k);
        set_lane(eta, lane_value(packed, 32), k + 1);
      }
      const bool mine = me < B && n0 + me < N;
      const double y = mine ? cx.obs_y(n0 + me) : 0.0;
      if (offs) eta = eta + (mine ? cx.obs_offset(n0 + me) : 0.0);
      double r;
      const double ll_new = Link::template term<Cx>(eta, y, r, wts ? 0.0 : ll, cx.gather_tab());
      if (wts) {
        ll = weigh_row<Cx>(mine ? cx.obs_weight(n0 + me) : 0.0, ll_new, r, ll);
      } else {
        ll = mine ? ll_new : ll;
        r = mine ? r : 0.0;
      }
#pragma unroll
      for (int k = 0; k < B; ++k) {
        const double rk = lane_value(r, k);
#pragma unroll
        for (int j = 0; j < EPL; ++j) g[j] = Cx::mad(x[k][j], rk, g[j]);
      }
    }
    acc = acc + ll;
  }
  __device__ __forceinline__ static double finish(double sum, const Aux&, int) { return sum; }

  // the pointwise hook (header comment): lane k's likelihood term of row n0 + k, constant dropped
  static constexpr bool kPointwise = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static double pointwise(Cx& cx, const double (&th)[EPL], int n0, bool live) {
    double eta = pointwise_eta<EPL>(cx, th, n0, live, EPL / 2);
    const int n = n0 + opaque_lane_id();
    const double y = live ? cx.obs_y(n) : 0.0;
    if (cx.has_offset()) eta = eta + (live ? cx.obs_offset(n) : 0.0);
    double r;
    return Link::template term<Cx>(eta, y, r, 0.0, cx.gather_tab());
  }
  static long double pointwise_const(double y) { return Link::pointwise_const(y); }

  // the predict hook (header comment): lane k's (eta, mu, v) of row n0 + k
  static constexpr bool kPredict = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static void predict(Cx& cx, const double (&th)[EPL], int n0, bool live, double& eta,
                                                 double& mu, double& v) {
    eta = pointwise_eta<EPL>(cx, th, n0, live, EPL / 2);
    if (cx.has_offset()) eta = eta + (live ? cx.obs_offset(n0 + opaque_lane_id()) : 0.0);
    Link::template response<Cx>(eta, mu, v, cx.gather_tab());
  }

  // the replicate hook (header comment): predict()'s triple and, from the lane's counter stream, y_rep of row n0 + k
  static constexpr bool kReplicate = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static void replicate(Cx& cx, const double (&th)[EPL], int n0, bool live, RepStream& rng,
                                                   double& eta, double& mu, double& v, double& yrep) {
    predict<EPL>(cx, th, n0, live, eta, mu, v);
    yrep = Link::replicate(mu, rng, cx.gather_tab());
  }

  // host side: the prior variances -> their reciprocals (rounded once), and the observations' checks
  static void host_params(double* s2, int num_params) {
    for (int i = 0; i < num_params; ++i) {
      if (!(s2[i] > 0) || !std::isfinite(s2[i])) throw std::invalid_argument("prior variances must be positive and finite");
      s2[i] = 1.0 / s2[i];
    }
  }
  static void host_data(const double*, const double* y, int num_obs, int, bool weighted) {
    for (int n = 0; n < num_obs; ++n) Link::check_y(y[n], weighted);
  }
  static void validate(int num_params) {
    if (num_params > 1024)
      throw std::invalid_argument("a data model supports 1 <= num_params <= 1024 (one wavefront per chain), got " +
                                  std::to_string(num_params));
  }
};

using LinearRegressionModel = GlmModel<IdentityLink>;
using LogisticRegressionModel = GlmModel<LogitLink>;
using PoissonRegressionModel = GlmModel<LogLink>;

}  // namespace wn
