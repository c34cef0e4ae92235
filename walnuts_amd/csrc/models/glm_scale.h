// models/glm_scale.h -- flat data models whose LAST coordinate is a scale parameter, not a column of x (wn_model_api.h,
// kUsesData + kScaleParam): negative binomial regression and linear regression with an unknown noise level, one
// template over the family.
//
//   theta = [beta_0 .. beta_{P-1} | s],  P = num_params - 1,  eta_n = x_n . beta,  scale = exp(s)
//   model_params [P + 1]: the prior variances s2_i of beta, then the half-normal scale sigma_0 of exp(s)
//   both:  logp += -1/2 sum_i beta_i^2 / s2_i + s - exp(2 s) / (2 sigma_0^2)   (half-normal on exp(s) in log space, with
//          its Jacobian, as tau in hier_glm.h);  g_beta = X^T r - beta / s2,  g_s = sum_n dll_n/ds + 1 - exp(2 s) / sigma_0^2
//   neg_binomial_regression (NB2):  kappa = exp(s), phi = 1 / kappa, t = eta + s,  E y = exp(eta), Var y = mu + kappa mu^2
//          ll_n = lgamma(y + phi) - lgamma(phi) + y t - (y + phi) softplus(t)                 (-lgamma(y + 1) dropped)
//          r_n = y - (y + phi) sigmoid(t),   dll_n/ds = r_n + phi (softplus(t) - [psi(y + phi) - psi(phi)])
//   linear_regression_sigma:  sigma = exp(s)
//          ll_n = -(y - eta)^2 / (2 sigma^2) - s,   r_n = (y - eta) / sigma^2,   dll_n/ds = (y - eta)^2 / sigma^2 - 1
// (constants dropped).  The host stores x's P columns at the flat stride Dp with column num_params - 1 zero, so the row
// pass of glm.h never sees s; g[D-1] receives no row terms and is written in the epilogue.
//
// The row pass is glm.h's (blocks of B = 32 / EPL rows, two rows' dot products per packed butterfly, the family's row
// term on lanes 0..B-1 at once, the residuals broadcast back from registers).  The family's row term also returns a
// per-lane partial of d/ds, summed over the lanes by ONE cx.sum1 in the epilogue.  What depends on s alone -- scale,
// phi and the lgamma / digamma constants of phi (wnd::GammaConsts), 1 / sigma^2 -- is computed once per evaluation from
// the wave-uniform s.  A non-finite scale (s beyond about +-709) takes no path of its own: the energy turns non-finite
// and the trajectory treats it as every non-finite energy.
//
// Per-row offsets and weights as in glm.h (its header states the order).  With weights the family's term is evaluated
// with zero running sums (t, r, ds_n the row's own), then ds = ds + w * ds_n (a rounded product, then the add),
// ll = Cx::mad(w, t, ll) and r = w * r; a row with w == 0 is discarded by select.
//
// The pointwise hook (glm.h's header; wn_pointwise.h): glm.h's pointwise_eta, then the family's term with zero running
// sums on the full wavefront; what depends on s alone is computed once per draw and tile as above.  The constants the
// terms drop: -lgamma(y + 1) (negative binomial), -1/2 log 2 pi (linear_regression_sigma).
//
// The predict hook (glm.h's header; wn_predict.h): glm.h's pointwise_eta and the offset, then the family's response on
// the full wavefront with scale = exp(s) computed once per draw and tile: the negative binomial's mu = exp(eta),
// v = mu + kappa mu^2 as Cx::mad(kappa * mu, mu, mu) with kappa = scale; the normal's mu = eta, v = scale * scale.
//
// The replicate hook (glm.h's header; wn_replicate.h): predict()'s triple, then the family's draw on the full wavefront
// with the same scale: the negative binomial's gamma-Poisson mixture with kappa = scale, the normal's
// fmad(scale, z, mu) -- scale itself, not sqrt(scale * scale).
#pragma once

#include "glm.h"

namespace wn {

struct NegBinomialFamily {
  struct Consts {
    double s, phi;
    wnd::GammaConsts gam;
  };
  template <class Tab>
  __device__ __forceinline__ static Consts consts(double s, double scale, const Tab& tab) {
    const double phi = 1.0 / scale;
    return Consts{s, phi, wnd::gamma_consts(phi, tab)};
  }
  // ll += the row's term; r = d ll / d eta; ds += d ll / ds.  Per lane: two true divisions (the sigmoid's and the
  // one of wnd::dlgamma_digamma_diff), one dexp, two dlog1p, and one dlog when phi < 16.
  template <class Cx, class Tab>
  __device__ __forceinline__ static void term(double eta, double y, const Consts& k, const Tab& tab, double& r,
                                              double& ll, double& ds) {
    const double t = eta + k.s;
    const double e = wnd::dexp(-__builtin_fabs(t), tab);  // (0, 1]
    const double d = 1.0 / (1.0 + e);
    const double sig = t >= 0.0 ? d : e * d;
    const double sp = (t > 0.0 ? t : 0.0) + wnd::dlog1p(e, tab);  // wnd::dsoftplus(t), sharing e with the sigmoid
    double lg, dg;
    wnd::dlgamma_digamma_diff(y, k.gam, tab, lg, dg);
    const double yp = y + k.phi;
    r = y - yp * sig;
    ll = (ll + (Cx::mad(y, t, lg))) - yp * sp;
    ds = ds + Cx::mad(k.phi, sp - dg, r);
  }
  // E y = exp(eta), Var y = mu + kappa mu^2 (NB2), kappa = scale
  template <class Cx, class Tab>
  __device__ __forceinline__ static void response(double eta, double scale, double& mu, double& v, const Tab& tab) {
    mu = wnd::dexp(eta, tab);
    v = Cx::mad(scale * mu, mu, mu);
  }
  // y_rep ~ NB2(mu, kappa = scale)
  template <class Tab>
  __device__ __forceinline__ static double replicate(double mu, double scale, RepStream& rng, const Tab& tab) {
    return sample_negbin(mu, scale, rng, tab, WaveAny{});
  }
  static void check_y(double y, bool) { LogLink::check_count(y, "negative binomial regression"); }
  static long double pointwise_const(double y) { return LogLink::pointwise_const(y); }
};

struct NormalSigmaFamily {
  struct Consts {
    double s, isig2;
  };
  template <class Tab>
  __device__ __forceinline__ static Consts consts(double s, double scale, const Tab&) {
    return Consts{s, 1.0 / (scale * scale)};
  }
  // no division, no dexp / dlog per row
  template <class Cx, class Tab>
  __device__ __forceinline__ static void term(double eta, double y, const Consts& k, const Tab&, double& r, double& ll,
                                              double& ds) {
    const double d = y - eta;
    r = d * k.isig2;
    ll = Cx::mad(-0.5 * d, r, ll) - k.s;
    ds = Cx::mad(d, r, ds) - 1.0;
  }
  // E y = eta, Var y = sigma^2, sigma = scale
  template <class Cx, class Tab>
  __device__ __forceinline__ static void response(double eta, double scale, double& mu, double& v, const Tab&) {
    mu = eta;
    v = scale * scale;
  }
  // y_rep ~ normal(mu, sigma = scale)
  template <class Tab>
  __device__ __forceinline__ static double replicate(double mu, double scale, RepStream& rng, const Tab& tab) {
    return sample_normal(mu, scale, rng, tab);
  }
  static void check_y(double, bool) {}
  static long double pointwise_const(double) { return kHalfLog2Pi; }
};

template <class Family>
struct GlmScaleModel {
  static constexpr bool kUsesParams = true;  // [s2_0 .. s2_{P-1} | sigma_0]
  static constexpr bool kUsesData = true;
  static constexpr bool kScaleParam = true;
  static constexpr bool kUsesRowTerms = true;
  static constexpr bool kElementwise = false;
  static constexpr bool kGradIsNegTheta = false;
  static constexpr bool kCheapGrad = false;
  __device__ __forceinline__ static double grad_elem(double, double) { return 0.0; }
  struct Aux {};

  template <int EPL>
  static constexpr int kBlock = GlmModel<IdentityLink>::template kBlock<EPL>;

  template <int EPL, class Cx>
  __device__ __forceinline__ static void eval(Cx& cx, const double (&th)[EPL], double (&g)[EPL],
                                              const double (&mp)[EPL], Aux&, double& acc) {
    static_assert(Cx::L == 64, "data models run one wavefront per chain");
    constexpr int B = kBlock<EPL>;
    static_assert(B % 2 == 0 && B <= 64, "rows are reduced in pairs");
    const int D = cx.dim();
    const double s = coord_value(th, D - 1);
    const double isig0 = coord_value(mp, D - 1);  // 1 / sigma_0^2 (host_params)
    const double scale = wnd::dexp(s, cx.uniform_tab());
    const typename Family::Consts k = Family::consts(s, scale, cx.uniform_tab());
    // beta: the prior as in glm.h (padding slots: theta 0, mp 1 -> nothing); s: written in the epilogue
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const bool beta = cx.index(j) != D - 1;
      g[j] = beta ? -th[j] * mp[j] : 0.0;
      if (beta) acc = Cx::mad(-0.5 * th[j] * th[j], mp[j], acc);
    }
    const int N = cx.num_obs();
    const int me = opaque_lane_id();
    const bool offs = cx.has_offset(), wts = cx.has_weight();
    double ll = 0.0;  // this lane's log-likelihood terms
    double ds = 0.0;  // ... and their derivatives with respect to s
    for (int n0 = 0; n0 < N; n0 += B) {
      double x[B][EPL];
      double eta = 0.0;
#pragma unroll
      for (int kk = 0; kk < B; ++kk) {
        if (n0 + kk < N) {
          cx.load_row(n0 + kk, x[kk]);
        } else {
#pragma unroll
          for (int j = 0; j < EPL; ++j) x[kk][j] = 0.0;
        }
      }
#pragma unroll
      for (int kk = 0; kk < B; kk += 2) {
        double da = 0.0, db = 0.0;
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
          da = Cx::mad(x[kk][j], th[j], da);
          db = Cx::mad(x[kk + 1][j], th[j], db);
        }
        const double packed = wave_sum_packed(da, db);
        set_lane(eta, uni(packed), kk);
        set_lane(eta, lane_value(packed, 32), kk + 1);
      }
      const bool mine = me < B && n0 + me < N;
      const double y = mine ? cx.obs_y(n0 + me) : 0.0;
      if (offs) eta = eta + (mine ? cx.obs_offset(n0 + me) : 0.0);
      double r, ll_new = wts ? 0.0 : ll, ds_new = wts ? 0.0 : ds;
      Family::template term<Cx>(eta, y, k, cx.gather_tab(), r, ll_new, ds_new);
      if (wts) {
        const double w = mine ? cx.obs_weight(n0 + me) : 0.0;
        ds = w != 0.0 ? ds + w * ds_new : ds;
        ll = weigh_row<Cx>(w, ll_new, r, ll);
      } else {
        ll = mine ? ll_new : ll;
        ds = mine ? ds_new : ds;
        r = mine ? r : 0.0;
      }
#pragma unroll
      for (int kk = 0; kk < B; ++kk) {
        const double rk = lane_value(r, kk);
#pragma unroll
        for (int j = 0; j < EPL; ++j) g[j] = Cx::mad(x[kk][j], rk, g[j]);
      }
    }
    acc = acc + ll;
    const double sum = cx.sum1(ds);
    const double tt = scale * scale * isig0;  // exp(2 s) / sigma_0^2
    const double gs = (sum + 1.0) - tt;
    const double lps = s - 0.5 * tt;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const bool last = cx.index(j) == D - 1;
      g[j] = last ? gs : g[j];
      if (last) acc = acc + lps;
    }
  }
  __device__ __forceinline__ static double finish(double sum, const Aux&, int) { return sum; }

  // the pointwise hook (header comment): lane k's likelihood term of row n0 + k, constant dropped
  static constexpr bool kPointwise = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static double pointwise(Cx& cx, const double (&th)[EPL], int n0, bool live) {
    const double s = coord_value(th, cx.dim() - 1);
    const double scale = wnd::dexp(s, cx.uniform_tab());
    const typename Family::Consts k = Family::consts(s, scale, cx.uniform_tab());
    double eta = pointwise_eta<EPL>(cx, th, n0, live, EPL / 2);
    const int n = n0 + opaque_lane_id();
    const double y = live ? cx.obs_y(n) : 0.0;
    if (cx.has_offset()) eta = eta + (live ? cx.obs_offset(n) : 0.0);
    double r, ll = 0.0, ds = 0.0;
    Family::template term<Cx>(eta, y, k, cx.gather_tab(), r, ll, ds);
    return ll;
  }
  static long double pointwise_const(double y) { return Family::pointwise_const(y); }

  // the predict hook (header comment): lane k's (eta, mu, v) of row n0 + k
  static constexpr bool kPredict = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static void predict(Cx& cx, const double (&th)[EPL], int n0, bool live, double& eta,
                                                 double& mu, double& v) {
    const double scale = wnd::dexp(coord_value(th, cx.dim() - 1), cx.uniform_tab());
    eta = pointwise_eta<EPL>(cx, th, n0, live, EPL / 2);
    if (cx.has_offset()) eta = eta + (live ? cx.obs_offset(n0 + opaque_lane_id()) : 0.0);
    Family::template response<Cx>(eta, scale, mu, v, cx.gather_tab());
  }

  // the replicate hook (header comment): predict()'s triple and y_rep of row n0 + k
  static constexpr bool kReplicate = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static void replicate(Cx& cx, const double (&th)[EPL], int n0, bool live, RepStream& rng,
                                                   double& eta, double& mu, double& v, double& yrep) {
    predict<EPL>(cx, th, n0, live, eta, mu, v);
    const double scale = wnd::dexp(coord_value(th, cx.dim() - 1), cx.uniform_tab());  // (predict()'s own, again)
    yrep = Family::replicate(mu, scale, rng, cx.gather_tab());
  }

  // host side: the beta prior variances -> reciprocals, sigma_0 -> 1 / sigma_0^2 (each rounded once); the
  // observations' checks are the family's (x has num_params - 1 columns)
  static void host_params(double* mp, int num_params) {
    for (int i = 0; i < num_params; ++i)
      if (!(mp[i] > 0) || !std::isfinite(mp[i]))
        throw std::invalid_argument("model_params (prior variances, sigma_0) must be positive and finite");
    for (int i = 0; i + 1 < num_params; ++i) mp[i] = 1.0 / mp[i];
    mp[num_params - 1] = 1.0 / (mp[num_params - 1] * mp[num_params - 1]);
  }
  static void host_data(const double*, const double* y, int num_obs, int, bool weighted) {
    for (int n = 0; n < num_obs; ++n) Family::check_y(y[n], weighted);
  }
  static void validate(int num_params) {
    if (num_params < 2 || num_params > 1024)
      throw std::invalid_argument("a data model with a scale parameter supports 2 <= num_params <= 1024 (beta and s, one "
                                  "wavefront per chain), got " + std::to_string(num_params));
  }
};

using NegBinomialRegressionModel = GlmScaleModel<NegBinomialFamily>;
using LinearRegressionSigmaModel = GlmScaleModel<NormalSigmaFamily>;

}  // namespace wn
