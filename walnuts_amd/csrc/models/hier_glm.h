// models/hier_glm.h -- hierarchical (multilevel) regression with varying intercepts by group, on an observation block
// with a group channel (wn_model_api.h, kUsesData + kUsesGroups): linear, logistic and Poisson, each non-centered and
// centered, one template over the link (models/glm.h) and the parameterization.
//
//   theta = [beta_0 .. beta_{P-1} | u_0 .. u_{J-1} | s],  tau = exp(s),  g(n) in [0, J) the group of observation n
//   model_params [P + J + 1]: the prior variances s2_i of beta, J reserved entries (1), the half-normal scale sigma_tau
//   non-centered (u = z):  eta_n = x_n . beta + tau z_{g(n)},  logp += -1/2 sum_j z_j^2
//   centered     (u = a):  eta_n = x_n . beta + a_{g(n)},      logp += -J s - sum_j a_j^2 / (2 tau^2)
//   both:                  logp += s - tau^2 / (2 sigma_tau^2)     (half-normal on tau, in log space, with its Jacobian)
//                          + the beta prior and the likelihood of glm.h, r_n = y_n - mean(eta_n)
//   S_j = sum_{n in group j} r_n;
//   non-centered:  d/dz_j = tau S_j - z_j,        d/ds = tau sum_j z_j S_j + 1 - tau^2 / sigma_tau^2
//   centered:      d/da_j = S_j - a_j / tau^2,    d/ds = -J + sum_j a_j^2 / tau^2 + 1 - tau^2 / sigma_tau^2
// (constants dropped).  x has P = num_params - J - 1 columns, stored at the narrower stride Dx = 128 ceil(P / 128):
// cx.load_row fills slot pairs at and beyond Dx / 128 with zeros without loading them, and the row pass below takes no
// multiply-add there either (a wave-uniform test).
//
// The row pass is glm.h's: blocks of B = 32 / EPL rows, two rows' dot products per packed butterfly, the link of a
// whole block in one vector evaluation, the gradient accumulated from the registers that hold the rows.  Each block adds:
//   1. lanes 0..B-1 read their row's group (one int32 load per lane); per row k, in order, the group is made
//      wave-uniform (readlane), the value v_g of its coordinate P + g is taken from the lane that owns it (a select
//      over the EPL slots by the wave-uniform slot, then a readlane), times tau when non-centered, and set into lane k,
//      which adds it to its eta before the link;
//   2. the residual of row k, broadcast for the gradient of beta, is added into S_g in the owner lane's slot of
//      coordinate P + g (S_j accumulates in g[] there), rows in order: no atomics, no scheduling-dependent order, so
//      the CPU emulation of the same source gives the same bits.
// Per-row offsets and weights as in glm.h (its header states the order): the offset is added to eta after the group
// effect; the residual carries the weight, so S_g is a weighted sum with no further code.
// tau = wnd::dexp(s) of the wave-uniform s, once per evaluation; the epilogue applies the formulas above with one
// cx.sum1 (sum_j z_j S_j, or sum_j a_j^2).  A non-finite tau (s beyond +-709) takes no path of its own: the energy
// turns non-finite and the trajectory treats it as every non-finite energy.
//
// The pointwise hook (glm.h's header; wn_pointwise.h): glm.h's pointwise_eta over the P columns, the group effect of the
// tile's rows set into their lanes row by row as in step 1 above, the offset, then the link once on the full wavefront.
// The predict hook (glm.h's header; wn_predict.h) forms eta in the same way and evaluates Link::response in place of
// Link::term; y is never read.
#pragma once

#include "glm.h"

namespace wn {

template <class Link, bool Centered>
struct HierGlmModel {
  static constexpr bool kUsesParams = true;  // [s2_0 .. s2_{P-1} | 1 .. 1 | sigma_tau]
  static constexpr bool kUsesData = true;
  static constexpr bool kUsesGroups = true;
  static constexpr bool kUsesRowTerms = true;
  static constexpr bool kElementwise = false;
  static constexpr bool kGradIsNegTheta = false;
  static constexpr bool kCheapGrad = false;
  __device__ __forceinline__ static double grad_elem(double, double) { return 0.0; }
  struct Aux {};

  template <int EPL>
  static constexpr int kBlock = GlmModel<Link>::template kBlock<EPL>;

  // the value of coordinate c (wave-uniform) of a vector laid out like theta, in every lane (glm.h)
  template <int EPL>
  __device__ __forceinline__ static double coord(const double (&v)[EPL], int c) {
    return coord_value(v, c);
  }

  template <int EPL, class Cx>
  __device__ __forceinline__ static void eval(Cx& cx, const double (&th)[EPL], double (&g)[EPL],
                                              const double (&mp)[EPL], Aux&, double& acc) {
    static_assert(Cx::L == 64, "data models run one wavefront per chain");
    constexpr int B = kBlock<EPL>;
    static_assert(B % 2 == 0 && B <= 64, "rows are reduced in pairs");
    const int D = cx.dim();
    const int J = cx.num_groups();
    const int P = D - J - 1;
    const int nx = (P + 127) >> 7;  // slot pairs that hold columns of x
    const double s = coord(th, D - 1);
    const double isig2 = coord(mp, D - 1);  // 1 / sigma_tau^2 (host_params)
    const double tau = wnd::dexp(s, cx.uniform_tab());
    const double itau2 = Centered ? 1.0 / (tau * tau) : 0.0;
    // beta: the prior as in glm.h; z (non-centered): -1/2 z^2; u slots start S_j at 0
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const int c = cx.index(j);
      const bool beta = c < P;
      const bool grp = c >= P && c < P + J;
      g[j] = beta ? -th[j] * mp[j] : 0.0;
      if (beta) acc = Cx::mad(-0.5 * th[j] * th[j], mp[j], acc);
      if (!Centered && grp) acc = Cx::mad(-0.5 * th[j], th[j], acc);
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
          if ((j >> 1) < nx) {
            da = Cx::mad(x[k][j], th[j], da);
            db = Cx::mad(x[k + 1][j], th[j], db);
          }
        }
        const double packed = wave_sum_packed(da, db);
        set_lane(eta, uni(packed), k);
        set_lane(eta, lane_value(packed, 32), k + 1);
      }
      const bool mine = me < B && n0 + me < N;
      const int grp = mine ? cx.obs_group(n0 + me) : 0;
      int gk[B];  // wave-uniform: the coordinate P + g of row k's group
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < B; ++k) {
        gk[k] = P + lane_value(grp, k);
        const double vk = coord(th, gk[k]);
        set_lane(v, Centered ? vk : tau * vk, k);
      }
      eta = eta + v;
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
        for (int j = 0; j < EPL; ++j)
          if ((j >> 1) < nx) g[j] = Cx::mad(x[k][j], rk, g[j]);
        const int slot = 2 * (gk[k] >> 7) + (gk[k] & 1);
        const bool owner = me == ((gk[k] >> 1) & 63);
#pragma unroll
        for (int j = 0; j < EPL; ++j) g[j] = (owner && j == slot) ? g[j] + rk : g[j];
      }
    }
    acc = acc + ll;
    // epilogue: g[j] holds S_j in the u slots
    double part = 0.0;  // sum_j z_j S_j (non-centered) or sum_j a_j^2 (centered)
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const int c = cx.index(j);
      if (c >= P && c < P + J) part = Centered ? Cx::mad(th[j], th[j], part) : Cx::mad(th[j], g[j], part);
    }
    const double sum = cx.sum1(part);
    const double tt = tau * tau * isig2;  // tau^2 / sigma_tau^2
    double gs, lps;
    if constexpr (Centered) {
      const double q = sum * itau2;  // sum_j a_j^2 / tau^2
      gs = ((q - static_cast<double>(J)) + 1.0) - tt;
      lps = ((s - static_cast<double>(J) * s) - 0.5 * q) - 0.5 * tt;
    } else {
      gs = Cx::mad(tau, sum, 1.0) - tt;
      lps = s - 0.5 * tt;
    }
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const int c = cx.index(j);
      const bool grp = c >= P && c < P + J;
      if constexpr (Centered) {
        g[j] = grp ? g[j] - th[j] * itau2 : g[j];
      } else {
        g[j] = grp ? Cx::mad(tau, g[j], -th[j]) : g[j];
      }
      g[j] = c == D - 1 ? gs : g[j];
      if (c == D - 1) acc = acc + lps;
    }
  }
  __device__ __forceinline__ static double finish(double sum, const Aux&, int) { return sum; }

  // the pointwise hook (header comment): lane k's likelihood term of row n0 + k, constant dropped
  static constexpr bool kPointwise = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static double pointwise(Cx& cx, const double (&th)[EPL], int n0, bool live) {
    const int D = cx.dim();
    const int P = D - cx.num_groups() - 1;
    const double tau = Centered ? 1.0 : wnd::dexp(coord(th, D - 1), cx.uniform_tab());
    double eta = pointwise_eta<EPL>(cx, th, n0, live, (P + 127) >> 7);
    const int n = n0 + opaque_lane_id();
    const int grp = live ? cx.obs_group(n) : 0;
    const int liv = live ? 1 : 0;
    double v = 0.0;
    for (int k = 0; k < 64; ++k) {
      if (lane_value(liv, k) == 0) continue;
      const double vk = coord(th, P + lane_value(grp, k));
      set_lane(v, Centered ? vk : tau * vk, k);
    }
    eta = eta + v;
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
    const int D = cx.dim();
    const int P = D - cx.num_groups() - 1;
    const double tau = Centered ? 1.0 : wnd::dexp(coord(th, D - 1), cx.uniform_tab());
    eta = pointwise_eta<EPL>(cx, th, n0, live, (P + 127) >> 7);
    const int n = n0 + opaque_lane_id();
    const int grp = live ? cx.obs_group(n) : 0;
    const int liv = live ? 1 : 0;
    double u = 0.0;
    for (int k = 0; k < 64; ++k) {
      if (lane_value(liv, k) == 0) continue;
      const double uk = coord(th, P + lane_value(grp, k));
      set_lane(u, Centered ? uk : tau * uk, k);
    }
    eta = eta + u;
    if (cx.has_offset()) eta = eta + (live ? cx.obs_offset(n) : 0.0);
    Link::template response<Cx>(eta, mu, v, cx.gather_tab());
  }

  // the replicate hook (glm.h's header; wn_replicate.h): predict()'s triple and y_rep of row n0 + k
  static constexpr bool kReplicate = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static void replicate(Cx& cx, const double (&th)[EPL], int n0, bool live, RepStream& rng,
                                                   double& eta, double& mu, double& v, double& yrep) {
    predict<EPL>(cx, th, n0, live, eta, mu, v);
    yrep = Link::replicate(mu, rng, cx.gather_tab());
  }

  // host side: the beta prior variances and the reserved entries -> reciprocals, sigma_tau -> 1 / sigma_tau^2 (each
  // rounded once); the observations' checks are the link's
  static void host_params(double* mp, int num_params) {
    for (int i = 0; i < num_params; ++i)
      if (!(mp[i] > 0) || !std::isfinite(mp[i]))
        throw std::invalid_argument("model_params (prior variances, reserved entries, sigma_tau) must be positive and finite");
    for (int i = 0; i + 1 < num_params; ++i) mp[i] = 1.0 / mp[i];
    mp[num_params - 1] = 1.0 / (mp[num_params - 1] * mp[num_params - 1]);
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

using HierLinearRegressionModel = HierGlmModel<IdentityLink, false>;
using HierLogisticRegressionModel = HierGlmModel<LogitLink, false>;
using HierLinearRegressionCenteredModel = HierGlmModel<IdentityLink, true>;
using HierLogisticRegressionCenteredModel = HierGlmModel<LogitLink, true>;
using HierPoissonRegressionModel = HierGlmModel<LogLink, false>;
using HierPoissonRegressionCenteredModel = HierGlmModel<LogLink, true>;

}  // namespace wn
