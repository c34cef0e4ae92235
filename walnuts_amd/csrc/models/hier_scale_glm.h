// models/hier_scale_glm.h -- hierarchical regression with varying intercepts by group AND an estimated scale: the
// grouped models of models/hier_glm.h with the families of models/glm_scale.h (wn_model_api.h, kUsesData +
// kUsesGroups + kScaleParam): linear regression with an unknown noise level, non-centered and centered, one template
// over the family and the parameterization (the aliases at the end say which instantiations the library registers).
//
//   theta = [beta_0 .. beta_{P-1} | u_0 .. u_{J-1} | s_tau | s],  tau = exp(s_tau),  scale = exp(s),  D = P + J + 2
//   model_params [D]: the prior variances s2_i of beta, J reserved entries (1), the half-normal scales sigma_tau of tau
//   and sigma_0 of exp(s)
//   non-centered (u = z):  eta_n = x_n . beta + tau z_{g(n)} + offset_n,  logp += -1/2 sum_j z_j^2
//   centered     (u = a):  eta_n = x_n . beta + a_{g(n)} + offset_n,      logp += -J s_tau - sum_j a_j^2 / (2 tau^2)
//   both:  logp += -1/2 sum_i beta_i^2 / s2_i + [s_tau - tau^2 / (2 sigma_tau^2)] + [s - exp(2 s) / (2 sigma_0^2)]
//                  + sum_n w_n ll_n(eta_n, y_n, s)                            (the family's term, glm_scale.h's header)
//   r_n = w_n dll_n/deta,  g_beta = X^T r - beta / s2,  S_j = sum_{n in group j} r_n
//   non-centered:  d/dz_j = tau S_j - z_j,        d/ds_tau = tau sum_j z_j S_j + 1 - tau^2 / sigma_tau^2
//   centered:      d/da_j = S_j - a_j / tau^2,    d/ds_tau = -J + sum_j a_j^2 / tau^2 + 1 - tau^2 / sigma_tau^2
//   both:          d/ds = sum_n w_n dll_n/ds + 1 - exp(2 s) / sigma_0^2
// (constants dropped).  x has P = D - J - 2 columns at the grouped stride Dx = 128 ceil(P / 128) (hier_glm.h's header):
// neither scale is ever a column, and the row pass takes no multiply-add in slot pairs at and beyond Dx / 128.
//
// Where the two scales live: coordinate c sits in lane (c >> 1) & 63, slot 2 (c >> 7) + (c & 1) (glm.h's coord_value).
// s_tau is coordinate D - 2 and s coordinate D - 1; they share a lane when D is even and sit in neighbouring lanes (or
// in lane 63 and lane 0 of the next slot pair) when D is odd.  Both are read once, wave-uniform, before the row loop.
//
// The order of operations of one evaluation:
//   0. s_tau, s and the reciprocal prior scales 1 / sigma_tau^2, 1 / sigma_0^2 are taken from their lanes (readlane).
//      tau = wnd::dexp(s_tau), scale = wnd::dexp(s), 1 / tau^2 = 1.0 / (tau * tau) (centered only) and Family::consts(s,
//      scale) -- the normal's 1 / sigma^2; the negative binomial's phi = 1 / kappa and the wnd::GammaConsts of phi -- are
//      computed ONCE from the wave-uniform values, as the siblings do.
//   1. the priors of beta and z as in hier_glm.h; the slots of u, s_tau and s start their gradient at 0.
//   2. per block of B = 32 / EPL rows, hier_glm.h's block pass: two rows' dot products per packed butterfly into lanes
//      k, k + 1 of eta; the group of row k made wave-uniform and the effect u_g gathered from its owner lane by readlane
//      (times tau, a rounded product, when non-centered) and ADDED to eta; then the offset is added; then the family's
//      row term on lanes 0..B-1 at once: Family::term(eta, y, consts) gives the row's log-likelihood, r = dll/deta and
//      the lane's partial of d/ds.  Without weights the term adds into the lane's running sums ll and ds; with weights
//      it is evaluated with zero running sums and ds = ds + w * ds_n (a rounded product, then the add), ll = mad(w, t,
//      ll), r = w * r, a row with w == 0 discarded by select -- glm_scale.h's weighted form to the letter.
//      The residual of row k, broadcast, feeds g_beta from the registers that hold the rows and is added into S_g in the
//      owner lane's slot of coordinate P + g, rows in order (no atomics: the CPU emulation gives the same bits).
//   3. epilogue: the two sums over the lanes -- sum_j z_j S_j (or sum_j a_j^2) and sum ds -- go through ONE packed
//      butterfly (cx.sum2: the first in lanes 0-31, the second in lanes 32-63).  Then hier_glm.h's formulas for u and
//      s_tau with tau^2 / sigma_tau^2 = tau * tau * isig_tau2, and glm_scale.h's for s with exp(2 s) / sigma_0^2 =
//      scale * scale * isig0.  logp receives the s_tau term in the lane that owns D - 2 and the s term in the lane that
//      owns D - 1, in slot order.
// A non-finite tau or scale (a log scale beyond about +-709) takes no path of its own: the energy turns non-finite and
// the trajectory treats it as every non-finite energy.
//
// The pointwise, predict and replicate hooks follow the siblings' rules: eta is formed as eval()'s weighted path forms
// it (glm.h's pointwise_eta over the P columns, the group effect set into the tile's lanes row by row, then the offset);
// the family's term, response or replicate is evaluated once on the full wavefront with what depends on s_tau or s alone
// computed once per draw and tile; the row constant is Family::pointwise_const; y and the weights are never read in
// predict or replicate.
#pragma once

#include "glm_scale.h"
#include "hier_glm.h"

namespace wn {

template <class Family, bool Centered>
struct HierScaleGlmModel {
  static constexpr bool kUsesParams = true;  // [s2_0 .. s2_{P-1} | 1 .. 1 | sigma_tau | sigma_0]
  static constexpr bool kUsesData = true;
  static constexpr bool kUsesGroups = true;
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
    const int J = cx.num_groups();
    const int P = D - J - 2;
    const int nx = (P + 127) >> 7;  // slot pairs that hold columns of x
    const double st = coord_value(th, D - 2);
    const double s = coord_value(th, D - 1);
    const double isigt = coord_value(mp, D - 2);  // 1 / sigma_tau^2 (host_params)
    const double isig0 = coord_value(mp, D - 1);  // 1 / sigma_0^2
    const double tau = wnd::dexp(st, cx.uniform_tab());
    const double itau2 = Centered ? 1.0 / (tau * tau) : 0.0;
    const double scale = wnd::dexp(s, cx.uniform_tab());
    const typename Family::Consts kc = Family::consts(s, scale, cx.uniform_tab());
    // beta: the prior as in glm.h; z (non-centered): -1/2 z^2; u slots start S_j at 0; the scales: the epilogue
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
    double ds = 0.0;  // ... and their derivatives with respect to s
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
        const double vk = coord_value(th, gk[k]);
        set_lane(v, Centered ? vk : tau * vk, k);
      }
      eta = eta + v;
      const double y = mine ? cx.obs_y(n0 + me) : 0.0;
      if (offs) eta = eta + (mine ? cx.obs_offset(n0 + me) : 0.0);
      double r, ll_new = wts ? 0.0 : ll, ds_new = wts ? 0.0 : ds;
      Family::template term<Cx>(eta, y, kc, cx.gather_tab(), r, ll_new, ds_new);
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
    cx.sum2(part, ds);  // one packed butterfly: part's sum in lanes 0-31, ds's in lanes 32-63
    const double tt = tau * tau * isigt;      // tau^2 / sigma_tau^2
    const double ss = scale * scale * isig0;  // exp(2 s) / sigma_0^2
    double gst, lpst;
    if constexpr (Centered) {
      const double q = part * itau2;  // sum_j a_j^2 / tau^2
      gst = ((q - static_cast<double>(J)) + 1.0) - tt;
      lpst = ((st - static_cast<double>(J) * st) - 0.5 * q) - 0.5 * tt;
    } else {
      gst = Cx::mad(tau, part, 1.0) - tt;
      lpst = st - 0.5 * tt;
    }
    const double gs = (ds + 1.0) - ss;
    const double lps = s - 0.5 * ss;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const int c = cx.index(j);
      const bool grp = c >= P && c < P + J;
      if constexpr (Centered) {
        g[j] = grp ? g[j] - th[j] * itau2 : g[j];
      } else {
        g[j] = grp ? Cx::mad(tau, g[j], -th[j]) : g[j];
      }
      g[j] = c == D - 2 ? gst : g[j];
      g[j] = c == D - 1 ? gs : g[j];
      if (c == D - 2) acc = acc + lpst;
      if (c == D - 1) acc = acc + lps;
    }
  }
  __device__ __forceinline__ static double finish(double sum, const Aux&, int) { return sum; }

  // eta of rows n0 .. n0 + 63 as eval()'s weighted path forms it (header comment): the dot product over the P columns,
  // the group effect row by row, then the offset
  template <int EPL, class Cx>
  __device__ __forceinline__ static double row_eta(Cx& cx, const double (&th)[EPL], int n0, bool live) {
    const int D = cx.dim();
    const int P = D - cx.num_groups() - 2;
    const double tau = Centered ? 1.0 : wnd::dexp(coord_value(th, D - 2), cx.uniform_tab());
    double eta = pointwise_eta<EPL>(cx, th, n0, live, (P + 127) >> 7);
    const int n = n0 + opaque_lane_id();
    const int grp = live ? cx.obs_group(n) : 0;
    const int liv = live ? 1 : 0;
    double v = 0.0;
    for (int k = 0; k < 64; ++k) {
      if (lane_value(liv, k) == 0) continue;
      const double vk = coord_value(th, P + lane_value(grp, k));
      set_lane(v, Centered ? vk : tau * vk, k);
    }
    eta = eta + v;
    if (cx.has_offset()) eta = eta + (live ? cx.obs_offset(n) : 0.0);
    return eta;
  }

  // the pointwise hook (header comment): lane k's likelihood term of row n0 + k, constant dropped
  static constexpr bool kPointwise = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static double pointwise(Cx& cx, const double (&th)[EPL], int n0, bool live) {
    const double s = coord_value(th, cx.dim() - 1);
    const double scale = wnd::dexp(s, cx.uniform_tab());
    const typename Family::Consts kc = Family::consts(s, scale, cx.uniform_tab());
    const double eta = row_eta<EPL>(cx, th, n0, live);
    const double y = live ? cx.obs_y(n0 + opaque_lane_id()) : 0.0;
    double r, ll = 0.0, ds = 0.0;
    Family::template term<Cx>(eta, y, kc, cx.gather_tab(), r, ll, ds);
    return ll;
  }
  static long double pointwise_const(double y) { return Family::pointwise_const(y); }

  // the predict hook (header comment): lane k's (eta, mu, v) of row n0 + k
  static constexpr bool kPredict = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static void predict(Cx& cx, const double (&th)[EPL], int n0, bool live, double& eta,
                                                 double& mu, double& v) {
    const double scale = wnd::dexp(coord_value(th, cx.dim() - 1), cx.uniform_tab());
    eta = row_eta<EPL>(cx, th, n0, live);
    Family::template response<Cx>(eta, scale, mu, v, cx.gather_tab());
  }

  // the replicate hook (header comment): predict()'s triple and y_rep of row n0 + k
  static constexpr bool kReplicate = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static void replicate(Cx& cx, const double (&th)[EPL], int n0, bool live, RepStream& rng,
                                                   double& eta, double& mu, double& v, double& yrep) {
    const double scale = wnd::dexp(coord_value(th, cx.dim() - 1), cx.uniform_tab());
    eta = row_eta<EPL>(cx, th, n0, live);
    Family::template response<Cx>(eta, scale, mu, v, cx.gather_tab());
    yrep = Family::replicate(mu, scale, rng, cx.gather_tab());
  }

  // host side: the beta prior variances and the reserved entries -> reciprocals, sigma_tau and sigma_0 -> 1 / sigma^2
  // (each rounded once); the observations' checks are the family's
  static void host_params(double* mp, int num_params) {
    for (int i = 0; i < num_params; ++i)
      if (!(mp[i] > 0) || !std::isfinite(mp[i]))
        throw std::invalid_argument("model_params (prior variances, reserved entries, sigma_tau, sigma_0) must be positive "
                                    "and finite");
    for (int i = 0; i + 2 < num_params; ++i) mp[i] = 1.0 / mp[i];
    for (int i = num_params > 2 ? num_params - 2 : 0; i < num_params; ++i) mp[i] = 1.0 / (mp[i] * mp[i]);
  }
  static void host_data(const double*, const double* y, int num_obs, int, bool weighted) {
    for (int n = 0; n < num_obs; ++n) Family::check_y(y[n], weighted);
  }
  static void validate(int num_params) {
    if (num_params > 1024)
      throw std::invalid_argument("a data model supports 1 <= num_params <= 1024 (one wavefront per chain), got " +
                                  std::to_string(num_params));
  }
};

using HierLinearRegressionSigmaModel = HierScaleGlmModel<NormalSigmaFamily, false>;
using HierLinearRegressionSigmaCenteredModel = HierScaleGlmModel<NormalSigmaFamily, true>;
// The template takes NegBinomialFamily as well, but no negative binomial instantiation is registered: on the MI355X its
// sampling kernel at sixteen elements per lane did not reproduce the emulation's bits with fused multiply-add (DESIGN.md
// 3.8.10), and the cause is not found.

}  // namespace wn
