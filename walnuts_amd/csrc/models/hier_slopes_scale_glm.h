// models/hier_slopes_scale_glm.h -- hierarchical regression with varying intercepts AND slopes by group AND an estimated
// scale: the varying coefficients of models/hier_slopes_glm.h with the families of models/glm_scale.h (wn_model_api.h,
// kUsesData + kUsesGroups + kVaryingSlopes + kScaleParam), non-centered: y ~ x + (1 + x_0 + .. | g) with Gaussian noise of
// unknown sigma, one template over the family (the alias at the end says which instantiation the library registers).
//
// Q = cx.num_varying() coefficients vary by group: the intercept and the slopes of the FIRST Q - 1 columns of x.
//   theta = [beta_0 .. beta_{P-1} | u_{0,0..J-1} | .. | u_{Q-1,0..J-1} | s_0 .. s_{Q-1} | s],   D = P + Q (J + 1) + 1
//   z_{n,0} = 1,  z_{n,q} = x_{n,q-1} (q >= 1),  tau_q = exp(s_q),  scale = exp(s),  g(n) in [0, J)
//   model_params [D]: the prior variances s2_i of beta, Q J reserved entries (1), the half-normal scales sigma_q of
//   tau_q, the half-normal scale sigma_0 of exp(s)
//   eta_n = x_n . beta + sum_q tau_q u_{q,g(n)} z_{n,q}  (+ offset_n)
//   logp  = sum_n w_n ll_n(eta_n, y_n, s) - 1/2 sum_i beta_i^2 / s2_i - 1/2 sum_{q,j} u_{q,j}^2
//           + sum_q (s_q - tau_q^2 / (2 sigma_q^2)) + (s - exp(2 s) / (2 sigma_0^2))
//   r_n = w_n dll_n/deta,  S_{q,j} = sum_{n in group j} r_n z_{n,q}
//   d/du_{q,j} = tau_q S_{q,j} - u_{q,j},   d/ds_q = tau_q sum_j u_{q,j} S_{q,j} + 1 - tau_q^2 / sigma_q^2,
//   d/ds = sum_n w_n dll_n/ds + 1 - exp(2 s) / sigma_0^2,   d/dbeta as glm.h
// (constants dropped).  x has P = D - Q (J + 1) - 1 columns at the grouped stride Dx = 128 ceil(P / 128): no scale is ever
// a column.  At Q = 1 the layout, the parameter vector and every formula are those of hier_scale_glm.h's non-centered
// model, and so are the bits; what Q > 1 adds sits behind wave-uniform tests.  With s = 0 the likelihood is
// hier_slopes_glm.h's unit-noise one.
//
// ORDER OF OPERATIONS of one evaluation:
//   0. tau_q = wnd::dexp(s_q) of the wave-uniform s_q in a wave-uniform loop, lane q keeping tau_q (hier_slopes_glm.h's
//      taus with the s_q one coordinate earlier); s and 1 / sigma_0^2 from their lane, scale = wnd::dexp(s) and
//      Family::consts(s, scale) ONCE, before the row loop.
//   1. the priors of beta and u as in the siblings; the slots of u, s_q and s start their gradient at 0.
//   2. per block of B = 32 / EPL rows, hier_slopes_glm.h's block pass (gather: v = tau_0 u_0; v = mad(tau_q u_q, z_q, v)
//      for ascending q; eta = eta + v; then the offset) with Link::term replaced by Family::term, and the lane's partial
//      of d/ds handled as in hier_scale_glm.h: without weights the term adds into the running sums ll and ds, with
//      weights it is evaluated with zero running sums and ds = ds + w * ds_n (a rounded product, then the add), a row
//      with w == 0 discarded by select.  The scatter is hier_slopes_glm.h's, rows in order, no atomics.
//   3. epilogue: at q = 0, sum_j u_{0,j} S_{0,j} and ds go through ONE packed butterfly (cx.sum2, as in
//      hier_scale_glm.h); at q >= 1, cx.sum1 (as in hier_slopes_glm.h).  Then the siblings' formulas: the u slots of block
//      q become Cx::mad(tau_q, S, -u), coordinate D - 1 - Q + q gets Cx::mad(tau_q, sum, 1) - tau_q^2 isig2_q, coordinate
//      D - 1 gets (ds + 1) - scale^2 isig0; the owning lanes add s_q - 1/2 tau_q^2 isig2_q and s - 1/2 scale^2 isig0 to
//      the log density in slot order (the scales are consecutive coordinates, so within a lane ascending q, then s).
// No array is indexed at run time and nothing is unrolled Q times (Q <= 8, kMaxVaryingCoefficients in wn_launch.h).  A
// non-finite tau_q or scale (a log scale beyond about +-709) takes no path of its own: the energy turns non-finite and
// the trajectory treats it as every non-finite energy.
//
// pointwise(), predict(), replicate(): hier_slopes_glm.h's tile_eta (with this layout's P and scales), the offset, then
// Family::term / response / replicate ONCE on the full wavefront, scale computed once per draw and tile; the row
// constant is Family::pointwise_const; y and the weights are never read in predict or replicate.
#pragma once

#include "glm_scale.h"
#include "hier_slopes_glm.h"

namespace wn {

template <class Family>
struct HierSlopesScaleGlmModel {
  static constexpr bool kUsesParams = true;  // [s2_0 .. s2_{P-1} | 1 .. 1 (Q J) | sigma_0 .. sigma_{Q-1} | sigma_0 of s]
  static constexpr bool kUsesData = true;
  static constexpr bool kUsesGroups = true;
  static constexpr bool kVaryingSlopes = true;
  static constexpr bool kScaleParam = true;
  static constexpr bool kUsesRowTerms = true;
  static constexpr bool kElementwise = false;
  static constexpr bool kGradIsNegTheta = false;
  static constexpr bool kCheapGrad = false;
  __device__ __forceinline__ static double grad_elem(double, double) { return 0.0; }
  struct Aux {};

  using Slopes = HierSlopesGlmModel<IdentityLink>;  // coord, row_z: the layout helpers, no link in them

  template <int EPL>
  static constexpr int kBlock = GlmModel<IdentityLink>::template kBlock<EPL>;

  // tau_q = exp(s_q) in lane q (0 elsewhere); s_q is coordinate D - 1 - Q + q
  template <int EPL, class Cx>
  __device__ __forceinline__ static double taus(Cx& cx, const double (&th)[EPL], int D, int Q) {
    double tauv = 0.0;
    for (int q = 0; q < Q; ++q) set_lane(tauv, wnd::dexp(coord_value(th, D - 1 - Q + q), cx.uniform_tab()), q);
    return tauv;
  }

  template <int EPL, class Cx>
  __device__ __forceinline__ static void eval(Cx& cx, const double (&th)[EPL], double (&g)[EPL],
                                              const double (&mp)[EPL], Aux&, double& acc) {
    static_assert(Cx::L == 64, "data models run one wavefront per chain");
    constexpr int B = kBlock<EPL>;
    static_assert(B % 2 == 0 && B <= 64, "rows are reduced in pairs");
    const int D = cx.dim();
    const int J = cx.num_groups();
    const int Q = cx.num_varying();
    const int P = D - Q * (J + 1) - 1;
    const int U = P + Q * J;        // one past the last group effect
    const int nx = (P + 127) >> 7;  // slot pairs that hold columns of x
    const double tauv = taus<EPL>(cx, th, D, Q);
    const double tau0 = lane_value(tauv, 0);
    const double s = coord_value(th, D - 1);
    const double isig0 = coord_value(mp, D - 1);  // 1 / sigma_0^2 (host_params)
    const double scale = wnd::dexp(s, cx.uniform_tab());
    const typename Family::Consts kc = Family::consts(s, scale, cx.uniform_tab());
    // beta: the prior as in glm.h; u: -1/2 u^2; u slots start S at 0; the scales: the epilogue
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const int c = cx.index(j);
      const bool beta = c < P;
      const bool grp = c >= P && c < U;
      g[j] = beta ? -th[j] * mp[j] : 0.0;
      if (beta) acc = Cx::mad(-0.5 * th[j] * th[j], mp[j], acc);
      if (grp) acc = Cx::mad(-0.5 * th[j], th[j], acc);
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
        set_lane(v, tau0 * vk, k);
      }
      if (Q > 1) {
        for (int q = 1; q < Q; ++q) {
          double uq = 0.0, zq = 0.0;
#pragma unroll
          for (int k = 0; k < B; ++k) {
            set_lane(uq, coord_value(th, gk[k] + q * J), k);
            set_lane(zq, Slopes::row_z(x[k], q), k);
          }
          v = Cx::mad(lane_value(tauv, q) * uq, zq, v);
        }
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
      if (Q > 1) {
        for (int q = 1; q < Q; ++q) {
          double zq = 0.0;
#pragma unroll
          for (int k = 0; k < B; ++k) set_lane(zq, Slopes::row_z(x[k], q), k);
          const double rz = r * zq;  // lane k: r_k z_{k,q}
#pragma unroll
          for (int k = 0; k < B; ++k) {
            const double a = lane_value(rz, k);
            const int c = gk[k] + q * J;
            const int slot = 2 * (c >> 7) + (c & 1);
            const bool owner = me == ((c >> 1) & 63);
#pragma unroll
            for (int j = 0; j < EPL; ++j) g[j] = (owner && j == slot) ? g[j] + a : g[j];
          }
        }
      }
    }
    acc = acc + ll;
    // epilogue: g[j] holds S_{q,j} in the u slots
    for (int q = 0; q < Q; ++q) {
      const int lo = P + q * J, hi = lo + J, cs = D - 1 - Q + q;
      double part = 0.0;  // sum_j u_{q,j} S_{q,j}
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        const int c = cx.index(j);
        if (c >= lo && c < hi) part = Cx::mad(th[j], g[j], part);
      }
      if (q == 0) {
        cx.sum2(part, ds);  // one packed butterfly: part's sum in lanes 0-31, ds's in lanes 32-63
      } else {
        part = cx.sum1(part);
      }
      const double sq = coord_value(th, cs);
      const double isig2 = coord_value(mp, cs);  // 1 / sigma_q^2 (host_params)
      const double tau = lane_value(tauv, q);
      const double tt = tau * tau * isig2;  // tau_q^2 / sigma_q^2
      const double gsq = Cx::mad(tau, part, 1.0) - tt;
      const double lpsq = sq - 0.5 * tt;
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        const int c = cx.index(j);
        const bool grp = c >= lo && c < hi;
        g[j] = grp ? Cx::mad(tau, g[j], -th[j]) : g[j];
        g[j] = c == cs ? gsq : g[j];
        if (c == cs) acc = acc + lpsq;
      }
    }
    const double ss = scale * scale * isig0;  // exp(2 s) / sigma_0^2
    const double gs = (ds + 1.0) - ss;
    const double lps = s - 0.5 * ss;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const int c = cx.index(j);
      g[j] = c == D - 1 ? gs : g[j];
      if (c == D - 1) acc = acc + lps;
    }
  }
  __device__ __forceinline__ static double finish(double sum, const Aux&, int) { return sum; }

  // eta of rows n0 .. n0 + 63, row n0 + k in lane k, with the offset: hier_slopes_glm.h's tile_eta in this layout
  template <int EPL, class Cx>
  __device__ __forceinline__ static double row_eta(Cx& cx, const double (&th)[EPL], int n0, bool live) {
    const int D = cx.dim();
    const int J = cx.num_groups();
    const int Q = cx.num_varying();
    const int P = D - Q * (J + 1) - 1;
    const double tauv = taus<EPL>(cx, th, D, Q);
    const double tau0 = lane_value(tauv, 0);
    double eta = pointwise_eta<EPL>(cx, th, n0, live, (P + 127) >> 7);
    const int n = n0 + opaque_lane_id();
    const int grp = live ? cx.obs_group(n) : 0;
    const int liv = live ? 1 : 0;
    double v = 0.0;
    for (int k = 0; k < 64; ++k) {
      if (lane_value(liv, k) == 0) continue;
      const double vk = coord_value(th, P + lane_value(grp, k));
      set_lane(v, tau0 * vk, k);
    }
    if (Q > 1) {
      for (int q = 1; q < Q; ++q) {
        const double zq = live ? cx.obs_x(n, q - 1) : 0.0;
        double uq = 0.0;
        for (int k = 0; k < 64; ++k) {
          if (lane_value(liv, k) == 0) continue;
          set_lane(uq, coord_value(th, P + q * J + lane_value(grp, k)), k);
        }
        const double vq = Cx::mad(lane_value(tauv, q) * uq, zq, v);
        v = live ? vq : v;
      }
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

  // host side (ModelOps::host_params_varying: the engine hands in Q): the beta prior variances and the reserved
  // entries -> reciprocals, the last Q + 1 entries (sigma_q, sigma_0) -> 1 / sigma^2 (each rounded once); the
  // observations' checks are the family's
  static void host_params(double* mp, int num_params, int num_varying) {
    for (int i = 0; i < num_params; ++i)
      if (!(mp[i] > 0) || !std::isfinite(mp[i]))
        throw std::invalid_argument("model_params (prior variances, reserved entries, sigma_q, sigma_0) must be positive "
                                    "and finite");
    const int first = num_params > num_varying + 1 ? num_params - num_varying - 1 : 0;
    for (int i = 0; i < first; ++i) mp[i] = 1.0 / mp[i];
    for (int i = first; i < num_params; ++i) mp[i] = 1.0 / (mp[i] * mp[i]);
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

using HierLinearRegressionSlopesSigmaModel = HierSlopesScaleGlmModel<NormalSigmaFamily>;

}  // namespace wn
