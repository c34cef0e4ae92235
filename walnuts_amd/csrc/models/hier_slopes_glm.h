// models/hier_slopes_glm.h -- hierarchical (multilevel) regression with varying intercepts AND slopes by group,
// non-centered, on an observation block with a group channel (wn_model_api.h, kUsesData + kUsesGroups +
// kVaryingSlopes): linear (unit noise), logistic and Poisson, one template over the link (models/glm.h).
//
// Q = cx.num_varying() coefficients vary by group: the intercept and the slopes of the FIRST Q - 1 columns of x.  The
// random effects are independent, one scale per coefficient.  Coefficient-major:
//   theta = [beta_0 .. beta_{P-1} | u_{0,0..J-1} | u_{1,0..J-1} | .. | u_{Q-1,0..J-1} | s_0 .. s_{Q-1}],  D = P + Q J + Q
//   z_{n,0} = 1,  z_{n,q} = x_{n,q-1} (q >= 1),  tau_q = exp(s_q),  g(n) in [0, J) the group of observation n
//   model_params [D]: the prior variances s2_i of beta, Q J reserved entries (1), the half-normal scales sigma_q
//   eta_n = x_n . beta + sum_q tau_q u_{q,g(n)} z_{n,q}  (+ offset_n)
//   logp  = sum_n w_n ll_n(eta_n, y_n) - 1/2 sum_i beta_i^2 / s2_i - 1/2 sum_{q,j} u_{q,j}^2
//           + sum_q (s_q - tau_q^2 / (2 sigma_q^2))           (half-normal on tau_q, in log space, with its Jacobian)
//   S_{q,j} = sum_{n in group j} r_n z_{n,q}                  (r_n the link's residual, weighted as in glm.h)
//   d/du_{q,j} = tau_q S_{q,j} - u_{q,j},   d/ds_q = tau_q sum_j u_{q,j} S_{q,j} + 1 - tau_q^2 / sigma_q^2,
//   d/dbeta as glm.h
// (constants dropped).  At Q = 1 the layout, the parameter vector and every formula are those of hier_glm.h's
// non-centered models, and so are the bits: the operations below are hier_glm.h's, in its order, and what Q > 1 adds
// sits behind wave-uniform tests.  x has P = num_params - Q (J + 1) columns at the narrow stride Dx = 128 ceil(P / 128).
//
// The row pass is hier_glm.h's (blocks of B = 32 / EPL rows held in registers, two rows per packed butterfly, the link
// of a block in one vector evaluation on lanes 0..B-1).  ORDER OF OPERATIONS, per block:
//   gather   rows k = 0..B-1 in order: the group is made wave-uniform, v_k = tau_0 * u_{0,g} is set into lane k
//            (hier_glm.h's step 1).  Then, only if Q > 1, for q = 1..Q-1 ascending (a wave-uniform run-time loop):
//            u_{q,g(k)} (owner lane of coordinate P + q J + g, a select and a readlane) and z_{k,q} (coordinate q - 1 of
//            the row in registers) are set into lane k for every row k, and ONE vector operation forms
//            v = Cx::mad(tau_q * u_q, z_q, v).  Then eta = eta + v, then the offset (glm.h).
//            Lane k therefore computes  v = tau_0 u_0;  v = mad(tau_q u_q, z_q, v) for ascending q;  eta = eta + v.
//   scatter  after the link, rows k in order: r_k goes into beta's gradient (glm.h) and into the owner lane's slot of
//            coordinate P + g (hier_glm.h's step 2: the addend of q = 0 is r_k itself).  Then, only if Q > 1, for
//            q = 1..Q-1 ascending: the vector r * z_q is formed once (lane k: r_k z_{k,q}, one rounded product), and for
//            rows k in order lane k's product is added into the owner lane's slot of coordinate P + q J + g.  A slot
//            belongs to one (q, j), so every S_{q,j} receives its rows in order whatever the order of q: no atomics,
//            nothing depends on scheduling, and the CPU emulation of this source gives the same bits.
//   epilogue for q = 0..Q-1 ascending: one cx.sum1 of sum_j u_{q,j} S_{q,j} (slot order, Cx::mad), the u slots of block
//            q become Cx::mad(tau_q, S, -u), coordinate D - Q + q gets g_s = Cx::mad(tau_q, sum, 1) - tau_q^2 isig2_q
//            and its lane adds s_q - 1/2 tau_q^2 isig2_q to the log density.
// tau_q = wnd::dexp(s_q) of the wave-uniform s_q, once per evaluation, in a wave-uniform loop (nothing diverges around
// the table reads, wn_devrand.h); lane q keeps tau_q, and a wave-uniform readlane hands it to the loops over q, so no
// array is indexed at run time and nothing is unrolled Q times (hence Q <= 8, kMaxVaryingCoefficients in wn_launch.h;
// the engine refuses more).  A non-finite tau_q (s_q beyond +-709) takes no path
// of its own: the energy turns non-finite and the trajectory treats it as every non-finite energy.  Rows a partial
// last block does not have are zeros with residual 0 (select), so their products vanish or are discarded.
//
// pointwise(), predict(), replicate() (glm.h's header): glm.h's pointwise_eta over the P columns, the group terms of the
// tile's rows set into their lanes in the order above, the offset, then Link::term / response / replicate ONCE on the
// full wavefront.  The tile's rows are streamed, not kept, so lane k reads z of its own row n0 + k with one per-lane
// load per q (cx.obs_x(n, q - 1)).
#pragma once

#include "glm.h"

namespace wn {

template <class Link>
struct HierSlopesGlmModel {
  static constexpr bool kUsesParams = true;  // [s2_0 .. s2_{P-1} | 1 .. 1 (Q J) | sigma_0 .. sigma_{Q-1}]
  static constexpr bool kUsesData = true;
  static constexpr bool kUsesGroups = true;
  static constexpr bool kVaryingSlopes = true;
  static constexpr bool kUsesRowTerms = true;
  static constexpr bool kElementwise = false;
  static constexpr bool kGradIsNegTheta = false;
  static constexpr bool kCheapGrad = false;
  __device__ __forceinline__ static double grad_elem(double, double) { return 0.0; }
  struct Aux {};

  template <int EPL>
  static constexpr int kBlock = GlmModel<Link>::template kBlock<EPL>;

  template <int EPL>
  __device__ __forceinline__ static double coord(const double (&v)[EPL], int c) {
    return coord_value(v, c);
  }
  // z_q (q >= 1, wave-uniform) of a row held in registers: its coordinate q - 1 < 7, which slot 0 or 1 of lane
  // (q - 1) / 2 holds -- coord_value's answer without its select over all EPL slots.  (Both slots are read into values
  // first: a select between the two ELEMENTS is a select between addresses, which keeps the block's rows in scratch.)
  template <int EPL>
  __device__ __forceinline__ static double row_z(const double (&x)[EPL], int q) {
    const int c = q - 1;
    const double z0 = x[0], z1 = x[1];
    return lane_value((c & 1) ? z1 : z0, c >> 1);
  }
  // tau_q = exp(s_q) in lane q (0 elsewhere); s_q is coordinate D - Q + q
  template <int EPL, class Cx>
  __device__ __forceinline__ static double taus(Cx& cx, const double (&th)[EPL], int D, int Q) {
    double tauv = 0.0;
    for (int q = 0; q < Q; ++q) set_lane(tauv, wnd::dexp(coord(th, D - Q + q), cx.uniform_tab()), q);
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
    const int P = D - Q * (J + 1);
    const int U = P + Q * J;            // one past the last group effect
    const int nx = (P + 127) >> 7;  // slot pairs that hold columns of x
    const double tauv = taus<EPL>(cx, th, D, Q);
    const double tau0 = lane_value(tauv, 0);
    // beta: the prior as in glm.h; u: -1/2 u^2; u slots start S at 0
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
        set_lane(v, tau0 * vk, k);
      }
      if (Q > 1) {
        for (int q = 1; q < Q; ++q) {
          double uq = 0.0, zq = 0.0;
#pragma unroll
          for (int k = 0; k < B; ++k) {
            set_lane(uq, coord(th, gk[k] + q * J), k);
            set_lane(zq, row_z(x[k], q), k);
          }
          v = Cx::mad(lane_value(tauv, q) * uq, zq, v);
        }
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
      if (Q > 1) {
        for (int q = 1; q < Q; ++q) {
          double zq = 0.0;
#pragma unroll
          for (int k = 0; k < B; ++k) set_lane(zq, row_z(x[k], q), k);
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
      const int lo = P + q * J, hi = lo + J, cs = D - Q + q;
      double part = 0.0;  // sum_j u_{q,j} S_{q,j}
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        const int c = cx.index(j);
        if (c >= lo && c < hi) part = Cx::mad(th[j], g[j], part);
      }
      const double sum = cx.sum1(part);
      const double s = coord(th, cs);
      const double isig2 = coord(mp, cs);  // 1 / sigma_q^2 (host_params)
      const double tau = lane_value(tauv, q);
      const double tt = tau * tau * isig2;  // tau_q^2 / sigma_q^2
      const double gs = Cx::mad(tau, sum, 1.0) - tt;
      const double lps = s - 0.5 * tt;
#pragma unroll
      for (int j = 0; j < EPL; ++j) {
        const int c = cx.index(j);
        const bool grp = c >= lo && c < hi;
        g[j] = grp ? Cx::mad(tau, g[j], -th[j]) : g[j];
        g[j] = c == cs ? gs : g[j];
        if (c == cs) acc = acc + lps;
      }
    }
  }
  __device__ __forceinline__ static double finish(double sum, const Aux&, int) { return sum; }

  // eta of rows n0 .. n0 + 63, row n0 + k in lane k, without the offset (header comment): what the three hooks share
  template <int EPL, class Cx>
  __device__ __forceinline__ static double tile_eta(Cx& cx, const double (&th)[EPL], int n0, bool live) {
    const int D = cx.dim();
    const int J = cx.num_groups();
    const int Q = cx.num_varying();
    const int P = D - Q * (J + 1);
    const double tauv = taus<EPL>(cx, th, D, Q);
    const double tau0 = lane_value(tauv, 0);
    double eta = pointwise_eta<EPL>(cx, th, n0, live, (P + 127) >> 7);
    const int n = n0 + opaque_lane_id();
    const int grp = live ? cx.obs_group(n) : 0;
    const int liv = live ? 1 : 0;
    double v = 0.0;
    for (int k = 0; k < 64; ++k) {
      if (lane_value(liv, k) == 0) continue;
      const double vk = coord(th, P + lane_value(grp, k));
      set_lane(v, tau0 * vk, k);
    }
    if (Q > 1) {
      for (int q = 1; q < Q; ++q) {
        const double zq = live ? cx.obs_x(n, q - 1) : 0.0;
        double uq = 0.0;
        for (int k = 0; k < 64; ++k) {
          if (lane_value(liv, k) == 0) continue;
          set_lane(uq, coord(th, P + q * J + lane_value(grp, k)), k);
        }
        const double vq = Cx::mad(lane_value(tauv, q) * uq, zq, v);
        v = live ? vq : v;
      }
    }
    return eta + v;
  }

  // the pointwise hook (header comment): lane k's likelihood term of row n0 + k, constant dropped
  static constexpr bool kPointwise = true;
  template <int EPL, class Cx>
  __device__ __forceinline__ static double pointwise(Cx& cx, const double (&th)[EPL], int n0, bool live) {
    double eta = tile_eta<EPL>(cx, th, n0, live);
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
    eta = tile_eta<EPL>(cx, th, n0, live);
    if (cx.has_offset()) eta = eta + (live ? cx.obs_offset(n0 + opaque_lane_id()) : 0.0);
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

  // host side (ModelOps::host_params_varying: the engine hands in Q): the beta prior variances and the reserved
  // entries -> reciprocals, sigma_q -> 1 / sigma_q^2 (each rounded once); the observations' checks are the link's
  static void host_params(double* mp, int num_params, int num_varying) {
    for (int i = 0; i < num_params; ++i)
      if (!(mp[i] > 0) || !std::isfinite(mp[i]))
        throw std::invalid_argument("model_params (prior variances, reserved entries, sigma_q) must be positive and finite");
    for (int i = 0; i < num_params - num_varying; ++i) mp[i] = 1.0 / mp[i];
    for (int i = num_params - num_varying; i < num_params; ++i) mp[i] = 1.0 / (mp[i] * mp[i]);
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

using HierLinearRegressionSlopesModel = HierSlopesGlmModel<IdentityLink>;
using HierLogisticRegressionSlopesModel = HierSlopesGlmModel<LogitLink>;
using HierPoissonRegressionSlopesModel = HierSlopesGlmModel<LogLink>;

}  // namespace wn
