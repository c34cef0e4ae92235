// wn_devrand.h -- exact samplers on the counter streams: what a data model draws when it simulates REPLICATED data
// y_rep ~ p(y | theta, x_n) from a draw (wn_replicate.h; wn_model_api.h, kReplicate).  Normal, Bernoulli, Poisson, gamma
// and negative binomial (NB2) variates, one per lane, keyed by counters: a variate depends on (seed, chain, draw, row)
// and on the distribution's arguments alone -- not on the grid, the slab, the mask or what the other lanes draw.
//
// The rules are wn_devmath.h's: binary64 + - * / sqrt, wnd::fmad and integer operations only, -ffp-contract=off, so the
// host build of this source (the CPU emulation) gives the device's bits.  Apart from the normal's one fused
// multiply-add every step below is a PLAIN rounded operation, written in the order stated here, so that a replay in
// ordinary floating point (tests/helpers/hp_replicate_reference.py) follows it operation by operation.
//
// COUNTERS.  Stream id kStreamReplicate = 4 (wn_devmath.h; kStreamVersion does not change: the streams 0-3 are
// untouched).  The Philox4x32-7 key is the caller's 64-bit seed (low word, high word); the counter is
//   (c0, c1, c2, c3) = (row n within the dataset's block of rows, draw index i within its chain,
//                       chain index c within the whole chains block, kStreamReplicate + 256 * call)
// with call = 0, 1, 2, ... numbering the Philox calls made for that (row, draw, chain) in the order the algorithm
// below states them.  (The matrix mode of wn_replicate.h has no chains: c2 is the position t and c1 = 0.)  ONE call
// yields EITHER two open-interval uniforms, u = open01(x, y) and w = open01(z, w), OR one Box-Muller pair computed
// exactly as wnd::stream_normal_pair computes it (of which the first normal is used).  Every attempt of a rejection
// loop consumes a fixed number of calls, so a replay can index them.
//
// THE ALGORITHMS (calls in this order; `call` counts what the lane's own algorithm consumed):
//   normal(mu, sd)      1 call (normals).  y = fmad(sd, z0, mu)  -- fused in BOTH arithmetic modes of the engine, so a
//                       replicate does not depend on the mode beyond its mu and sd.
//   Bernoulli(mu)       1 call (uniforms).  y = u < mu ? 1 : 0;  mu NaN -> NaN.
//   Poisson(mu)         mu NaN, negative, infinite or above kPoissonMuMax = 2^30 -> NaN, no call.  mu == 0 -> 0, no call.
//     0 < mu < 10       1 call (uniforms), inversion by sequential search on u:
//                         p = dexp(-mu); cdf = p; k = 0;
//                         while (u > cdf && k < kPoissonSearchCap) { k = k + 1; p = (p * mu) / k; cdf = cdf + p; }
//                       u <= 1 - 2^-53 and the tail beyond k = 45 is below 2^-53 at mu = 10, so the search ends there
//                       unless cdf, summed in binary64, stalls a few ulps short of a u next to 1 (probability below
//                       1e-14): the search then stops at the cap and RETURNS kPoissonSearchCap = 64.
//     10 <= mu <= 2^30  Hoermann's transformed rejection PTRS (Insurance: Mathematics and Economics 12, 1993), one call
//                       (uniforms u, V) per attempt, at most kRejectionCap = 32 attempts:
//                         smu = sqrt(mu); lmu = dlog(mu); b = 0.931 + 2.53 * smu; a = -0.059 + 0.02483 * b;
//                         inva = 1.1239 + 1.1328 / (b - 3.4); vr = 0.9277 - 3.6224 / (b - 2); linva = dlog(inva);
//                       attempt:  U = u - 0.5; us = 0.5 - |U|; k = floor((((2 * a) / us + b) * U + mu) + 0.43);
//                         k >= 0 and us >= 0.07 and V <= vr                        -> accept k
//                         k < 0, or us < 0.013 and V > us                          -> next attempt
//                         lhs = (dlog(V) + linva) - dlog(a / (us * us) + b);
//                         rhs = (k * lmu - mu) - dlgamma_diff(k, 1.0)               (the log-factorial)
//                         lhs <= rhs                                               -> accept k, otherwise next attempt
//                       PTRS accepts with probability >= 0.74 per attempt for mu >= 10 (1.13-1.33 attempts on average),
//                       so fewer than 1 sample in 1e18 reaches the cap; such a sample is NaN.
//                       Why 2^30: k * lmu, mu and the log-factorial are each ~ mu log mu and cancel to O(log mu), so the
//                       comparison carries a rounding error of a few ulps of mu log mu -- 1e-5 at 2^30, where it shifts
//                       an acceptance probability by 1e-5 relative; beyond it the sampler would stop being exact at the
//                       precision a posterior predictive check can see, and such a mean is refused rather than served.
//   gamma(shape, 1)     shape NaN, <= 0 or infinite -> NaN, no call.  Marsaglia & Tsang (ACM TOMS 26, 2000), two calls
//                       per attempt (normals z; uniforms u), at most kRejectionCap attempts (acceptance >= 0.95):
//                         d0 = shape < 1 ? shape + 1 : shape; d = d0 - RN(1/3); c = 1 / sqrt(9 * d);
//                       attempt:  t = 1 + c * z; v = (t * t) * t;
//                         v > 0 and dlog(u) < (((0.5 * z) * z + d) - d * v) + d * dlog(v)  -> G = d * v
//                       shape < 1 (the boost): one more call (uniforms u), G = G * dexp((1 / shape) * dlog(u)) -- the
//                       value wnd::dpow_pos(u, 1 / shape) returns for an exponent above 1, taken on every lane.
//                       A gamma that exhausts the cap is NaN.
//   negbin(mu, kappa)   NB2, E y = mu, Var y = mu + kappa mu^2: phi = 1 / kappa; mu NaN, negative or infinite, or phi
//                       NaN, <= 0 or infinite -> NaN, no call.  G ~ gamma(phi, 1) as above, then
//                       y ~ Poisson((mu * G) / phi) as above, its calls numbered after the gamma's.
//
// EVERY LOOP IS BOUNDED (the caps above) AND WAVE-CONVERGED.  GatherTab looks the tables up with a cross-lane shuffle
// from lane-held registers: a lane that has left a divergent loop would supply 0 to the lanes still inside it on the
// device, and block the exchange under the emulation.  So every loop runs `while (any(undecided))` with `any` a wave
// vote over all 64 lanes; finished lanes compute on and their results (and call counts) are discarded by select.  The
// two Poisson ranges, the gamma's boost and the negative binomial's stages are entered by the same wave-uniform "any
// lane needs it" test, never by a per-lane branch around a dexp / dlog / dlgamma_diff.  `Any` is WaveAny with the lane
// tables, LaneAny (the lane's own condition) with tables read from memory, where no lane waits for another.
#pragma once

#include "wn_traj.h"

namespace wn {

constexpr double kPoissonSplit = 10.0;
constexpr double kPoissonMuMax = 1073741824.0;  // 2^30
constexpr int kPoissonSearchCap = 64;
constexpr int kRejectionCap = 32;
constexpr double kGammaThird = 0.333333333333333314829616256247;  // RN(1/3)

// does the condition hold in ANY of the wavefront's 64 lanes (all of which take part)?
struct WaveAny {
  __device__ __forceinline__ bool operator()(bool c) const {
#if defined(WN_CPU_SIM)
    int v = c ? 1 : 0;
    v |= __shfl_xor(v, 32, 64);
    for (int off = 1; off < 32; off <<= 1) v |= __shfl_xor(v, off, 64);
    return v != 0;
#else
    return __builtin_amdgcn_ballot_w64(c) != 0ull;
#endif
  }
};
struct LaneAny {
  __device__ __forceinline__ bool operator()(bool c) const { return c; }
};

// the counter stream of one (row, draw, chain): header comment.  `on`: the call belongs to this lane's algorithm (the
// words are generated either way; a lane that is only keeping the wavefront company does not count them)
struct RepStream {
  uint64_t seed;
  uint32_t row, draw, chain, call;
  __device__ __forceinline__ uint32_t word() const { return wnd::kStreamReplicate + 256u * call; }
  __device__ __forceinline__ void uniforms(bool on, double& u, double& w) {
    const wnd::U4 o = wnd::philox(row, draw, chain, word(), static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
    u = wnd::open01(o.x, o.y);
    w = wnd::open01(o.z, o.w);
    call += on ? 1u : 0u;
  }
  template <class Tab>
  __device__ __forceinline__ void normals(bool on, double& z0, double& z1, const Tab& tab) {
    wnd::stream_normal_pair(seed, chain, draw, word(), row, z0, z1, tab);
    call += on ? 1u : 0u;
  }
};

template <class Tab>
__device__ __forceinline__ double sample_normal(double mu, double sd, RepStream& s, const Tab& tab) {
  double z0, z1;
  s.normals(true, z0, z1, tab);
  return wnd::fmad(sd, z0, mu);
}

__device__ __forceinline__ double sample_bernoulli(double mu, RepStream& s) {
  double u, w;
  s.uniforms(true, u, w);
  return mu != mu ? mu : (u < mu ? 1.0 : 0.0);
}

template <class Tab, class Any>
__device__ __forceinline__ double sample_poisson(double mu, RepStream& s, const Tab& tab, const Any& any) {
  const double nan = __builtin_nan("");
  const bool valid = mu >= 0.0 && mu <= kPoissonMuMax;
  const bool small = valid && mu > 0.0 && mu < kPoissonSplit;
  const bool large = valid && mu >= kPoissonSplit;
  double y = valid ? 0.0 : nan;
  if (any(small)) {
    const double m = small ? mu : 1.0;  // (a lane that only keeps company computes on a harmless mean)
    double u, w;
    s.uniforms(small, u, w);
    double p = wnd::dexp(-m, tab), cdf = p, k = 0.0;
    bool go = small && u > cdf;
    for (int it = 0; it < kPoissonSearchCap && any(go); ++it) {
      const double k1 = k + 1.0;
      const double p1 = (p * m) / k1;
      const double c1 = cdf + p1;
      k = go ? k1 : k;
      p = go ? p1 : p;
      cdf = go ? c1 : cdf;
      go = go && u > cdf;
    }
    y = small ? k : y;
  }
  if (any(large)) {
    const double m = large ? mu : kPoissonSplit;
    const double smu = __builtin_sqrt(m), lmu = wnd::dlog(m, tab);
    const double b = 0.931 + 2.53 * smu;
    const double a = -0.059 + 0.02483 * b;
    const double inva = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    const double linva = wnd::dlog(inva, tab);
    const wnd::GammaConsts one = wnd::gamma_consts(1.0, tab);
    bool todo = large;
    for (int att = 0; att < kRejectionCap && any(todo); ++att) {
      double u, V;
      s.uniforms(todo, u, V);
      const double U = u - 0.5;
      const double us = 0.5 - __builtin_fabs(U);
      const double k = __builtin_floor((((2.0 * a) / us + b) * U + m) + 0.43);
      const bool neg = !(k >= 0.0);
      const bool fast = !neg && us >= 0.07 && V <= vr;
      const bool skip = neg || (us < 0.013 && V > us);
      const double kk = neg ? 0.0 : k;
      double lg, dg;
      wnd::dlgamma_digamma_diff(kk, one, tab, lg, dg);
      const double lhs = (wnd::dlog(V, tab) + linva) - wnd::dlog(a / (us * us) + b, tab);
      const double rhs = (kk * lmu - m) - lg;
      const bool acc = fast || (!skip && lhs <= rhs);
      y = (todo && acc) ? k : y;
      todo = todo && !acc;
    }
    y = todo ? nan : y;
  }
  return y;
}

template <class Tab, class Any>
__device__ __forceinline__ double sample_gamma(double shape, RepStream& s, const Tab& tab, const Any& any) {
  const double nan = __builtin_nan("");
  const bool valid = shape > 0.0 && shape < __builtin_inf();
  double g = nan;
  if (any(valid)) {
    const double a0 = valid ? shape : 1.0;
    const bool boost = valid && a0 < 1.0;
    const double d0 = boost ? a0 + 1.0 : a0;
    const double d = d0 - kGammaThird;
    const double c = 1.0 / __builtin_sqrt(9.0 * d);
    bool todo = valid;
    for (int att = 0; att < kRejectionCap && any(todo); ++att) {
      double z, z1, u, w;
      s.normals(todo, z, z1, tab);
      s.uniforms(todo, u, w);
      const double t = 1.0 + c * z;
      const double v = (t * t) * t;
      const bool ok = v > 0.0;
      const double lv = wnd::dlog(ok ? v : 1.0, tab);
      const double rhs = (((0.5 * z) * z + d) - d * v) + d * lv;
      const double lu = wnd::dlog(u, tab);  // (ahead of the test: `ok && dlog(...)` would let a lane skip the look-up)
      const bool acc = ok && lu < rhs;
      g = (todo && acc) ? d * v : g;
      todo = todo && !acc;
    }
    if (any(boost)) {
      double u, w;
      s.uniforms(boost, u, w);
      const double pw = wnd::dexp((1.0 / a0) * wnd::dlog(u, tab), tab);
      g = boost ? g * pw : g;
    }
  }
  return g;
}

template <class Tab, class Any>
__device__ __forceinline__ double sample_negbin(double mu, double kappa, RepStream& s, const Tab& tab, const Any& any) {
  const double nan = __builtin_nan("");
  const double inf = __builtin_inf();
  const double phi = 1.0 / kappa;
  const bool valid = mu >= 0.0 && mu < inf && phi > 0.0 && phi < inf;
  const double g = sample_gamma(valid ? phi : nan, s, tab, any);
  const double lam = (mu * g) / phi;
  return sample_poisson(valid ? lam : nan, s, tab, any);
}

// the probe's and the tests' numbering of the samplers
constexpr int kSampleNormal = 0, kSampleBernoulli = 1, kSamplePoisson = 2, kSampleGamma = 3, kSampleNegBin = 4;

}  // namespace wn
