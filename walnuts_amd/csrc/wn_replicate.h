// wn_replicate.h -- SIMULATED REPLICATES of a data model on the device, y_rep ~ p(y | theta, x_n), and the posterior
// predictive checks folded from them where the draws live.
//
// (wn_model_api.h, kReplicate: Model::replicate() leaves in lane k the triple (eta, mu, v) of row n0 + k of a tile of 64
// rows -- predict()'s, by the same expression -- and y_rep, drawn ONCE on the full wavefront by Link::replicate /
// Family::replicate from the lane's counter stream.)  The samplers, their counter layout, their caps and what they refuse
// are wn_devrand.h's: the stream of a replicate is keyed by (seed; row n0 + k within the block of rows, draw i within its
// chain, chain c within the whole chains block), so a replicate depends on nothing but its key and the row's mu and scale:
// not on the grid, the slab, the mask, the row order's other rows or the engine's arithmetic mode beyond mu and scale.
// The engine's momentum, tree and initialisation streams (ids 0-3) are never touched.
//
// One workgroup of ONE wavefront per work item, items taken grid-stride, as predict_kernel (wn_predict.h):
//   matrix   item = (position t, tile): lane k stores y_rep of row n0 + k to out[t][n0 + k]; the stream is that of
//            chain t, draw 0 (wn_engine_replicate);
//   chains   item = (chain c, tile): every draw is read straight from the wn_chains block and y_rep goes to
//            gen[chain c][draw i][n0 + k] of a [k chains][max_len][N] block that becomes a wn_chains of its own with the
//            source lengths -- a predictive interval of an OBSERVATION is wn_summary_quantiles of it
//            (wn_engine_replicate_chains);
//   check    item = (chain c, draw i): the wavefront loads theta ONCE and walks the block's tiles in ascending order; lane
//            k accumulates its rows n0 + k in registers; after the last tile one wave reduction per statistic is stored
//            per draw (wn_engine_replicate_check).  No workspace, and no [draws][N] matrix at any time.
// Rows a mask switches off are not evaluated (a tile that is all off is skipped) and enter no statistic.
//
// THE CHECK.  Six statistics per draw over the live rows, for q = y (the engine's observations) and q = y_rep, with
// (mu, v) the row's predict() values under the draw; weights are never applied:
//   0 sum q    1 sum q^2    2 min q    3 max q    4 #{q == 0}    5 sum (q - mu)^2 / v   (the Pearson discrepancy)
// within lane k, tile by tile:  a0 = a0 + q;  a1 = a1 + q * q;  a2 = q < a2 ? q : a2;  a3 = q > a3 ? q : a3;
//   a4 = a4 + (q == 0 ? 1 : 0);  d = q - mu;  a5 = a5 + (d * d) / v     (start 0, 0, +inf, -inf, 0, 0; products rounded
//   in either arithmetic mode: -ffp-contract=off);
// across the lanes: the sums by the wave_sum butterfly (offsets 32, 1, 2, 4, 8, 16: wave_sum_packed, the replicate's
// total and the observations' in one pass), min and max by the same butterfly.  A draw with a non-finite live replicate
// has NaN in all six replicate statistics; with no live row the sums are 0, min = +inf, max = -inf.  Entries beyond a
// chain's length are NaN.  The CPU emulation runs this source with the same wavefront primitives: same bits.
//
// REGISTERS (gfx950, the widest instantiation: 16 elements per lane, negative binomial; 512 VGPRs available to a lone
// wavefront): DESIGN.md section 3.8.7 holds the table.
//
// The kernels take a parameter struct of their own (ReplicateParams embeds the engine's wn::Observations); wn::Params and
// wn::Observations are untouched.
#pragma once

#include "wn_devrand.h"
#include "wn_predict.h"

namespace wn {

template <class M, class = void>
struct is_replicate : std::false_type {};
template <class M>
struct is_replicate<M, std::enable_if_t<M::kReplicate>> : std::true_type {};

constexpr int kReplicateMatrix = 0, kReplicateChains = 1, kReplicateCheck = 2;
constexpr int kReplicateStats = 6;

struct ReplicateParams {
  Observations obs;  // the engine's observation block (all datasets / the shared rows)
  int32_t dim, mode;
  // the block of rows this launch evaluates: data rows [row0, row0 + num_rows) of obs
  int64_t row0;
  int32_t num_rows, num_tiles;
  int64_t num_items;  // matrix: positions * num_tiles; chains: chains * num_tiles; check: chains * max_len
  uint64_t seed;
  // matrix: theta [T][dim] (unpadded rows), out [T][num_rows]
  const double* theta;
  double* out;
  // chains and check: the chains block (chain c's draw i at draws + chain_off[c] + i * dim), chains [chain0, chain0 +
  // slab_chains) of it
  const double* draws;
  const long long* chain_off;
  const int* chain_len;
  int32_t chain0, slab_chains;
  // chains: gen [slab_chains][max_len][num_rows]; check: max_len of the statistics' arrays
  int32_t max_len;
  double* gen;
  // check: mask [num_rows] of this block (null: every row); stat_rep, stat_obs [6][total_chains][max_len]
  const uint8_t* mask;
  int32_t total_chains;
  double* stat_rep;
  double* stat_obs;
};

// one row of the check's within-lane fold (header comment)
__device__ __forceinline__ void replicate_fold(double q, double mu, double v, bool live, double (&a)[kReplicateStats]) {
  const double d = q - mu;
  a[0] = live ? a[0] + q : a[0];
  a[1] = live ? a[1] + q * q : a[1];
  a[2] = (live && q < a[2]) ? q : a[2];
  a[3] = (live && q > a[3]) ? q : a[3];
  a[4] = live ? a[4] + (q == 0.0 ? 1.0 : 0.0) : a[4];
  a[5] = live ? a[5] + (d * d) / v : a[5];
}
// min (lower) or max over the 64 lanes, in every lane
template <bool lower>
__device__ __forceinline__ double wave_extreme(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = (lower ? o < v : o > v) ? o : v;
  }
  return v;
}

template <class Model, int EPL, bool FMA>
__global__ __launch_bounds__(64) void replicate_kernel(const ReplicateParams Q) {
  static_assert(is_replicate<Model>::value, "the model declares no replicate hook");
  using Cx = PointwiseCx<Model, EPL, FMA, ReplicateParams>;
  Cx cx(Q);
  const int me = cx.tid;
  const WaveAny any;
  for (long long item = blockIdx.x; item < Q.num_items; item += gridDim.x) {
    double th[EPL];
    double eta, mu, v, yrep;
    if (Q.mode == kReplicateCheck) {
      const int who = static_cast<int>(item / Q.max_len);  // chain of the slab
      const int i = static_cast<int>(item - static_cast<long long>(who) * Q.max_len);
      const int chain = Q.chain0 + who;
      const long long plane = static_cast<long long>(Q.total_chains) * Q.max_len;
      const long long at = static_cast<long long>(chain) * Q.max_len + i;
      const double nan = __builtin_nan("");
      if (i >= Q.chain_len[chain]) {  // (wave-uniform) beyond the chain's length
        if (me == 0) {
#pragma unroll
          for (int s = 0; s < kReplicateStats; ++s) {
            Q.stat_rep[s * plane + at] = nan;
            Q.stat_obs[s * plane + at] = nan;
          }
        }
        continue;
      }
      cx.load_theta(Q.draws + Q.chain_off[chain] + static_cast<long long>(i) * Q.dim, th);
      const double inf = __builtin_inf();
      double rep[kReplicateStats] = {0.0, 0.0, inf, -inf, 0.0, 0.0};
      double obs[kReplicateStats] = {0.0, 0.0, inf, -inf, 0.0, 0.0};
      bool bad = false;
      for (int tile = 0; tile < Q.num_tiles; ++tile) {
        const int n0 = tile * kPointwiseTile;
        const bool row = n0 + me < Q.num_rows;
        const bool live = row && (Q.mask == nullptr || Q.mask[row ? n0 + me : 0] != 0);
        if (!any(live)) continue;
        RepStream rng{Q.seed, static_cast<uint32_t>(n0 + me), static_cast<uint32_t>(i), static_cast<uint32_t>(chain), 0u};
        Model::template replicate<EPL>(cx, th, n0, live, rng, eta, mu, v, yrep);
        const double y = live ? cx.obs_y(n0 + me) : 0.0;
        replicate_fold(yrep, mu, v, live, rep);
        replicate_fold(y, mu, v, live, obs);
        bad = bad || (live && !(__builtin_fabs(yrep) < inf));
      }
      const bool spoilt = any(bad);
      double out_rep[kReplicateStats], out_obs[kReplicateStats];
#pragma unroll
      for (int s = 0; s < kReplicateStats; ++s) {
        if (s == 2 || s == 3) continue;
        const double packed = wave_sum_packed(rep[s], obs[s]);
        out_rep[s] = uni(packed);
        out_obs[s] = lane_value(packed, 32);
      }
      out_rep[2] = wave_extreme<true>(rep[2]);
      out_obs[2] = wave_extreme<true>(obs[2]);
      out_rep[3] = wave_extreme<false>(rep[3]);
      out_obs[3] = wave_extreme<false>(obs[3]);
      if (me == 0) {
#pragma unroll
        for (int s = 0; s < kReplicateStats; ++s) {
          Q.stat_rep[s * plane + at] = spoilt ? nan : out_rep[s];
          Q.stat_obs[s * plane + at] = out_obs[s];
        }
      }
      continue;
    }
    const int who = static_cast<int>(item / Q.num_tiles);  // position t, or chain of the slab
    const int tile = static_cast<int>(item - static_cast<long long>(who) * Q.num_tiles);
    const int n0 = tile * kPointwiseTile;
    const bool live = n0 + me < Q.num_rows;
    if (Q.mode == kReplicateMatrix) {
      cx.load_theta(Q.theta + static_cast<long long>(who) * Q.dim, th);
      RepStream rng{Q.seed, static_cast<uint32_t>(n0 + me), 0u, static_cast<uint32_t>(who), 0u};
      Model::template replicate<EPL>(cx, th, n0, live, rng, eta, mu, v, yrep);
      if (live) Q.out[static_cast<long long>(who) * Q.num_rows + n0 + me] = yrep;
      continue;
    }
    const int chain = Q.chain0 + who;
    const int len = Q.chain_len[chain];
    const double* draw = Q.draws + Q.chain_off[chain];
    double* out = Q.gen + static_cast<long long>(who) * Q.max_len * Q.num_rows + n0 + me;
    for (int i = 0; i < len; ++i) {
      cx.load_theta(draw + static_cast<long long>(i) * Q.dim, th);
      RepStream rng{Q.seed, static_cast<uint32_t>(n0 + me), static_cast<uint32_t>(i), static_cast<uint32_t>(chain), 0u};
      Model::template replicate<EPL>(cx, th, n0, live, rng, eta, mu, v, yrep);
      if (live) out[static_cast<long long>(i) * Q.num_rows] = yrep;
    }
  }
}

}  // namespace wn
