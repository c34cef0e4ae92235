// wn_predict.h -- PREDICTIONS of a data model on the device: for a draw theta and a row n the triple
//   eta = the linear predictor, formed exactly as pointwise() forms it (pointwise_eta, the group effect, the offset),
//   mu  = E[y | theta, x_n],   v = Var[y | theta, x_n]
// (wn_model_api.h, kPredict: Model::predict() leaves the triple of row n0 + k of a tile of 64 rows in lane k; the link is
// evaluated ONCE on the full wavefront: Link::response / Family::response beside term()).  x, group and offset are
// read; y and the weights never are, so a logistic row with binomial weights is predicted per trial.
//
//   family                     mu                                      v
//   identity (unit noise)      eta                                     1
//   linear_regression_sigma    eta                                     scale * scale,  scale = dexp(s)
//   hier_linear_regression_sigma*   eta (with the group effect)        scale * scale,  scale = dexp(s), s the LAST coordinate
//   hier_linear_regression_slopes_sigma   eta (with the group terms)   scale * scale,  scale = dexp(s), s the LAST coordinate
//   logit                      eta >= 0 ? d : e * d                    (e * d) * d      e = dexp(-|eta|), d = 1 / (1 + e)
//   log (Poisson)              dexp(eta)                               mu
//   negative binomial          dexp(eta)                               Cx::mad(kappa * mu, mu, mu),  kappa = dexp(s)
// (the logit mu is the value LogitLink::term computes for its residual; v is per trial and has no mu (1 - mu)
// cancellation; scale / kappa come from the wave-uniform s once per draw and tile, as in pointwise()).  Non-finite values
// follow IEEE: an overflowing Poisson link gives inf.
//
// One workgroup of ONE wavefront per work item, items taken grid-stride (any grid gives the same bits: an item's result
// depends on nothing but the item).  Three modes consume the triple, which comes from the SAME expression in all of
// them, so the matrix, the generated chains and the fold's inputs are the same bits:
//   matrix   item = (position t, tile): lane k stores the selected outputs of row n0 + k to [T][N] planes
//            (wn_engine_predict);
//   chains   item = (chain c, tile): every draw is read straight from the wn_chains block, and ONE selected quantity
//            (eta or mu) is stored to out[chain c][draw i][n0 + k] of a [k chains][max_len][N] block that becomes a
//            wn_chains of its own -- quantiles, R-hat, ESS and MCSE of a prediction are the wn_summary_* functions'
//            (wn_engine_predict_chains);
//   fold     item = (chain c, tile), draws in order: lane k keeps FIVE accumulator registers for row n0 + k -- Welford
//            (mean, M2) of eta, Welford (mean, M2) of mu, a running mean of v; the chain's partial goes to a workspace
//            laid out [5][slab chains][rows].  predict_combine_kernel (one thread per row) merges the partials of a
//            block's chains IN CHAIN ORDER into a running state carried from slab to slab and, after the last chain,
//            writes the outputs (wn_engine_predict_fold).
// Rows a mask switches off are not evaluated: a pair of rows that is off issues no load, a tile that is all off folds
// nothing; such a row returns NaN everywhere and count = 0.
//
// THE FOLD (draws ordered by chain, then by iteration; arithmetic independent of the engine's arithmetic mode: rounded
// products, -ffp-contract=off):
//   within a chain, for draw number n = 1, 2, ... and q in {eta, mu}:
//     d = q - mean;  mean = mean + d / n;  M2 = M2 + d * (q - mean);      vbar = vbar + (v - vbar) / n
//   across chains, chain by chain (the first chain's partial is taken as it is):
//     nn = n_a + n_b;  d = mean_b - mean_a;  mean = mean_a + d * (n_b / nn);
//     M2 = (M2_a + M2_b) + (d * d) * (n_a * n_b / nn);                    vbar = vbar_a + (vbar_b - vbar_a) * (n_b / nn)
//   at the end: the variances are M2 / (n - 1), NaN with fewer than 2 draws; noise_var = vbar; count = n.
// The CPU emulation runs this source with the same wavefront primitives, so device and emulation agree bit for bit.
//
// The kernels take a parameter struct of their own (PredictParams embeds the engine's wn::Observations); wn::Params and
// wn::Observations are untouched.
#pragma once

#include "wn_pointwise.h"

namespace wn {

template <class M, class = void>
struct is_predict : std::false_type {};
template <class M>
struct is_predict<M, std::enable_if_t<M::kPredict>> : std::true_type {};

constexpr int kPredictMatrix = 0, kPredictChains = 1, kPredictFold = 2;
constexpr int kPredictAccumulators = 5;  // eta: mean, M2; mu: mean, M2; v: mean

struct PredictParams {
  Observations obs;  // the engine's observation block (all datasets / the shared rows)
  int32_t dim, mode;
  // the block of rows this launch evaluates: data rows [row0, row0 + num_rows) of obs
  int64_t row0;
  int32_t num_rows, num_tiles;
  int64_t num_items;  // positions (or chains) * num_tiles
  // matrix: theta [T][dim] (unpadded rows); each output [T][num_rows], null: not wanted
  const double* theta;
  double* eta_out;
  double* mu_out;
  double* v_out;
  // chains and fold: the chains block (chain c's draw i at draws + chain_off[c] + i * dim), chains [chain0, chain0 +
  // slab_chains) of it
  const double* draws;
  const long long* chain_off;
  const int* chain_len;
  int32_t chain0, slab_chains;
  // chains: gen [slab_chains][max_len][num_rows] receives eta (what == 0) or mu (what == 1)
  int32_t what, max_len;
  double* gen;
  // fold: mask [num_rows] of this block (null: every row); partial [5][slab_chains][num_rows]
  const uint8_t* mask;
  double* partial;
};

// One draw of the within-chain fold (header comment): lane k's accumulators for its row.
__device__ __forceinline__ void predict_fold(double eta, double mu, double v, double n, double (&a)[kPredictAccumulators]) {
  const double de = eta - a[0];
  a[0] = a[0] + de / n;
  a[1] = a[1] + de * (eta - a[0]);
  const double dm = mu - a[2];
  a[2] = a[2] + dm / n;
  a[3] = a[3] + dm * (mu - a[2]);
  a[4] = a[4] + (v - a[4]) / n;
}

template <class Model, int EPL, bool FMA>
__global__ __launch_bounds__(64) void predict_kernel(const PredictParams Q) {
  static_assert(is_predict<Model>::value, "the model declares no predict hook");
  using Cx = PointwiseCx<Model, EPL, FMA, PredictParams>;
  Cx cx(Q);
  const int me = cx.tid;
  for (long long item = blockIdx.x; item < Q.num_items; item += gridDim.x) {
    const int who = static_cast<int>(item / Q.num_tiles);  // position t, or chain of the slab
    const int tile = static_cast<int>(item - static_cast<long long>(who) * Q.num_tiles);
    const int n0 = tile * kPointwiseTile;
    const bool row = n0 + me < Q.num_rows;
    const bool live = row && (Q.mask == nullptr || Q.mask[row ? n0 + me : 0] != 0);
    double th[EPL];
    double eta, mu, v;
    if (Q.mode == kPredictMatrix) {
      cx.load_theta(Q.theta + static_cast<long long>(who) * Q.dim, th);
      Model::template predict<EPL>(cx, th, n0, live, eta, mu, v);
      if (live) {
        const long long at = static_cast<long long>(who) * Q.num_rows + n0 + me;
        if (Q.eta_out != nullptr) Q.eta_out[at] = eta;
        if (Q.mu_out != nullptr) Q.mu_out[at] = mu;
        if (Q.v_out != nullptr) Q.v_out[at] = v;
      }
      continue;
    }
    const int chain = Q.chain0 + who;
    const int len = Q.chain_len[chain];
    const double* draw = Q.draws + Q.chain_off[chain];
    if (Q.mode == kPredictChains) {
      double* out = Q.gen + static_cast<long long>(who) * Q.max_len * Q.num_rows + n0 + me;
      for (int i = 0; i < len; ++i) {
        cx.load_theta(draw + static_cast<long long>(i) * Q.dim, th);
        Model::template predict<EPL>(cx, th, n0, live, eta, mu, v);
        if (live) out[static_cast<long long>(i) * Q.num_rows] = Q.what == 0 ? eta : mu;
      }
      continue;
    }
    double acc[kPredictAccumulators] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // (a tile without a live row folds nothing: its partial is never read)
    int any = 0;
    for (int k = 0; k < kPointwiseTile; ++k) any |= lane_value(live ? 1 : 0, k);
    if (any) {
      for (int i = 0; i < len; ++i) {
        cx.load_theta(draw + static_cast<long long>(i) * Q.dim, th);
        Model::template predict<EPL>(cx, th, n0, live, eta, mu, v);
        predict_fold(eta, mu, v, static_cast<double>(i + 1), acc);
      }
    }
    if (live) {
      const long long plane = static_cast<long long>(Q.slab_chains) * Q.num_rows;
      double* p = Q.partial + static_cast<long long>(who) * Q.num_rows + n0 + me;
#pragma unroll
      for (int a = 0; a < kPredictAccumulators; ++a) p[a * plane] = acc[a];
    }
  }
}

// The across-chain merge and the final values (header comment).  One thread per row of the block; `state` [6][num_rows]
// (n and the five accumulators) carries the fold from one slab of chains to the next, so the size of the workspace
// changes nothing.
struct PredictCombineParams {
  const double* partial;  // [5][slab_chains][num_rows]
  const int* chain_len;   // of the whole chains block
  int32_t chain0, slab_chains, num_rows;
  int32_t first, last;    // this slab holds the block's first / last chain
  const uint8_t* mask;    // [num_rows] (null: every row)
  double* state;          // [6][num_rows]
  double* eta_mean;       // [num_rows] of this block, each
  double* eta_var;
  double* mean;
  double* mean_var;
  double* noise_var;
  long long* count;
};

template <int kBlock>
__global__ __launch_bounds__(kBlock) void predict_combine_kernel(const PredictCombineParams Q) {
  constexpr int A = kPredictAccumulators;
  const double nan = __builtin_nan("");
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < Q.num_rows;
       r += static_cast<long long>(gridDim.x) * kBlock) {
    if (Q.mask != nullptr && Q.mask[r] == 0) {
      if (Q.last) {
        Q.eta_mean[r] = nan;
        Q.eta_var[r] = nan;
        Q.mean[r] = nan;
        Q.mean_var[r] = nan;
        Q.noise_var[r] = nan;
        Q.count[r] = 0;
      }
      continue;
    }
    const long long N = Q.num_rows, plane = static_cast<long long>(Q.slab_chains) * N;
    double n = 0.0;
    double a[A] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (!Q.first) {
      n = Q.state[r];
#pragma unroll
      for (int k = 0; k < A; ++k) a[k] = Q.state[(k + 1) * N + r];
    }
    for (int c = 0; c < Q.slab_chains; ++c) {
      const double* p = Q.partial + static_cast<long long>(c) * N + r;
      const double nb = static_cast<double>(Q.chain_len[Q.chain0 + c]);
      double b[A];
#pragma unroll
      for (int k = 0; k < A; ++k) b[k] = p[k * plane];
      if (Q.first && c == 0) {
        n = nb;
#pragma unroll
        for (int k = 0; k < A; ++k) a[k] = b[k];
        continue;
      }
      const double nn = n + nb;
      const double w = nb / nn, cross = n * nb / nn;
#pragma unroll
      for (int k = 0; k < 4; k += 2) {
        const double d = b[k] - a[k];
        a[k] = a[k] + d * w;
        a[k + 1] = (a[k + 1] + b[k + 1]) + (d * d) * cross;
      }
      a[4] = a[4] + (b[4] - a[4]) * w;
      n = nn;
    }
    if (!Q.last) {
      Q.state[r] = n;
#pragma unroll
      for (int k = 0; k < A; ++k) Q.state[(k + 1) * N + r] = a[k];
      continue;
    }
    Q.eta_mean[r] = a[0];
    Q.eta_var[r] = n >= 2.0 ? a[1] / (n - 1.0) : nan;
    Q.mean[r] = a[2];
    Q.mean_var[r] = n >= 2.0 ? a[3] / (n - 1.0) : nan;
    Q.noise_var[r] = a[4];
    Q.count[r] = static_cast<long long>(n);
  }
}

}  // namespace wn
