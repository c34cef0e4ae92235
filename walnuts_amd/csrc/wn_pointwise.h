// wn_pointwise.h -- the POINTWISE log-likelihood of a data model on the device: l_n(theta), the full log density of
// observation row n under one draw (constants included, weights never applied), and what is folded from it over the
// draws of a wn_chains block -- the log pointwise predictive density and the moments WAIC reads.
//
//   log_lik      theta [T][D] at positions the caller chose           -> l [T][N]            (wn_engine_log_lik)
//   predictive   a wn_chains block [C][max_len][D], lengths respected -> per row n: lpd_n = log mean_t exp l_n(theta_t),
//                mean_n and var_n of l_n(theta_t) over the draws, their count            (wn_engine_log_predictive)
//   matrix       the same block -> l [N][ld], a row's draws in one contiguous column, in a device workspace
//                (stage 1 of wn_engine_psis_loo: wn_psis.h)
//
// The row term is the model's own (wn_model_api.h, kPointwise): Model::pointwise() streams a TILE of 64 consecutive rows,
// forms eta in the order models/glm.h states (slot-order Cx::mad dot product, wave_sum_packed butterfly, group effect,
// offset), leaves eta of row n0 + k in lane k and evaluates the link ONCE on the full wavefront, Link::term with a zero
// running sum -- the expression the weighted path of eval() uses, so the bits of eta and of the term are eval()'s.  There
// is no gradient pass and no block of rows held in registers.  The kernel then adds the row's constant c_n(y_n)
// (-1/2 log 2 pi, -lgamma(y + 1), 0: Model::pointwise_const, computed on the host in long double and rounded once,
// a device array beside y) as the LAST operation.
//
// One workgroup of ONE wavefront per work item, items taken grid-stride (any grid gives the same bits: an item's result
// depends on nothing but the item):
//   log_lik:     item = (position t, tile): the tile's 64 terms are stored, lane k -> l[t][n0 + k].
//   predictive:  item = (chain c, tile): for each draw of the chain, in order, theta is read straight from the chains
//                block (never a [draws][N] matrix), the tile is streamed, and lane k updates FOUR accumulator registers
//                for row n0 + k; the chain's partial (m, s, mean, M2) goes to a workspace laid out [4][chains][rows].
//                pointwise_combine_kernel (one thread per row) then merges the partials of a block's chains IN CHAIN
//                ORDER into a running state and, after the last chain, writes lpd, mean, var and count.
//   matrix:      item = (chain c, tile), the predictive walk without the fold: the term of the chain's draw i is stored,
//                lane k -> l[n0 + k][draw0[c] + i], draw0[c] the draws of the block's chains before c.
// Rows a mask switches off are not evaluated: a pair of rows that is off issues no load, a tile that is all off no draw.
//
// THE FOLD (draws ordered by chain, then by iteration; arithmetic independent of the engine's arithmetic mode:
// rounded products, -ffp-contract=off):
//   within a chain, draw by draw, with l = l_n(theta):
//     log-sum-exp   running max m (start -inf) and rescaled sum s (start 0):
//                     e = exp(-|l - m|) (1 when l == m);  l > m: s = s * e + 1, m = l;  otherwise s = s + e
//                     l == -inf: nothing changes (the term contributes 0 to s);  l NaN: s = NaN (it stays NaN)
//     moments       the project's Welford form (wn_traj.h, lp_stats): n = n + 1, d = l - mean, mean = mean + d / n,
//                     M2 = M2 + d * (l - mean)
//   across chains, chain by chain (the first chain's partial is taken as it is):
//     log-sum-exp   M = max(m_a, m_b), s = s_a * f_a + s_b * f_b, f_x = 1 when m_x == M, 0 when m_x == -inf, else
//                     exp(m_x - M)
//     moments       n = n_a + n_b, d = mean_b - mean_a, mean = mean_a + d * (n_b / n),
//                     M2 = (M2_a + M2_b) + (d * d) * (n_a * n_b / n)
//   at the end      lpd = (m + log s) - log n, and -inf when s == 0 (every term -inf);  var = M2 / (n - 1), NaN with
//                     fewer than 2 draws;  a masked row: lpd = mean = var = NaN, count = 0.  NaN propagates everywhere.
// exp / log are wnd::dexp / wnd::dlog; the CPU emulation runs this source with the same wavefront primitives, so device
// and emulation agree bit for bit.
//
// The kernels take a parameter struct of their own (PointwiseParams embeds the engine's wn::Observations); wn::Params and
// wn::Observations are untouched.
#pragma once

#include <type_traits>

#include "wn_traj.h"

namespace wn {

template <class M, class = void>
struct is_pointwise : std::false_type {};
template <class M>
struct is_pointwise<M, std::enable_if_t<M::kPointwise>> : std::true_type {};

constexpr int kPointwiseTile = 64;      // rows per tile: one per lane
constexpr int kPointwiseCombineBlock = 64;

struct PointwiseParams {
  Observations obs;         // the engine's observation block (all datasets / the shared rows)
  const double* row_const;  // [rows of the block]: c_n(y_n), beside y
  int32_t dim, predictive;  // predictive: 0 log_lik, 1 (kPointwiseFold) the fold, 2 (kPointwiseMatrix) the matrix
  // the block of rows this launch evaluates: data rows [row0, row0 + num_rows) of obs
  int64_t row0;
  int32_t num_rows, num_tiles;
  int64_t num_items;  // positions (or chains) * num_tiles
  // log_lik: theta [T][dim] (unpadded rows), out [T][num_rows]
  const double* theta;
  double* out;
  // predictive: the chains block (chain c's draw i at draws + chain_off[c] + i * dim), chains [chain0, chain0 + ...) of
  // it; mask [num_rows] of this block (null: every row); partial [4][slab_chains][num_rows]
  const double* draws;
  const long long* chain_off;
  const int* chain_len;
  int32_t chain0, slab_chains;
  const uint8_t* mask;
  double* partial;
  // matrix: out [num_rows][ld]; draw0 [chains of the chains block]: the column of chain c's first draw
  const long long* draw0;
  int64_t ld;
};
constexpr int kPointwiseFold = 1, kPointwiseMatrix = 2;

// What Model::pointwise sees as `cx`: the data-model calls of wn_model_api.h over ONE block of rows (row indices are
// relative to the block), one wavefront.  P: the kernel's parameter struct -- obs, dim, row0, num_rows are read
// (wn_predict.h hands its own).
template <class Model, int EPL, bool FMA, class P = PointwiseParams>
struct PointwiseCx {
  static constexpr int L = 64;
  static constexpr int NP = EPL / 2;
  const P& Q;
  int tid;
  LaneTables tabs;
  const double* obs_xv;
  const double* obs_yv;
  const int32_t* obs_gv;
  const double* obs_ov;
  int x_stride;

  __device__ __forceinline__ explicit PointwiseCx(const P& q) : Q(q) {
    tid = opaque_lane_id();
    tabs.load(tid);
    x_stride = uses_groups<Model>::value ? Q.obs.stride : L * EPL;
    obs_xv = Q.obs.x + Q.row0 * x_stride;
    obs_yv = Q.obs.y + Q.row0;
    obs_gv = Q.obs.group != nullptr ? Q.obs.group + Q.row0 : nullptr;
    obs_ov = Q.obs.offset != nullptr ? Q.obs.offset + Q.row0 : nullptr;
  }
  __device__ __forceinline__ static double mad(double a, double b, double c) {
    if constexpr (FMA) return __builtin_fma(a, b, c);
    return a * b + c;
  }
  __device__ __forceinline__ int index(int j) const { return ((j >> 1) * L + tid) * 2 + (j & 1); }
  __device__ __forceinline__ bool valid(int j) const { return index(j) < Q.dim; }
  __device__ __forceinline__ int dim() const { return Q.dim; }
  __device__ __forceinline__ UniformTab uniform_tab() const { return UniformTab{tabs}; }
  __device__ __forceinline__ GatherTab gather_tab() const { return GatherTab{tabs}; }
  __device__ __forceinline__ int num_obs() const { return Q.num_rows; }
  // the lane's slots of row n (0 <= n < num_rows, wave-uniform): 16-byte pair loads, as TrajChip::load_row
  __device__ __forceinline__ void load_row(int n, double (&x)[EPL]) const {
    const int nx = x_stride / (2 * L);  // slot pairs the row holds (a grouped model's rows are narrower than theta)
    const v2f64* row = reinterpret_cast<const v2f64*>(obs_xv + static_cast<long long>(n) * x_stride) + tid;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      if (k < nx) {
        const v2f64 t = row[k * L];
        x[2 * k] = t[0];
        x[2 * k + 1] = t[1];
      } else {
        x[2 * k] = 0.0;
        x[2 * k + 1] = 0.0;
      }
    }
  }
  __device__ __forceinline__ double obs_y(int n) const { return obs_yv[n]; }
  __device__ __forceinline__ int num_groups() const { return Q.obs.num_groups; }
  __device__ __forceinline__ int obs_group(int n) const { return obs_gv[n]; }
  // varying slopes (kVaryingSlopes): Q, and column `col` of row n of x, a per-lane load (as TrajChip::obs_x)
  __device__ __forceinline__ int num_varying() const { return Q.obs.num_varying; }
  __device__ __forceinline__ double obs_x(int n, int col) const { return obs_xv[static_cast<long long>(n) * x_stride + col]; }
  __device__ __forceinline__ bool has_offset() const { return obs_ov != nullptr; }
  __device__ __forceinline__ bool has_weight() const { return false; }  // weights are never applied
  __device__ __forceinline__ double obs_offset(int n) const { return obs_ov[n]; }
  __device__ __forceinline__ double obs_weight(int) const { return 1.0; }
  // one draw, laid out like theta: slot j holds coordinate index(j) of an UNPADDED row of dim doubles, 0 beyond
  __device__ __forceinline__ void load_theta(const double* row, double (&th)[EPL]) const {
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      const int c = index(j);
      th[j] = c < Q.dim ? row[c] : 0.0;
    }
  }
};

// One draw of the within-chain fold (header comment): lane k's accumulators for its row.
template <class Tab>
__device__ __forceinline__ void pointwise_fold(double l, double n, double& m, double& s, double& mean, double& m2,
                                               const Tab& tab) {
  const double inf = __builtin_inf();
  const bool up = l > m;
  const double d = l == m ? 0.0 : -__builtin_fabs(l - m);
  const double e = wnd::dexp(d, tab);
  double s_new = up ? s * e + 1.0 : s + e;
  double m_new = up ? l : m;
  if (l == -inf) {
    s_new = s;
    m_new = m;
  }
  if (l != l) s_new = l;
  s = s_new;
  m = m_new;
  const double delta = l - mean;
  mean = mean + delta / n;
  m2 = m2 + delta * (l - mean);
}

template <class Model, int EPL, bool FMA>
__global__ __launch_bounds__(64) void pointwise_kernel(const PointwiseParams Q) {
  static_assert(is_pointwise<Model>::value, "the model declares no pointwise hook");
  using Cx = PointwiseCx<Model, EPL, FMA>;
  Cx cx(Q);
  const int me = cx.tid;
  for (long long item = blockIdx.x; item < Q.num_items; item += gridDim.x) {
    const int who = static_cast<int>(item / Q.num_tiles);  // position t, or chain of the slab
    const int tile = static_cast<int>(item - static_cast<long long>(who) * Q.num_tiles);
    const int n0 = tile * kPointwiseTile;
    const bool row = n0 + me < Q.num_rows;
    const bool live = row && (Q.mask == nullptr || Q.mask[row ? n0 + me : 0] != 0);
    const double c = live ? Q.row_const[Q.row0 + n0 + me] : 0.0;
    double th[EPL];
    if (!Q.predictive) {
      cx.load_theta(Q.theta + static_cast<long long>(who) * Q.dim, th);
      const double l = Model::template pointwise<EPL>(cx, th, n0, live) + c;
      if (live) Q.out[static_cast<long long>(who) * Q.num_rows + n0 + me] = l;
      continue;
    }
    const int chain = Q.chain0 + who;
    const int len = Q.chain_len[chain];
    const double* draw = Q.draws + Q.chain_off[chain];
    double m = -__builtin_inf(), s = 0.0, mean = 0.0, m2 = 0.0;
    // (a tile without a live row folds nothing: its partial is never read)
    int any = 0;
    for (int k = 0; k < kPointwiseTile; ++k) any |= lane_value(live ? 1 : 0, k);
    if (Q.predictive == kPointwiseMatrix) {
      double* column = Q.out + (row ? n0 + me : 0) * Q.ld + Q.draw0[chain];
      for (int i = 0; any && i < len; ++i) {
        cx.load_theta(draw + static_cast<long long>(i) * Q.dim, th);
        const double l = Model::template pointwise<EPL>(cx, th, n0, live) + c;
        if (live) column[i] = l;
      }
      continue;
    }
    if (any) {
      for (int i = 0; i < len; ++i) {
        cx.load_theta(draw + static_cast<long long>(i) * Q.dim, th);
        const double l = Model::template pointwise<EPL>(cx, th, n0, live) + c;
        pointwise_fold(l, static_cast<double>(i + 1), m, s, mean, m2, cx.gather_tab());
      }
    }
    if (live) {
      const long long plane = static_cast<long long>(Q.slab_chains) * Q.num_rows;
      double* p = Q.partial + static_cast<long long>(who) * Q.num_rows + n0 + me;
      p[0] = m;
      p[plane] = s;
      p[2 * plane] = mean;
      p[3 * plane] = m2;
    }
  }
}

// The across-chain merge and the final values (header comment).  One thread per row of the block; `state` [5][num_rows]
// (n, m, s, mean, M2) carries the fold from one slab of chains to the next, so the size of the workspace changes nothing.
struct PointwiseCombineParams {
  const double* partial;  // [4][slab_chains][num_rows]
  const int* chain_len;   // of the whole chains block
  int32_t chain0, slab_chains, num_rows;
  int32_t first, last;    // this slab holds the block's first / last chain
  const uint8_t* mask;    // [num_rows] (null: every row)
  double* state;          // [5][num_rows]
  double* lpd;            // [num_rows] of this block
  double* mean;
  double* var;
  long long* count;
};

template <int kBlock>
__global__ __launch_bounds__(kBlock) void pointwise_combine_kernel(const PointwiseCombineParams Q) {
  const wnd::ArrayTables tab = wnd::array_tables();
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  for (long long r = blockIdx.x * static_cast<long long>(kBlock) + threadIdx.x; r < Q.num_rows;
       r += static_cast<long long>(gridDim.x) * kBlock) {
    if (Q.mask != nullptr && Q.mask[r] == 0) {
      if (Q.last) {
        Q.lpd[r] = nan;
        Q.mean[r] = nan;
        Q.var[r] = nan;
        Q.count[r] = 0;
      }
      continue;
    }
    const long long N = Q.num_rows, plane = static_cast<long long>(Q.slab_chains) * N;
    double n = 0.0, m = 0.0, s = 0.0, mean = 0.0, m2 = 0.0;
    if (!Q.first) {
      n = Q.state[r];
      m = Q.state[N + r];
      s = Q.state[2 * N + r];
      mean = Q.state[3 * N + r];
      m2 = Q.state[4 * N + r];
    }
    for (int c = 0; c < Q.slab_chains; ++c) {
      const double* p = Q.partial + static_cast<long long>(c) * N + r;
      const double nb = static_cast<double>(Q.chain_len[Q.chain0 + c]);
      const double mb = p[0], sb = p[plane], meanb = p[2 * plane], m2b = p[3 * plane];
      if (Q.first && c == 0) {
        n = nb;
        m = mb;
        s = sb;
        mean = meanb;
        m2 = m2b;
        continue;
      }
      const double big = mb > m ? mb : m;
      const double fa = m == big ? 1.0 : (m == -inf ? 0.0 : wnd::dexp(m - big, tab));
      const double fb = mb == big ? 1.0 : (mb == -inf ? 0.0 : wnd::dexp(mb - big, tab));
      s = s * fa + sb * fb;
      m = big;
      const double nn = n + nb;
      const double d = meanb - mean;
      mean = mean + d * (nb / nn);
      m2 = (m2 + m2b) + (d * d) * (n * nb / nn);
      n = nn;
    }
    if (!Q.last) {
      Q.state[r] = n;
      Q.state[N + r] = m;
      Q.state[2 * N + r] = s;
      Q.state[3 * N + r] = mean;
      Q.state[4 * N + r] = m2;
      continue;
    }
    Q.lpd[r] = s == 0.0 ? -inf : (m + wnd::dlog(s, tab)) - wnd::dlog(n, tab);
    Q.mean[r] = mean;
    Q.var[r] = n >= 2.0 ? m2 / (n - 1.0) : nan;
    Q.count[r] = static_cast<long long>(n);
  }
}

}  // namespace wn
