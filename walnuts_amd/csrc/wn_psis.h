// wn_psis.h -- leave-one-out cross-validation by Pareto-smoothed importance sampling (PSIS-LOO; Vehtari, Gelman, Gabry
// 2017; Vehtari, Simpson, Gelman, Yao, Gabry 2024) of a data model on the device, from the draws of a wn_chains block:
// per data row n the estimate elpd_loo_n, the Pareto shape khat_n of the row's importance ratios, the effective sample
// size of the smoothed weights and lpd_n.  The [rows][draws] matrix of pointwise terms lives in a device workspace, a
// slab of rows at a time, and never reaches the host.                                          (wn_engine_psis_loo)
//
// STAGE 1, the matrix slab: pointwise_kernel (wn_pointwise.h) in its matrix mode.  Work item = (chain, tile of 64 rows);
// the chain's draws are walked in order and lane k's term l_n(theta) -- the value wn_engine_log_lik gives, bit for bit
// -- is stored at lmat[(n0 + k) * ld + first_draw_of_chain + i]: a row's draws, ordered by chain and then by iteration,
// are one contiguous column of S doubles.
//
// STAGE 2, psis_row_kernel: one workgroup of 256 threads (four wavefronts) per row, rows taken grid-stride; a row's
// result depends on nothing but its column, so any grid and any slab size give the same bits.  With l_s the column:
//   1. shift    r_s = (-l_s) - mx, mx = max_s(-l_s).  A column that holds a non-finite l gives NaN four times.
//   2. tail     M = min(floor(S / 5), ceil(3 sqrt(S))) (host, integers).  The draws are ordered by the summaries' order-
//               preserving 64-bit key of r (wn_summary.hip: order_key).  T = the key at sorted position S - M, found by
//               a radix select, 8 bits a pass, LDS histogram of 256 bins; cutoff = the value at position S - M - 1 (the
//               largest key below T when exactly S - M keys lie below T, else T itself).  The tail is every draw with
//               key > T plus M - #{key > T} copies of the T value; the other ties at T stay below the tail.  No draw
//               index is kept.  r is a non-increasing function of l, so the tail's l are kept (as inverted keys of l,
//               in LDS) and r is formed from them again -- the same subtraction, the same bits.  Draws tied in r have
//               equal l unless the subtraction rounded two neighbours together; the ties' l is then the smallest of
//               theirs.  The tail is sorted by a bitonic network in LDS, padded to a power of two with the largest key.
//   3. fit      when M >= 5: x_i = exp(r_(i)) - exp(cutoff), i = 1..M ascending, and the generalised Pareto fit of
//               Zhang and Stephens (2009) as the R package loo has it: m = 30 + floor(sqrt(M)), xq = x[floor(M/4 + 0.5)],
//               b_j = 1/x_M + (1 - sqrt(m / (j - 0.5))) / (3 xq), k_j = mean_i log1p(-b_j x_i),
//               L_j = M (log(-b_j / k_j) - k_j - 1), w_j = 1 / sum_i exp(L_i - L_j), b = sum_j b_j w_j,
//               k = mean_i log1p(-b x_i), sigma = -k / b, khat = (M k + 5) / (M + 10).
//               M < 5, xq or x_M not positive, or a non-finite khat or sigma: no smoothing, khat = +inf.
//   4. smooth   tail element i: lw = log(sigma * expm1(-khat * log1p(-p_i)) / khat + exp(cutoff)), p_i = (i - 0.5) / M;
//               every other draw: lw = r; then lw = min(lw, 0).
//   5. outputs  elpd_loo = lse(l + lw) - lse(lw), ess = 1 / sum w~^2 of the normalised weights (no autocorrelation
//               correction), lpd = lse(l) - log S, count = S; a masked row: NaN four times, count 0.
//
// ORDERS OF SUMMATION (arithmetic independent of the engine's arithmetic mode: rounded products, -ffp-contract=off;
// exp / log / log1p are wnd::dexp / dlog / dlog1p, expm1 is psis_expm1 below, sqrt and / are IEEE):
//   a BLOCK SUM over an index range: thread t adds its terms t, t + 256, t + 512, ... in that order to a partial that
//   starts at 0; each wavefront adds its 64 partials with the xor butterfly (offsets 32, 1, 2, 4, 8, 16); the four
//   wavefront sums are added as ((w0 + w1) + w2) + w3.
//   k_j, k      block sums over the sorted tail positions i, divided by M.
//   w_j         thread j adds exp(L_i - L_j) for i = 1..m in order;  b = sum_j b_j w_j for j = 1..m in order.
//   the final sums, each with its own exact maximum as the shift (a = max lw, c = max (l + lw), d = max l):
//               A = sum exp(lw - a), Q = sum exp(lw - a)^2, B = sum exp((l + lw) - c), D = sum exp(l - d), each as
//               (block sum over the draws with key < T, in draw order) + (number of ties below the tail) * (the tie's
//               term), then + (block sum over the sorted tail positions);
//               elpd_loo = (c + log B) - (a + log A), ess = (A * A) / Q, lpd = (d + log D) - log S.
// Maxima, minima and counts are exact in any order.  The CPU emulation runs this source with the same wavefront
// primitives, so device and emulation agree bit for bit.
//
// LDS, static: the tail's keys (4 096 x 8 bytes), x_i and then lw_i (4 096 x 8 bytes), the 256-bin histogram, the
// candidates' wavefront sums and a few scalars: about 70 KiB.  Every size is fixed at compile time, nothing depends on the
// launch, and a gfx950 workgroup may declare up to 160 KiB statically, so nothing is gained from a dynamic carve (which
// would also need its base kept 16-byte aligned behind the statics): two workgroups a compute unit, eight wavefronts.
// The bitonic network runs in pair form -- thread p handles elements i = 2 j (p / j) + p % j and i + j, every thread
// busy -- so strides of 32 elements and more read and write consecutive 8-byte words (no bank conflict), and strides
// below 32 leave gaps of j words between runs of j: a 2-way conflict at worst on those log2(32) * (number of merges)
// steps.  A tail beyond 4 096 draws (S > 1 864 135) is refused by the host.
#pragma once

#include "wn_traj.h"

namespace wn {

constexpr int kPsisBlock = 256;
constexpr int kPsisWaves = kPsisBlock / 64;
constexpr int kPsisMaxTail = 4096;
constexpr int kPsisMaxCandidates = 30 + 64;  // m = 30 + floor(sqrt(M)), M <= 4096
constexpr int kPsisMinFit = 5;

struct PsisParams {
  const double* lmat;  // [num_rows][ld]: row n's draws at lmat + n * ld
  int64_t ld;
  int32_t num_rows;    // rows of this slab
  int32_t num_draws;   // S
  int32_t tail, candidates, tail_padded;  // M, m, M rounded up to a power of two
  int32_t quartile;    // floor(M / 4 + 0.5) - 1: the 0-based position of xq
  const uint8_t* mask;  // [num_rows] (null: every row)
  double* elpd_loo;    // [num_rows] of this slab, like the three below
  double* pareto_k;
  double* ess;
  double* lpd;
  long long* count;
};

// the order-preserving image of a double (wn_summary.hip: order_key) and its inverse
__device__ __forceinline__ unsigned long long psis_key(double x) {
  if (x != x) return ~0ull;
  const unsigned long long u = wnd::as_u64(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double psis_key_value(unsigned long long k) {
  return wnd::as_f64((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// exp(x) - 1 with relative accuracy as x -> 0: dexp's reduction x = (64 e + j) ln 2 / 64 + r and its polynomial
// p = exp(r) - 1; with s = 2^e 2^(j/64) the result is p itself when s = 1 and (s - 1) + s p otherwise (s - 1 is exact
// for s in [1/2, 2]; the table entry's rounding is 2^-53 s against a result of ln 2 / 128 or more in magnitude).
// x > 709.78 -> +inf, x < -745.13 -> -1, NaN -> NaN.
template <class Tab>
__device__ __forceinline__ double psis_expm1(double x, const Tab& tab) {
  constexpr double kInvStep = 9.23324826168936567e+01;   // 64 / ln 2
  constexpr double kStepHi = 1.08304246095940471e-02;    // ln 2 / 64, upper 28 bits
  constexpr double kStepLo = 8.66550983900947049e-11;
  constexpr double kOver = 7.09782712893383973096e+02, kUnder = -7.45133219101941108420e+02;
  const double xc = (x != x) ? 0.0 : (x > kOver ? kOver : (x < kUnder ? kUnder : x));
  const double kf = __builtin_floor(wnd::fmad(xc, kInvStep, 0.5));
  const int k = static_cast<int>(kf);
  const double r = wnd::fmad(-kf, kStepLo, wnd::fmad(-kf, kStepHi, xc));
  const double t = tab.exp2(k & 63);
  const int e = k >> 6;
  const double r2 = r * r;
  const double lo = wnd::fmad(r, 1.66666666666666657e-01, 0.5);
  const double hi = wnd::fmad(r, 8.33333333333333322e-03, 4.16666666666666644e-02);
  const double p = wnd::fmad(r2, wnd::fmad(r2, hi, lo), r);
  const int ea = e / 2;
  const int eb = e - ea;
  const double s = (t * wnd::two_to(ea)) * wnd::two_to(eb);
  double y = k == 0 ? p : (s - 1.0) + s * p;
  if (x > kOver) y = __builtin_inf();
  if (x < kUnder) y = -1.0;
  if (x != x) y = x;
  return y;
}

// ---- workgroup reductions (kPsisBlock threads; `pad` holds one value per wavefront) -----------------------------------
// the BLOCK SUM of the header comment: every thread returns the same bits
__device__ __forceinline__ double psis_block_sum(double v, double* pad) {
  v = wave_sum_packed(v, v);  // (both halves hold the wavefront's sum: offsets 32, 1, 2, 4, 8, 16)
  if ((threadIdx.x & 63u) == 0) pad[threadIdx.x >> 6] = v;
  __syncthreads();
  const double total = ((pad[0] + pad[1]) + pad[2]) + pad[3];
  __syncthreads();
  return total;
}
// exact in any order: maximum, minimum, integer sum
struct PsisMax {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};
struct PsisMin {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};
struct PsisAdd {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
template <class T, class Op>
__device__ __forceinline__ T psis_block_reduce(T v, Op op, T* pad) {
  for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
  if ((threadIdx.x & 63u) == 0) pad[threadIdx.x >> 6] = v;
  __syncthreads();
  const T total = op(op(pad[0], pad[1]), op(pad[2], pad[3]));
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(kPsisBlock) void psis_row_kernel(const PsisParams Q) {
  static_assert(kPsisWaves == 4, "the block sum adds four wavefront sums");
  __shared__ unsigned long long tail[kPsisMaxTail];  // ~psis_key(l) of the tail: ascending keys = ascending r
  __shared__ double xs[kPsisMaxTail];                // x_i, then lw_i
  __shared__ unsigned hist[256];
  __shared__ double cand_sum[kPsisMaxCandidates][kPsisWaves];
  __shared__ double cand_b[kPsisMaxCandidates], cand_l[kPsisMaxCandidates], cand_bw[kPsisMaxCandidates];
  __shared__ double pad_d[kPsisWaves];
  __shared__ unsigned long long pad_u[kPsisWaves];
  __shared__ int pad_i[kPsisWaves];
  __shared__ unsigned above;  // draws with key > T collected so far
  const wnd::ArrayTables tab = wnd::array_tables();
  const double inf = __builtin_inf(), nan = __builtin_nan("");
  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
  const int S = Q.num_draws, M = Q.tail, m = Q.candidates;
  const double dM = static_cast<double>(M);
  for (int row = static_cast<int>(blockIdx.x); row < Q.num_rows; row += static_cast<int>(gridDim.x)) {
    if (Q.mask != nullptr && Q.mask[row] == 0) {
      if (tid == 0) {
        Q.elpd_loo[row] = nan;
        Q.pareto_k[row] = nan;
        Q.ess[row] = nan;
        Q.lpd[row] = nan;
        Q.count[row] = 0;
      }
      continue;
    }
    const double* col = Q.lmat + static_cast<long long>(row) * Q.ld;
    // ---- 1. the range of l, and whether every l is finite ----
    double l_min = inf, l_max = -inf;
    int bad = 0;
    for (int s = tid; s < S; s += kPsisBlock) {
      const double l = col[s];
      bad |= (__builtin_fabs(l) < inf) ? 0 : 1;
      l_min = l < l_min ? l : l_min;
      l_max = l > l_max ? l : l_max;
    }
    bad = psis_block_reduce(bad, PsisAdd{}, pad_i);
    if (bad != 0) {
      if (tid == 0) {
        Q.elpd_loo[row] = nan;
        Q.pareto_k[row] = nan;
        Q.ess[row] = nan;
        Q.lpd[row] = nan;
        Q.count[row] = S;
      }
      continue;
    }
    l_min = psis_block_reduce(l_min, PsisMin{}, pad_d);
    l_max = psis_block_reduce(l_max, PsisMax{}, pad_d);
    const double mx = -l_min;
    // ---- 2. T, the key at sorted position S - M: radix select, most significant byte first ----
    unsigned long long T = ~0ull;  // M == 0: every draw lies below the tail
    if (M > 0) {
      unsigned long long prefix = 0;
      unsigned rank = static_cast<unsigned>(S - M);
      for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int s = tid; s < S; s += kPsisBlock) {
          const unsigned long long key = psis_key((-col[s]) - mx);
          if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        unsigned before = 0;
        int bin = 0;
        for (; bin < 255; ++bin) {  // (every thread reads the same words: broadcasts)
          const unsigned c = hist[bin];
          if (rank < before + c) break;
          before += c;
        }
        rank -= before;
        prefix = (prefix << 8) | static_cast<unsigned long long>(bin);
        __syncthreads();
      }
      T = prefix;
    }
    // ---- the tail's l into LDS; what lies below the tail ----
    if (tid == 0) above = 0;
    __syncthreads();
    unsigned long long below_key = 0;  // the largest key below T
    int n_below = 0, n_ties = 0;
    double tie_l = inf;        // the ties' l (the smallest, should they differ)
    double c_below = -inf;     // max of l + lw over the draws below T
    for (int s = tid; s < S; s += kPsisBlock) {
      const double l = col[s];
      const double r = (-l) - mx;
      const unsigned long long key = psis_key(r);
      if (key > T) {
        const unsigned at = atomicAdd(&above, 1u);
        if (at < static_cast<unsigned>(kPsisMaxTail)) tail[at] = ~psis_key(l);
      } else if (key == T) {
        ++n_ties;
        tie_l = l < tie_l ? l : tie_l;
      } else {
        ++n_below;
        below_key = key > below_key ? key : below_key;
        const double t = l + r;
        c_below = t > c_below ? t : c_below;
      }
    }
    __syncthreads();
    const int n_above = static_cast<int>(above);
    n_below = psis_block_reduce(n_below, PsisAdd{}, pad_i);
    n_ties = psis_block_reduce(n_ties, PsisAdd{}, pad_i);
    below_key = psis_block_reduce(below_key, PsisMax{}, pad_u);
    tie_l = psis_block_reduce(tie_l, PsisMin{}, pad_d);
    c_below = psis_block_reduce(c_below, PsisMax{}, pad_d);
    const int ties_in_tail = M - n_above;             // >= 1 when M > 0
    const int ties_below = n_ties - ties_in_tail;     // counted, never listed
    const double tie_r = M > 0 ? psis_key_value(T) : 0.0;
    const double cutoff = M > 0 ? psis_key_value(n_below == S - M ? below_key : T) : 0.0;
    const double e_cutoff = wnd::dexp(cutoff, tab);
    for (int i = n_above + tid; i < Q.tail_padded && i < kPsisMaxTail; i += kPsisBlock)
      tail[i] = i < M ? ~psis_key(tie_l) : ~0ull;
    __syncthreads();
    // ---- bitonic sort of the padded tail, ascending (pair form: header comment) ----
    for (int k = 2; k <= Q.tail_padded; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int p = tid; p < Q.tail_padded / 2; p += kPsisBlock) {
          const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
          const unsigned long long a = tail[i], b = tail[i + j];
          const bool ascending = (i & k) == 0;
          if ((a > b) == ascending) {
            tail[i] = b;
            tail[i + j] = a;
          }
        }
        __syncthreads();
      }
    }
    // ---- 3. the fit ----
    for (int i = tid; i < M; i += kPsisBlock) {
      const double r = (-psis_key_value(~tail[i])) - mx;
      xs[i] = wnd::dexp(r, tab) - e_cutoff;
    }
    __syncthreads();
    bool fitted = false;
    double khat = inf, sigma = 0.0;
    if (M >= kPsisMinFit) {
      const double x_top = xs[M - 1], x_q = xs[Q.quartile];
      if (x_q > 0.0 && x_top > 0.0) {
        const double dm = static_cast<double>(m);
        for (int j = 0; j < m; ++j) {
          const double bj = 1.0 / x_top + (1.0 - __builtin_sqrt(dm / (static_cast<double>(j + 1) - 0.5))) / (3.0 * x_q);
          double part = 0.0;
          for (int i = tid; i < M; i += kPsisBlock) part = part + wnd::dlog1p(-bj * xs[i], tab);
          part = wave_sum_packed(part, part);
          if (lane == 0) cand_sum[j][wave] = part;
          if (tid == 0) cand_b[j] = bj;
        }
        __syncthreads();
        if (tid < m) {
          const double kj = (((cand_sum[tid][0] + cand_sum[tid][1]) + cand_sum[tid][2]) + cand_sum[tid][3]) / dM;
          cand_l[tid] = dM * ((wnd::dlog(-cand_b[tid] / kj, tab) - kj) - 1.0);
        }
        __syncthreads();
        if (tid < m) {
          const double lj = cand_l[tid];
          double total = 0.0;
          for (int i = 0; i < m; ++i) total = total + wnd::dexp(cand_l[i] - lj, tab);
          cand_bw[tid] = cand_b[tid] * (1.0 / total);
        }
        __syncthreads();
        double b = 0.0;
        for (int j = 0; j < m; ++j) b = b + cand_bw[j];
        double part = 0.0;
        for (int i = tid; i < M; i += kPsisBlock) part = part + wnd::dlog1p(-b * xs[i], tab);
        const double k = psis_block_sum(part, pad_d) / dM;
        sigma = -k / b;
        khat = (dM * k + 5.0) / (dM + 10.0);
        fitted = __builtin_fabs(khat) < inf && __builtin_fabs(sigma) < inf;
        if (!fitted) khat = inf;
      }
    }
    // ---- 4. the tail's log weights replace x; the maxima of the final sums ----
    __syncthreads();
    double a_max = -inf, c_max = c_below;
    for (int i = tid; i < M; i += kPsisBlock) {
      const double l = psis_key_value(~tail[i]);
      double lw;
      if (fitted) {
        const double p = (static_cast<double>(i) + 0.5) / dM;
        const double z = wnd::dlog1p(-p, tab);
        lw = wnd::dlog(sigma * psis_expm1(-khat * z, tab) / khat + e_cutoff, tab);
      } else {
        lw = (-l) - mx;
      }
      lw = lw > 0.0 ? 0.0 : lw;
      xs[i] = lw;
      a_max = lw > a_max ? lw : a_max;
      const double t = l + lw;
      c_max = t > c_max ? t : c_max;
    }
    // (below the tail lw = r: its maximum is the cutoff -- or 0, the largest r there is, without a tail)
    if (S - M > 0) a_max = cutoff > a_max ? cutoff : a_max;
    if (ties_below > 0) {
      const double t = tie_l + tie_r;
      c_max = t > c_max ? t : c_max;
    }
    a_max = psis_block_reduce(a_max, PsisMax{}, pad_d);  // (its barriers also publish lw)
    c_max = psis_block_reduce(c_max, PsisMax{}, pad_d);
    // ---- 5. the final sums ----
    double sa = 0.0, sq = 0.0, sb = 0.0, sd = 0.0;
    for (int s = tid; s < S; s += kPsisBlock) {
      const double l = col[s];
      const double r = (-l) - mx;
      if (psis_key(r) < T) {
        const double e = wnd::dexp(r - a_max, tab);
        sa = sa + e;
        sq = sq + e * e;
        sb = sb + wnd::dexp((l + r) - c_max, tab);
        sd = sd + wnd::dexp(l - l_max, tab);
      }
    }
    sa = psis_block_sum(sa, pad_d);
    sq = psis_block_sum(sq, pad_d);
    sb = psis_block_sum(sb, pad_d);
    sd = psis_block_sum(sd, pad_d);
    if (ties_below > 0) {
      const double n = static_cast<double>(ties_below);
      const double e = wnd::dexp(tie_r - a_max, tab);
      sa = sa + n * e;
      sq = sq + n * (e * e);
      sb = sb + n * wnd::dexp((tie_l + tie_r) - c_max, tab);
      sd = sd + n * wnd::dexp(tie_l - l_max, tab);
    }
    double ta = 0.0, tq = 0.0, tb = 0.0, td = 0.0;
    for (int i = tid; i < M; i += kPsisBlock) {
      const double l = psis_key_value(~tail[i]);
      const double lw = xs[i];
      const double e = wnd::dexp(lw - a_max, tab);
      ta = ta + e;
      tq = tq + e * e;
      tb = tb + wnd::dexp((l + lw) - c_max, tab);
      td = td + wnd::dexp(l - l_max, tab);
    }
    sa = sa + psis_block_sum(ta, pad_d);
    sq = sq + psis_block_sum(tq, pad_d);
    sb = sb + psis_block_sum(tb, pad_d);
    sd = sd + psis_block_sum(td, pad_d);
    if (tid == 0) {
      Q.elpd_loo[row] = (c_max + wnd::dlog(sb, tab)) - (a_max + wnd::dlog(sa, tab));
      Q.pareto_k[row] = khat;
      Q.ess[row] = (sa * sa) / sq;
      Q.lpd[row] = (l_max + wnd::dlog(sd, tab)) - wnd::dlog(static_cast<double>(S), tab);
      Q.count[row] = S;
    }
    __syncthreads();  // (the next row reuses the LDS)
  }
}

}  // namespace wn
