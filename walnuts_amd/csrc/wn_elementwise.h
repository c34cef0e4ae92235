// wn_elementwise.h -- element-wise kernels around the transition kernel (its kernels are static: included by
// wn_engine_elementwise.hip only).
#pragma once

#include "wn_devmath.h"
#include "wn_hip.h"

namespace wn {

// AdaptiveWalnuts construction (adaptive_walnuts.hpp:205-223): estimator planes from the
// init mass (:54-62), Adam on log step (adam.hpp:48-62), min-micro handler (:127-132)
static __global__ void begin_warmup_kernel(int C, int Dp, double count, const double* mass, double* draw_mean,
                                    double* draw_ssd, double* score_mean, double* score_ssd, double* est_weight,
                                    const double* step_init, double* adam, double* mm_state) {
  const long long n = static_cast<long long>(C) * Dp;
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const double m = mass[i];
    draw_mean[i] = 0.0;
    score_mean[i] = 0.0;
    score_ssd[i] = count * m;
    draw_ssd[i] = count * (1.0 / m);
    if (i < C) {
      est_weight[2 * i] = count;
      est_weight[2 * i + 1] = count;
      adam[6 * i + 0] = wnd::dlog(step_init[i]);
      adam[6 * i + 1] = 0.0;
      adam[6 * i + 2] = 0.0;
      adam[6 * i + 3] = 0.0;
      adam[6 * i + 4] = 1.0;
      adam[6 * i + 5] = 1.0;
      mm_state[2 * i] = 2.0;
      mm_state[2 * i + 1] = 1.0;
    }
  }
}

// AdaptiveWalnuts::sampler() (adaptive_walnuts.hpp:263-271)
static __global__ void freeze_kernel(int C, int Dp, const double* draw_ssd, const double* score_ssd,
                              const double* est_weight, const double* adam, const double* mm_state,
                              double macro_target, int cfg_min_micro, double* inv_mass, double* chol_mass,
                              double* step_size, int* min_micro) {
  const long long n = static_cast<long long>(C) * Dp;
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const long long c = i / Dp;
    const wnd::SharedDivisor wd(est_weight[2 * c]), ws(est_weight[2 * c + 1]);  // (as the warmup transitions divide)
    const double im = __builtin_sqrt((draw_ssd[i] / wd) / (score_ssd[i] / ws));
    inv_mass[i] = im;
    chol_mass[i] = 1.0 / __builtin_sqrt(im);  // walnuts.hpp:647
    if (i < C) {
      step_size[i] = wnd::dexp(adam[6 * i]);
      const double mean_micro = mm_state[2 * i] / mm_state[2 * i + 1];
      const long long est = static_cast<long long>(__builtin_round(mean_micro / macro_target));
      min_micro[i] = static_cast<int>(est > cfg_min_micro ? est : cfg_min_micro);
    }
  }
}

// AdaptiveWalnuts::inv_mass() during warmup (adaptive_walnuts.hpp:89-94, :297-299): the estimate the NEXT warmup
// transition will integrate with, written to the (otherwise idle before freeze) inverse-mass plane
static __global__ void inv_mass_estimate_kernel(int C, int Dp, const double* draw_ssd, const double* score_ssd,
                                                const double* est_weight, double* inv_mass) {
  const long long n = static_cast<long long>(C) * Dp;
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const long long c = i / Dp;
    inv_mass[i] = __builtin_sqrt((draw_ssd[i] / wnd::SharedDivisor(est_weight[2 * c])) / (score_ssd[i] / wnd::SharedDivisor(est_weight[2 * c + 1])));
  }
}

// ---- cross-chain monitors (the reference's controller loops) --------------------------------------
// Every monitor runs over G SEGMENTS of k consecutive chains, segment g being chains [g * k, (g + 1) * k): the pooled
// statistic is the one segment (1, C), an engine with datasets has one segment per dataset.  One launch per stage
// whatever G is.  Sums over a segment's chains are deterministic two-stage sums, independent of the launch geometry:
// stage 1 adds every RUN of kMonitorRun consecutive chains left to right (one thread per run; the runs start at the
// segment's first chain), stage 2 (one thread per segment) adds its run totals left to right.  Up to kMonitorRun chains
// that IS the left-to-right sum; beyond, the test suite's CPU restatement groups the same way (its chain_sum), so the
// statistics are compared bit for bit.
constexpr int kMonitorRun = 256;
inline int monitor_runs(int n) { return (n + kMonitorRun - 1) / kMonitorRun; }

template <int K, class F>
static __device__ void run_partial_sums(int G, int k, F f, double* partial /*[G][runs per segment][K]*/) {
  const int per = (k + kMonitorRun - 1) / kMonitorRun, runs = G * per;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < runs; r += gridDim.x * blockDim.x) {
    double acc[K];
    for (int q = 0; q < K; ++q) acc[q] = 0.0;
    const int g = r / per, first = g * k;
    const int lo = first + (r - g * per) * kMonitorRun, end = first + k;
    const int hi = lo + kMonitorRun < end ? lo + kMonitorRun : end;
    for (int i = lo; i < hi; ++i) f(g, i, acc);
    for (int q = 0; q < K; ++q) partial[r * K + q] = acc[q];
  }
}
// segment g's K sums -> out[g * stride + q]
template <int K>
static __global__ void finish_sums_kernel(const double* partial, int G, int per, double* out, int stride) {
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < G; g += gridDim.x * blockDim.x) {
    for (int q = 0; q < K; ++q) {
      double s = 0.0;
      for (int b = 0; b < per; ++b) s += partial[(g * per + b) * K + q];
      out[g * stride + q] = s;
    }
  }
}
// sampling monitor, sampler.hpp:132-145: sums of the per-chain lp means and sample variances
static __global__ void lp_sums_kernel(int G, int k, const double* lp_stats, double* partial) {
  run_partial_sums<2>(G, k, [&](int, int c, double* acc) {
    const double n = lp_stats[3 * c], mean = lp_stats[3 * c + 1], m2 = lp_stats[3 * c + 2];
    acc[0] += mean;
    acc[1] += n > 1 ? m2 / (n - 1) : __builtin_nan("");  // WelfordAccumulator::sample_variance
  }, partial);
}
// squared deviations of the chain means from their segment's mean of means, sums[2g] / n (n: the chains behind sums)
static __global__ void lp_sqdev_kernel(int G, int k, const double* lp_stats, const double* sums /*[G][2]*/, double n,
                                       double* partial) {
  run_partial_sums<1>(G, k, [&](int g, int c, double* acc) {
    const double d = lp_stats[3 * c + 1] - sums[2 * g] / n;
    acc[0] += d * d;
  }, partial);
}
// warmup monitor, adapt.hpp:193-221.  Stage 1 per segment, into sums[G][1 + D]: the sum of log step (from Adam's
// theta), then the D column sums of log mass = -log(inv_mass)
static __global__ void log_step_sum_kernel(int G, int k, const double* adam, double* partial) {
  run_partial_sums<1>(G, k, [&](int, int c, double* acc) { acc[0] += wnd::dlog(wnd::dexp(adam[6 * c])); }, partial);
}
// thread per (segment, column), its chains in order (coalesced rows)
static __global__ void log_mass_colsum_kernel(int G, int k, int D, int Dp, const double* draw_ssd,
                                              const double* score_ssd, const double* est_weight, double* sums) {
  const long long t = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  if (t >= static_cast<long long>(G) * D) return;
  const int g = static_cast<int>(t / D), d = static_cast<int>(t - static_cast<long long>(g) * D);
  double s = 0.0;
  for (int c = g * k; c < (g + 1) * k; ++c) {
    const long long i = static_cast<long long>(c) * Dp + d;
    const double im = __builtin_sqrt((draw_ssd[i] / wnd::SharedDivisor(est_weight[2 * c])) / (score_ssd[i] / wnd::SharedDivisor(est_weight[2 * c + 1])));
    s += -wnd::dlog(im);
  }
  sums[static_cast<long long>(g) * (1 + D) + 1 + d] = s;
}
// Stage 2, block per chain: l2_rel_diff(mass_m, geom_mean_mass) (util.hpp:379-382) and the rel. diff of the step,
// against the geometric means of its segment's sums[g] over n chains
static __global__ void warmup_spread_kernel(int k, int D, int Dp, const double* draw_ssd, const double* score_ssd,
                                            const double* est_weight, const double* adam, const double* sums, double n,
                                            double* rel_mass, double* rel_step) {
  __shared__ double sh[256];
  const int c = blockIdx.x;
  const double* seg = sums + static_cast<long long>(c / k) * (1 + D);
  double acc = 0.0;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const long long i = static_cast<long long>(c) * Dp + d;
    const double im = __builtin_sqrt((draw_ssd[i] / wnd::SharedDivisor(est_weight[2 * c])) / (score_ssd[i] / wnd::SharedDivisor(est_weight[2 * c + 1])));
    const double mass = wnd::dexp(-wnd::dlog(im));                       // snap.mass, adapt.hpp:141
    const double gm = wnd::dexp(seg[1 + d] / n);                         // geom_mean_mass, adapt.hpp:203-205
    const double r = (mass - gm) / gm;
    acc += r * r;
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    rel_mass[c] = __builtin_sqrt(sh[0]);
    const double gms = wnd::dexp(seg[0] / n);                            // adapt.hpp:201-202
    rel_step[c] = (wnd::dexp(wnd::dlog(wnd::dexp(adam[6 * c]))) - gms) / gms;  // adapt.hpp:213-215
  }
}
// block per segment: out[g] = (largest of a, largest of b) over its chains (std::fmax from 0.0, adapt.hpp:208-216),
// 256 threads striding, then a tree
static __global__ void max2_kernel(int k, const double* a, const double* b, double* out /*[G][2]*/) {
  __shared__ double sa[256], sb[256];
  const long long first = static_cast<long long>(blockIdx.x) * k;
  double ma = 0.0, mb = 0.0;
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    ma = fmax(ma, a[first + i]);
    mb = fmax(mb, b[first + i]);
  }
  sa[threadIdx.x] = ma;
  sb[threadIdx.x] = mb;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) {
      sa[threadIdx.x] = fmax(sa[threadIdx.x], sa[threadIdx.x + s]);
      sb[threadIdx.x] = fmax(sb[threadIdx.x], sb[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = sa[0];
    out[2 * blockIdx.x + 1] = sb[0];
  }
}
// InitConfigBuilder::masses(..., average_masses = true), config.hpp:371-380: every chain's mass becomes the geometric
// mean over its segment's chains.  Thread per (segment, column); chains summed in order.
static __global__ void mass_log_colsum_kernel(int G, int k, int D, int Dp, const double* mass, double* geom /*[G][D]*/) {
  const long long t = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  if (t >= static_cast<long long>(G) * D) return;
  const int g = static_cast<int>(t / D), d = static_cast<int>(t - static_cast<long long>(g) * D);
  double s = 0.0;
  for (int c = g * k; c < (g + 1) * k; ++c) s += wnd::dlog(mass[static_cast<long long>(c) * Dp + d]);
  geom[t] = wnd::dexp(s / static_cast<double>(k));
}
static __global__ void mass_broadcast_kernel(int C, int k, int D, int Dp, const double* geom, double* mass) {
  const long long n = static_cast<long long>(C) * Dp;
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const long long c = i / Dp;
    const int d = static_cast<int>(i - c * Dp);
    if (d < D) mass[i] = geom[(c / k) * D + d];
  }
}

static __global__ void fill_kernel(double* p, long long n, double v) {
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x)
    p[i] = v;
}
static __global__ void sum_i64_kernel(const int64_t* v, int n, unsigned long long* out) {
  unsigned long long acc = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    acc += static_cast<unsigned long long>(v[i]);
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}

}  // namespace wn
