// wn_engine_elementwise.hip -- the engine's element-wise passes: everything that launches a kernel of wn_elementwise.h
// (whose kernels are static: this is the one unit that includes it).  Fills, the adapters' start and freeze, the
// inverse-mass estimate, the gradient count, and the cross-chain monitors.
#include "wn_engine.h"

#include "wn_elementwise.h"
#include "wn_monitor.h"

void wn_engine::fill(DevBuf<double>& b, double v) {
  const int blocks = static_cast<int>(std::min<size_t>((b.n + 255) / 256, 4096));
  hipLaunchKernelGGL(wn::fill_kernel, dim3(blocks), dim3(256), 0, stream, b.p, static_cast<long long>(b.n), v);
  HIP_OK(hipGetLastError());
}

void wn_engine::ensure_adapters() {
  if (adapters_ready) return;
  use_device();
  const int blocks = static_cast<int>(std::min<size_t>((C * Dp + 255) / 256, 4096));
  hipLaunchKernelGGL(wn::begin_warmup_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<int>(C), Dp,
                     cfg.mass_init_count, mass.p, draw_mean.p, draw_ssd.p, score_mean.p, score_ssd.p,
                     est_weight.p, step_init.p, adam.p, mm_state.p);
  HIP_OK(hipGetLastError());
  adapters_ready = true;
  warmup_iter = 0;
  est_pending = false;
}

void wn_engine::alloc_monitors() {
  // sized for the engine's G segments of k chains, which covers the pooled (1, C): G * runs(k) >= runs(G * k)
  const size_t G = static_cast<size_t>(num_datasets);
  mon_runs.alloc(2 * G * static_cast<size_t>(wn::monitor_runs(static_cast<int>(C / G))));
  mon_sums.alloc(G * (1 + static_cast<size_t>(D)));
  mon_out.alloc(2 * G);
}

extern "C" {

int wn_engine_freeze(wn_engine* e, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr) throw std::invalid_argument("null argument");
    e->ensure_adapters();
    e->use_device();
    const int blocks = static_cast<int>(std::min<size_t>((e->C * e->Dp + 255) / 256, 4096));
    hipLaunchKernelGGL(wn::freeze_kernel, dim3(blocks), dim3(256), 0, e->stream, static_cast<int>(e->C), e->Dp,
                       e->draw_ssd.p, e->score_ssd.p, e->est_weight.p, e->adam.p, e->mm_state.p,
                       e->cfg.max_macro_steps_target, e->cfg.min_micro_steps, e->inv_mass.p, e->chol_mass.p,
                       e->step_size.p, e->min_micro.p);
    HIP_OK(hipGetLastError());
    e->frozen = true;
    if (e->ref_streams)  // WalnutsSampler builds a new detail::Random over the same engine (walnuts.hpp:642)
      e->ref_streams->normal.assign(e->C, std::normal_distribution<double>(0.0, 1.0));
  });
}
int wn_engine_get_inv_mass(wn_engine* e, double* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument");
    if (!e->frozen) {
      e->ensure_adapters();
      e->use_device();
      const int blocks = static_cast<int>(std::min<size_t>((e->C * e->Dp + 255) / 256, 4096));
      hipLaunchKernelGGL(wn::inv_mass_estimate_kernel, dim3(blocks), dim3(256), 0, e->stream, static_cast<int>(e->C),
                         e->Dp, e->draw_ssd.p, e->score_ssd.p, e->est_weight.p, e->inv_mass.p);
      HIP_OK(hipGetLastError());
    }
    e->download_rows(e->inv_mass, out);
  });
}
int wn_engine_total_grad_evals(wn_engine* e, int64_t* out, WalnutpyError** err) {
  return guarded(err, [&] {
    e->use_device();
    HIP_OK(hipMemsetAsync(e->scratch64.p, 0, sizeof(unsigned long long), e->stream));
    hipLaunchKernelGGL(wn::sum_i64_kernel, dim3(std::min<size_t>(256, (e->C + 255) / 256)), dim3(256), 0, e->stream, e->grad_evals.p,
                       static_cast<int>(e->C), e->scratch64.p);
    HIP_OK(hipGetLastError());
    unsigned long long v = 0;
    HIP_OK(hipMemcpyAsync(&v, e->scratch64.p, sizeof(v), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    *out = static_cast<int64_t>(v);
  });
}

// ---- cross-chain monitors (adapt.hpp:172-229, sampler.hpp:117-158) ---------------------------------
// One routine per statistic over G segments of k consecutive chains (wn_elementwise.h).  The pooled entry points run it
// at (1, C); the _datasets ones at (num_datasets, chains_per_dataset), where dataset g's value is what the pooled entry
// point returns on a standalone engine of its k chains.  The two stages a multi-GPU driver all-reduces in between
// (wn_engine_lp_sums / _lp_sq_dev, wn_engine_warmup_sums / _warmup_max_rel) are the routines' stages at G = 1.
namespace {
int monitor_grid(size_t n) { return static_cast<int>(std::max<size_t>(1, (n + 255) / 256)); }

// R-hat, stage 1 -> mon_sums[G][2]: the sums of the chains' lp means and sample variances
void lp_sums_stage(wn_engine& e, int G, int k) {
  const int per = wn::monitor_runs(k);
  hipLaunchKernelGGL(wn::lp_sums_kernel, dim3(monitor_grid(static_cast<size_t>(G) * per)), dim3(256), 0, e.stream, G, k,
                     e.lp_stats.p, e.mon_runs.p);
  hipLaunchKernelGGL(wn::finish_sums_kernel<2>, dim3(monitor_grid(G)), dim3(256), 0, e.stream, e.mon_runs.p, G, per,
                     e.mon_sums.p, 2);
  HIP_OK(hipGetLastError());
}
// stage 2 -> mon_out[G]: the sums of squared deviations from the means of means mon_sums[2g] / n
void lp_sq_dev_stage(wn_engine& e, int G, int k, double n) {
  const int per = wn::monitor_runs(k);
  hipLaunchKernelGGL(wn::lp_sqdev_kernel, dim3(monitor_grid(static_cast<size_t>(G) * per)), dim3(256), 0, e.stream, G,
                     k, e.lp_stats.p, e.mon_sums.p, n, e.mon_runs.p);
  hipLaunchKernelGGL(wn::finish_sums_kernel<1>, dim3(monitor_grid(G)), dim3(256), 0, e.stream, e.mon_runs.p, G, per,
                     e.mon_out.p, 1);
  HIP_OK(hipGetLastError());
}
void rhat_segments(wn_engine& e, int G, int k, double* rhat) {
  e.use_device();
  lp_sums_stage(e, G, k);
  lp_sq_dev_stage(e, G, k, k);
  std::vector<double> s(2 * static_cast<size_t>(G)), q(static_cast<size_t>(G));
  e.download(e.mon_sums, s.data(), s.size());
  e.download(e.mon_out, q.data(), q.size());
  for (int g = 0; g < G; ++g) rhat[g] = wn::rhat_from_sums(s[2 * g + 1], q[g], k);
}

void begin_warmup_monitor(wn_engine& e) {
  if (e.frozen) throw std::runtime_error("warmup monitor after freeze");
  e.ensure_adapters();
  e.use_device();
}
// warmup spread, stage 1 -> mon_sums[G][1 + D]: the sums of log step, then of log mass per dimension
void warmup_sums_stage(wn_engine& e, int G, int k) {
  const int per = wn::monitor_runs(k);
  hipLaunchKernelGGL(wn::log_step_sum_kernel, dim3(monitor_grid(static_cast<size_t>(G) * per)), dim3(256), 0, e.stream,
                     G, k, e.adam.p, e.mon_runs.p);
  hipLaunchKernelGGL(wn::finish_sums_kernel<1>, dim3(monitor_grid(G)), dim3(256), 0, e.stream, e.mon_runs.p, G, per,
                     e.mon_sums.p, 1 + e.D);
  hipLaunchKernelGGL(wn::log_mass_colsum_kernel, dim3(monitor_grid(static_cast<size_t>(G) * e.D)), dim3(256), 0,
                     e.stream, G, k, e.D, e.Dp, e.draw_ssd.p, e.score_ssd.p, e.est_weight.p, e.mon_sums.p);
  HIP_OK(hipGetLastError());
}
// stage 2 -> mon_out[G][2]: the largest relative distances (mass, step) from the geometric means of mon_sums over n
// chains
void warmup_max_rel_stage(wn_engine& e, int G, int k, double n) {
  hipLaunchKernelGGL(wn::warmup_spread_kernel, dim3(G * k), dim3(256), 0, e.stream, k, e.D, e.Dp, e.draw_ssd.p,
                     e.score_ssd.p, e.est_weight.p, e.adam.p, e.mon_sums.p, n, e.mon_rel_mass.p, e.mon_rel_step.p);
  hipLaunchKernelGGL(wn::max2_kernel, dim3(G), dim3(256), 0, e.stream, k, e.mon_rel_mass.p, e.mon_rel_step.p,
                     e.mon_out.p);
  HIP_OK(hipGetLastError());
}
void warmup_spread_segments(wn_engine& e, int G, int k, double* max_rel_diff_step, double* max_rel_diff_mass) {
  begin_warmup_monitor(e);
  warmup_sums_stage(e, G, k);
  warmup_max_rel_stage(e, G, k, k);
  std::vector<double> m(2 * static_cast<size_t>(G));
  e.download(e.mon_out, m.data(), m.size());
  for (int g = 0; g < G; ++g) {
    max_rel_diff_mass[g] = m[2 * g];
    max_rel_diff_step[g] = m[2 * g + 1];
  }
}

void average_masses_segments(wn_engine& e, int G, int k) {
  e.use_device();
  hipLaunchKernelGGL(wn::mass_log_colsum_kernel, dim3(monitor_grid(static_cast<size_t>(G) * e.D)), dim3(256), 0,
                     e.stream, G, k, e.D, e.Dp, e.mass.p, e.mon_sums.p);
  const int blocks = static_cast<int>(std::min<size_t>((e.C * e.Dp + 255) / 256, 4096));
  hipLaunchKernelGGL(wn::mass_broadcast_kernel, dim3(blocks), dim3(256), 0, e.stream, static_cast<int>(e.C), k, e.D,
                     e.Dp, e.mon_sums.p, e.mass.p);
  HIP_OK(hipGetLastError());
  e.adapters_ready = false;
}

void require_datasets(const wn_engine* e) {
  if (e->obs.chains_per_dataset == 0)
    throw std::invalid_argument("this engine holds no datasets (wn_engine_create_observed with obs_offsets or weight sets)");
}
}  // namespace

int wn_engine_lp_sums(wn_engine* e, double* out /*[3]: sum of means, sum of sample variances, chains*/,
                      WalnutpyError** err) {
  return guarded(err, [&] {
    e->use_device();
    lp_sums_stage(*e, 1, static_cast<int>(e->C));
    e->download(e->mon_sums, out, 2);
    out[2] = static_cast<double>(e->C);
  });
}
int wn_engine_lp_sq_dev(wn_engine* e, double mean_of_means, double* out, WalnutpyError** err) {
  return guarded(err, [&] {
    e->use_device();
    // the caller's mean of means (over its chains on every engine) stands as the sum over one chain: x / 1 is x
    HIP_OK(hipMemcpyAsync(e->mon_sums.p, &mean_of_means, sizeof(double), hipMemcpyHostToDevice, e->stream));
    lp_sq_dev_stage(*e, 1, static_cast<int>(e->C), 1.0);
    e->download(e->mon_out, out, 1);
  });
}
int wn_engine_rhat(wn_engine* e, double* rhat, WalnutpyError** err) {
  return guarded(err, [&] { rhat_segments(*e, 1, static_cast<int>(e->C), rhat); });
}
// The warmup controller's statistic (adapt.hpp:193-221) in the two stages a multi-GPU driver needs: (1) this
// engine's sums over chains of log step and of log mass per dimension -- D+1 doubles to all-reduce (SUM) --,
// (2) given the sums over ALL chains, this engine's largest relative distances -- 2 doubles to all-reduce (MAX).
int wn_engine_warmup_sums(wn_engine* e, double* sum_log_step, double* colsum_log_mass, WalnutpyError** err) {
  return guarded(err, [&] {
    begin_warmup_monitor(*e);
    warmup_sums_stage(*e, 1, static_cast<int>(e->C));
    std::vector<double> sums(1 + static_cast<size_t>(e->D));
    e->download(e->mon_sums, sums.data(), sums.size());
    *sum_log_step = sums[0];
    std::copy(sums.begin() + 1, sums.end(), colsum_log_mass);
  });
}
int wn_engine_warmup_max_rel(wn_engine* e, double sum_log_step, const double* colsum_log_mass, size_t total_chains,
                             double* max_rel_diff_step, double* max_rel_diff_mass, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e->frozen) throw std::runtime_error("warmup monitor after freeze");
    if (total_chains < e->C) throw std::invalid_argument("total_chains is smaller than this engine's chain count");
    e->ensure_adapters();
    e->use_device();
    std::vector<double> sums(1 + static_cast<size_t>(e->D));
    sums[0] = sum_log_step;
    std::copy(colsum_log_mass, colsum_log_mass + e->D, sums.begin() + 1);
    HIP_OK(hipMemcpyAsync(e->mon_sums.p, sums.data(), sums.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    warmup_max_rel_stage(*e, 1, static_cast<int>(e->C), static_cast<double>(total_chains));
    double m[2];
    e->download(e->mon_out, m, 2);
    *max_rel_diff_mass = m[0];
    *max_rel_diff_step = m[1];
  });
}
int wn_engine_warmup_spread(wn_engine* e, double* max_rel_diff_step, double* max_rel_diff_mass, WalnutpyError** err) {
  return guarded(err, [&] {
    warmup_spread_segments(*e, 1, static_cast<int>(e->C), max_rel_diff_step, max_rel_diff_mass);
  });
}
int wn_engine_average_masses(wn_engine* e, WalnutpyError** err) {
  return guarded(err, [&] { average_masses_segments(*e, 1, static_cast<int>(e->C)); });
}

int wn_engine_rhat_datasets(wn_engine* e, double* rhat, WalnutpyError** err) {
  return guarded(err, [&] {
    if (rhat == nullptr) throw std::invalid_argument("null argument");
    require_datasets(e);
    rhat_segments(*e, e->num_datasets, e->obs.chains_per_dataset, rhat);
  });
}
int wn_engine_warmup_spread_datasets(wn_engine* e, double* max_rel_diff_step, double* max_rel_diff_mass,
                                     WalnutpyError** err) {
  return guarded(err, [&] {
    if (max_rel_diff_step == nullptr || max_rel_diff_mass == nullptr) throw std::invalid_argument("null argument");
    require_datasets(e);
    warmup_spread_segments(*e, e->num_datasets, e->obs.chains_per_dataset, max_rel_diff_step, max_rel_diff_mass);
  });
}
int wn_engine_average_masses_datasets(wn_engine* e, WalnutpyError** err) {
  return guarded(err, [&] {
    require_datasets(e);
    average_masses_segments(*e, e->num_datasets, e->obs.chains_per_dataset);
  });
}
// The driver's one-shard controller looks (wn_sample.hip): per dataset, or pooled on an engine without datasets
extern "C" int wn_internal_rhat_segments(wn_engine* e, double* rhat, WalnutpyError** err) {
  return guarded(err, [&] { rhat_segments(*e, e->num_datasets, static_cast<int>(e->C) / e->num_datasets, rhat); });
}
extern "C" int wn_internal_warmup_spread_segments(wn_engine* e, double* max_rel_diff_step, double* max_rel_diff_mass,
                                                  WalnutpyError** err) {
  return guarded(err, [&] {
    warmup_spread_segments(*e, e->num_datasets, static_cast<int>(e->C) / e->num_datasets, max_rel_diff_step,
                           max_rel_diff_mass);
  });
}

}  // extern "C"
