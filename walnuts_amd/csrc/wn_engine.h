// wn_engine.h -- the engine's state: struct wn_engine behind the C ABI in include/walnuts_hip.h, shared by the engine's
// translation units (wn_engine.hip: transitions, initialisation and the plain entry points; wn_engine_build.hip:
// wn_engine_create*; wn_engine_elementwise.hip: the element-wise passes and cross-chain monitors;
// wn_engine_pointwise.hip: pointwise scoring; wn_engine_predict.hip: predictions).  Members that launch a kernel are only declared here: each is defined in
// the one unit that includes the kernels' header, so no unit compiles another's kernels.
#ifndef WN_ENGINE_H
#define WN_ENGINE_H
#include "wn_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/walnuts_hip.h"
#include "wn_launch.h"

#include "wn_host.h"

// Host-side reproduction of the reference's per-chain random streams (api.hpp:46-51 + detail::Random,
// util.hpp:78-162): engine m = mt19937_64(seed_seq{seed, m+1}); per transition D normals (libstdc++'s polar
// method with its cached second variate), then one engine output per bernoulli / uniform.  The variates are
// generated here and fed to the kernel (kRngBuffer); after the launch each engine is advanced by the number of
// scalar draws its chain actually consumed.  Parity mode for small runs: one host round trip per transition.
struct ReferenceStreams {
  std::vector<std::mt19937_64> eng;
  std::vector<std::normal_distribution<double>> normal;
  std::vector<std::mt19937_64> after_normals;
  std::vector<double> z, u;
  std::vector<int32_t> used;
  int pool = 0;
};

struct wn_engine {
  int model = 0, D = 0, Dp = 0;
  size_t C = 0;
  wn_config cfg{};
  wn::Geometry geo{};
  int device = 0;
  int num_cus = 256;
  int grid = 0;
  int pool_lds = 0, pool_total = 0;
  bool im_in_lds = false;  // streaming kernels: the chain's inverse mass parked in LDS (wn_traj.h: TrajMem::im_lds)
  bool no_far_end_sums = false;  // experiment switch (WALNUTS_AMD_NO_FAR_END_SUMS=1)
  bool hold_moving_end = false;  // streaming kernels: the moving end's (theta, rho) stay in registers (TrajMem, HOLD)
  int64_t arena_stride = 0;  // doubles per persistent workgroup: HBM part of the span pool (+ streaming scratch)
  size_t smem = 0;
  hipStream_t stream = nullptr;

  DevBuf<double> theta, mass, inv_mass, chol_mass, draw_mean, draw_ssd, score_mean, score_ssd;
  DevBuf<double> step_init, step_size, adam, est_weight, mm_state, logp, model_params, arena, z_buf, u_buf;
  // the cross-chain monitors (wn_elementwise.h): run partials, stage-1 sums [G][1 + D] (R-hat: [G][2]; mass averaging:
  // [G][D]), stage-2 results [G][2], and per chain the relative distances of the warmup spread
  DevBuf<double> lp_stats, mon_runs, mon_sums, mon_out, mon_rel_mass, mon_rel_step;
  // a data model's observations, as the kernels take them (wn_params.h), and the buffers `obs` points into: x
  // [rows][obs.stride] (rows padded with zeros), y [rows]; with several datasets one after another, dataset g being rows
  // [offsets[g], offsets[g + 1]) and chains [g * k, (g + 1) * k), k = obs.chains_per_dataset; a grouped model's group
  // of every row, its x (P = D - J - 1 columns) at the narrower stride 128 * ceil(P / 128); optional offsets and weights
  // of every row, or weight sets: one block of rows, num_datasets weight vectors, k chains each
  wn::Observations obs{};
  DevBuf<double> data_x, data_y, data_offset, data_weight;  // (weight: [num_datasets][num_obs] with weight sets)
  DevBuf<double> data_const;  // beside y: the constant c_n(y_n) a row's pointwise log-likelihood carries (wn_pointwise.h)
  size_t data_rows = 0;       // rows of the observation block
  DevBuf<int64_t> data_offsets;
  DevBuf<int32_t> data_group;
  int num_datasets = 1;
  DevBuf<int32_t> min_micro, depth, rng_draws, failed_ext;
  DevBuf<int64_t> grad_evals;
  DevBuf<uint32_t> counter, error_flags;
  DevBuf<unsigned long long> scratch64;

  uint64_t seed = 0;
  uint32_t chain_offset = 0;
  uint32_t transition = 0;
  int64_t warmup_iter = 0;
  int64_t iteration = 0;
  bool adapters_ready = false;
  bool frozen = false;
  bool variates_pending = false;
  int u_stride = 0;
  std::unique_ptr<ReferenceStreams> ref_streams;

  // HIP event pairs around the transition launches: a fixed ring (the last kEventRing launches since the last
  // timing reset can be read back), created once
  static constexpr size_t kEventRing = 1024;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  size_t events_used = 0;  // launches since the last timing reset
  bool timing = false;     // record events around the launches (wn_engine_timing_reset switches it on)
  hipEvent_t region_begin = nullptr, region_end = nullptr;  // wn_engine_region_begin / _region_ms
  size_t region_launches = 0;
  bool own_stream = true;
  // Chain groups (round 4): with few work items per resident workgroup (config #2: 4, config #3: 5) a launch's tail --
  // the last chains finishing while the chip drains -- is 25-45 % of it (profiles/r03/item_balance.txt).  The chains are
  // then split into `groups` contiguous blocks, each with its own stream, chain counter and arena slice, launched
  // independently: nothing orders group 1's launch n + 1 behind group 0's launch n, so one group's tail is filled by the
  // other's workgroups (two engines on two streams measured +12 % / +23 % on configs #2 / #3 and +2 % on the headline,
  // profiles/r03/two_groups.txt; in the engine: +13 % / +26 % / +2 %, profiles/r04/ab_chain_groups.txt -- as long as
  // nothing re-aligns the groups: a join of the streams at every step gives the lock-step numbers back).  Everything
  // else the engine does runs on `stream` and first waits for the groups (join_groups(), reached through use_device()).
  static constexpr int kMaxGroups = 4;
  int groups = 1;
  size_t group_begin[kMaxGroups + 1] = {};
  int group_grid[kMaxGroups] = {};
  hipStream_t gstream[kMaxGroups] = {};  // [0] is `stream`
  hipEvent_t gdone[kMaxGroups] = {}, main_point = nullptr;
  hipEvent_t ext_point = nullptr, rel_point = nullptr;  // wn_engine_wait_stream / _release_stream
  uint32_t work_base[kMaxGroups] = {};  // value of each group's device-side chain counter at its next launch
  // register kernels, warmup: the mass estimator's observation of a launch's last transition is applied by the next
  // launch's first prologue (wn_chip.h kDeferObservation).  Until then it is PENDING: the planes and weights hold the
  // state before it, the position plane what it will observe.  Everything but a warmup launch applies it first
  // (flush_pending_observation(), reached through use_device()), so nothing outside the kernels ever sees the difference.
  bool est_pending = false;
  bool in_flush = false;
  bool groups_ahead = false;  // a group stream holds launches `stream` has not waited for
  bool main_moved = true;     // `stream` has done something since the groups last waited for it
  bool in_step = false;

  ~wn_engine() {
    for (auto& ev : events) {
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
    if (region_begin) (void)hipEventDestroy(region_begin);
    if (region_end) (void)hipEventDestroy(region_end);
    for (int g = 1; g < kMaxGroups; ++g) {
      if (gstream[g]) (void)hipStreamDestroy(gstream[g]);
      if (gdone[g]) (void)hipEventDestroy(gdone[g]);
    }
    if (main_point) (void)hipEventDestroy(main_point);
    if (ext_point) (void)hipEventDestroy(ext_point);
    if (rel_point) (void)hipEventDestroy(rel_point);
    if (stream && own_stream) (void)hipStreamDestroy(stream);
  }
  // `stream` waits for what the group streams hold
  void join_groups() {
    for (int g = 1; g < groups; ++g) HIP_OK(hipStreamWaitEvent(stream, gdone[g], 0));
    groups_ahead = false;
  }

  std::pair<hipEvent_t, hipEvent_t>& next_events() {
    const size_t slot = events_used++ % kEventRing;
    if (slot == events.size()) {
      hipEvent_t a, b;
      HIP_OK(hipEventCreate(&a));
      HIP_OK(hipEventCreate(&b));
      events.emplace_back(a, b);
    }
    return events[slot];
  }

  void use_device() {
    HIP_OK(hipSetDevice(device));
    if (est_pending && !in_step && !in_flush) flush_pending_observation();
    if (groups > 1 && !in_step) {  // anything but a transition launch: ordered after every group, and the groups after it
      if (groups_ahead) join_groups();
      main_moved = true;
    }
  }
  void flush_pending_observation();

  // host [C][D] -> [C][Dp] on the host; padding columns hold pad_value
  std::vector<double> padded_rows(const double* host, double pad_value) const {
    std::vector<double> padded(C * static_cast<size_t>(Dp), pad_value);
    for (size_t c = 0; c < C; ++c) std::memcpy(&padded[c * Dp], host + c * D, sizeof(double) * D);
    return padded;
  }
  void upload_rows(DevBuf<double>& dst, const double* host, double pad_value) {
    // host [C][D] -> device [C][Dp]; padding columns keep their fill value
    use_device();
    if (Dp != D) {
      const std::vector<double> padded = padded_rows(host, pad_value);
      HIP_OK(hipMemcpyAsync(dst.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, stream));
      HIP_OK(hipStreamSynchronize(stream));
    } else {
      HIP_OK(hipMemcpyAsync(dst.p, host, C * static_cast<size_t>(D) * sizeof(double), hipMemcpyHostToDevice, stream));
      HIP_OK(hipStreamSynchronize(stream));
    }
  }
  void download_rows(const DevBuf<double>& src, double* host) {
    use_device();
    HIP_OK(hipMemcpy2DAsync(host, sizeof(double) * D, src.p, sizeof(double) * Dp, sizeof(double) * D, C,
                            hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
  }
  template <class T>
  void download(const DevBuf<T>& src, T* host, size_t count) {
    use_device();
    HIP_OK(hipMemcpyAsync(host, src.p, count * sizeof(T), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
  }
  void fill(DevBuf<double>& b, double v);  // (wn_engine_elementwise.hip)
  // throws if any transition of any chain SINCE THE PREVIOUS CHECK reported a device-side error: the kernels OR their
  // error bits into one word, which is read and cleared here (a caller that supplied too few variates, or hit a pool
  // limit, can correct that and carry on; the draws of the failed transitions are not valid)
  void check_transitions() {
    use_device();
    uint32_t flags = 0;
    HIP_OK(hipMemcpyAsync(&flags, error_flags.p, sizeof(flags), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemsetAsync(error_flags.p, 0, sizeof(uint32_t), stream));
    HIP_OK(hipStreamSynchronize(stream));
    if (flags & wn::kErrPoolExhausted)
      throw std::runtime_error("a chain exhausted the span pool: its draws are not valid (lower max_trajectory_doublings)");
    if (flags & wn::kErrVariatesExhausted)
      throw std::runtime_error("a transition consumed more host-fed uniforms than wn_engine_set_variates supplied");
  }

  void ensure_adapters();  // (wn_engine_elementwise.hip)
  void alloc_monitors();   // (wn_engine_elementwise.hip) mon_runs, mon_sums, mon_out for num_datasets segments

  // (wn_engine.hip, like everything below)
  wn::Params make_params(bool warm, double* draws_dev, int64_t draws_stride, int fused = 1, int64_t draws_tstride = 0);

  void feed_reference_streams();
  void advance_reference_streams();

  // One launch = `fused` transitions of every chain, back to back on the workgroup that fetched the chain (the chain's
  // k-th draw row at draws_dev + chain * draws_stride + k * draws_tstride).  Host-fed variates cover one transition.
  void step(bool warm, double* draws_dev, int64_t draws_stride, int fused = 1, int64_t draws_tstride = 0,
            bool flush_only = false);
};

// ---- the row passes over the observation block (wn_engine_pointwise.hip, wn_engine_predict.hip) ----------------------
// block g of the engine's rows: where its data rows start, how many there are, and where its outputs start
struct RowBlock {
  int64_t row0, out0;
  int32_t rows;
};
inline RowBlock row_block(const wn_engine* e, const std::vector<int64_t>& offsets, int g) {
  if (!offsets.empty()) return RowBlock{offsets[g], offsets[g], static_cast<int32_t>(offsets[g + 1] - offsets[g])};
  return RowBlock{0, static_cast<int64_t>(g) * e->obs.num_obs, e->obs.num_obs};  // one block, or weight set g of it
}
inline std::vector<int64_t> host_offsets(wn_engine* e) {
  std::vector<int64_t> off;
  if (e->obs.offsets != nullptr) {
    off.resize(static_cast<size_t>(e->num_datasets) + 1);
    HIP_OK(hipMemcpyAsync(off.data(), e->data_offsets.p, off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  }
  return off;
}
// work items -> workgroups: one each up to a cap (the kernel strides beyond it; any grid gives the same bits)
inline int pointwise_grid(int64_t items) {
  int64_t cap = int64_t{1} << 20;
  if (const char* v = std::getenv("WALNUTS_AMD_POINTWISE_GRID")) cap = std::max<int64_t>(1, std::atoll(v));
  return static_cast<int>(std::max<int64_t>(1, std::min(items, cap)));
}
// bytes of the per-chain partials a fold keeps at a time (one SLAB of chains; the merge carries its state across slabs)
inline size_t pointwise_workspace_bytes() {
  size_t budget = size_t{256} << 20;
  if (const char* v = std::getenv("WALNUTS_AMD_POINTWISE_WORKSPACE")) budget = static_cast<size_t>(std::max(1ll, std::atoll(v)));
  return budget;
}

#endif  // WN_ENGINE_H
