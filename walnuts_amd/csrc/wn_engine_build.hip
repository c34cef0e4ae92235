// wn_engine_build.hip -- building an engine (wn_engine_create, wn_engine_create_observed): the checks of what the
// caller handed in, the launch geometry and residency, the buffers, and the upload of the model's parameters and
// observations.  build_engine() is the order of those steps; each step names what it reads.  Beside it the queries that
// answer ahead of time what build_engine will pick: the default configuration, the geometries, the model registry.
#include "wn_engine.h"

#include "wn_traj.h"

namespace {

void check_config(const wn_config& cfg) {
  if (cfg.max_trajectory_doublings < 1) throw std::invalid_argument("max_nuts_depth must be positive");
  if (cfg.max_trajectory_doublings > wn::kMaxLevels + 1)
    throw std::invalid_argument("max_trajectory_doublings exceeds the device span stack");
  if (cfg.max_step_halvings < 1) throw std::invalid_argument("max_step_halvings must be positive");
  if (cfg.min_micro_steps < 1) throw std::invalid_argument("min_micro_steps must be positive");
  if (!(cfg.max_hamiltonian_error > 0) || !std::isfinite(cfg.max_hamiltonian_error))
    throw std::invalid_argument("max_hamiltonian_error must be positive and finite");
}

// what the model declares it reads (wn_model_api.h) against what it was given
void check_model_inputs(const wn::ModelOps& ops, int num_params, const double* model_params, const wn_observations* data) {
  if (ops.uses_params && model_params == nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model needs a parameter vector of num_params doubles");
  ops.validate(num_params);
  if (ops.uses_data && data == nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model is conditioned on data: create it with "
                                "wn_engine_create_observed (x [num_obs][" +
                                std::string(ops.scale_param ? "num_params - 1" : "num_params") + "], y [num_obs])");
  if (!ops.uses_data && data != nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model reads no data (it does not declare kUsesData)");
  if (ops.uses_groups && data != nullptr && data->group == nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model reads a group per observation: create it with "
                                "wn_engine_create_observed (x [num_obs][num_params - " +
                                std::string(ops.scale_param && ops.host_params_varying != nullptr
                                                ? "num_varying * (num_groups + 1) - 1"
                                                : ops.scale_param ? "num_groups - 2" : "num_groups - 1") +
                                "], y, group [num_obs] in [0, num_groups))");
  if (!ops.uses_groups && data != nullptr && data->group != nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model reads no groups (it does not declare kUsesGroups)");
  if (ops.host_params_varying == nullptr && data != nullptr && data->num_varying > 1)
    throw std::invalid_argument(std::string(ops.name) + " model has no varying slopes (it does not declare kVaryingSlopes): "
                                "num_varying must be 0 or 1, got " + std::to_string(data->num_varying));
  if (!ops.uses_row_terms && data != nullptr && (data->offset != nullptr || data->weight != nullptr))
    throw std::invalid_argument(std::string(ops.name) + " model reads no offsets or weights (it does not declare "
                                "kUsesRowTerms)");
}

// The shape of a checked observation block, as the upload and the monitors need it (all defaults without data)
struct ObservationPlan {
  int cols = 0;          // columns of x: num_params, num_params - 1 for a model with a scale parameter, or
                         // P = num_params - Q (J + 1) for a grouped model (less 1 with a scale parameter as well)
  int num_varying = 0;   // Q of a grouped model: coefficients that vary by group (1 without kVaryingSlopes)
  size_t total_obs = 0;  // rows of the observation block
  int weight_sets = 1;   // W weight vectors over the one shared block, an engine of W datasets above the kernels
  bool weighted = false;
  int num_datasets = 1;  // the engine's segments of chains: datasets one after another, or weight sets
  int chains_per_dataset = 0;  // (0: neither obs_offsets nor weight sets, every chain reads the one block)
};

// every value of the block: finite x, y, offsets; groups in range; weights finite and >= 0
void check_observation_values(const wn_observations& d, const ObservationPlan& plan) {
  const size_t total_obs = plan.total_obs;
  if (d.x == nullptr || d.y == nullptr) throw std::invalid_argument("null data argument");
  const size_t n = total_obs * static_cast<size_t>(plan.cols);
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(d.x[i])) throw std::invalid_argument("data x must be finite");
  for (size_t i = 0; i < total_obs; ++i)
    if (!std::isfinite(d.y[i])) throw std::invalid_argument("data y must be finite");
  if (d.group != nullptr)
    for (size_t i = 0; i < total_obs; ++i)
      if (d.group[i] < 0 || d.group[i] >= d.num_groups)
        throw std::invalid_argument("every group must be in [0, num_groups), observation " + std::to_string(i) + " has " +
                                    std::to_string(d.group[i]));
  if (d.offset != nullptr)
    for (size_t i = 0; i < total_obs; ++i)
      if (!std::isfinite(d.offset[i]))
        throw std::invalid_argument("every offset must be finite, observation " + std::to_string(i) + " has " +
                                    std::to_string(d.offset[i]));
  if (plan.weighted) {
    const size_t nw = total_obs * static_cast<size_t>(plan.weight_sets);
    for (size_t i = 0; i < nw; ++i)
      if (!(d.weight[i] >= 0.0) || !std::isfinite(d.weight[i]))
        throw std::invalid_argument("every weight must be finite and >= 0, observation " + std::to_string(i % total_obs) +
                                    (plan.weight_sets > 1 ? " of weight set " + std::to_string(i / total_obs) : std::string()) +
                                    " has " + std::to_string(d.weight[i]));
  }
}

// the model's own look at its data (ModelOps::host_data), dataset by dataset
void check_with_model(const wn::ModelOps& ops, const wn_observations& d, const ObservationPlan& plan) {
  if (d.obs_offsets == nullptr) {
    ops.host_data(d.x, d.y, d.num_obs, plan.cols, plan.weighted);
    return;
  }
  for (int g = 0; g < d.num_datasets; ++g) {
    const int64_t first = d.obs_offsets[g];
    try {
      ops.host_data(d.x + static_cast<size_t>(first) * plan.cols, d.y + first,
                    static_cast<int>(d.obs_offsets[g + 1] - first), plan.cols, plan.weighted);
    } catch (const std::invalid_argument& ex) {
      throw std::invalid_argument("dataset " + std::to_string(g) + ": " + ex.what());
    }
  }
}

// Host only: checks the observations (the first failing check gives the message) and returns their shape
ObservationPlan plan_observations(const wn::ModelOps& ops, int num_params, size_t num_chains, const wn_observations* data) {
  ObservationPlan plan;
  plan.cols = ops.scale_param ? num_params - 1 : num_params;
  if (data == nullptr) return plan;
  plan.weight_sets = data->num_weight_sets > 1 ? data->num_weight_sets : 1;
  if (data->num_weight_sets < 0) throw std::invalid_argument("num_weight_sets must not be negative");
  if (plan.weight_sets > 1 && data->weight == nullptr)
    throw std::invalid_argument("num_weight_sets > 1 needs weight [num_weight_sets][num_obs]");
  if (plan.weight_sets > 1 && data->obs_offsets != nullptr)
    throw std::invalid_argument("weight sets share one block of rows: not with obs_offsets (several datasets)");
  if (plan.weight_sets > 1 && num_chains % static_cast<size_t>(plan.weight_sets) != 0)
    throw std::invalid_argument("num_chains must be a multiple of num_weight_sets (chain c reads weight set c / "
                                "(num_chains / num_weight_sets))");
  plan.weighted = data->weight != nullptr;
  if (ops.uses_groups && ops.host_params_varying != nullptr) {
    // varying slopes: Q coefficients vary by group, 0 meaning 1 (the intercept only)
    // (with a scale parameter theta ends with one more log scale, the family's: models/hier_slopes_scale_glm.h)
    const int J = data->num_groups, Q = data->num_varying == 0 ? 1 : data->num_varying;
    const long long P = static_cast<long long>(num_params) - static_cast<long long>(Q) * (static_cast<long long>(J) + 1) -
                        (ops.scale_param ? 1 : 0);
    if (Q < 1 || Q > wn::kMaxVaryingCoefficients)
      throw std::invalid_argument("a model with varying slopes needs 1 <= num_varying <= " +
                                  std::to_string(wn::kMaxVaryingCoefficients) + ", got " + std::to_string(data->num_varying));
    if (J < 1 || P < 1)
      throw std::invalid_argument("a model with varying slopes needs num_params == P + num_varying * (num_groups + 1) " +
                                  std::string(ops.scale_param ? "+ 1 " : "") +
                                  "with P >= 1 and num_groups >= 1, got num_params " + std::to_string(num_params) +
                                  ", num_groups " + std::to_string(J) + ", num_varying " + std::to_string(Q));
    if (Q - 1 > P)
      throw std::invalid_argument("the varying slopes belong to the first num_varying - 1 columns of x: num_varying - 1 <= P, "
                                  "got num_varying " + std::to_string(Q) + ", P " + std::to_string(P));
    plan.cols = static_cast<int>(P);
    plan.num_varying = Q;
  } else if (ops.uses_groups && ops.scale_param) {
    // theta ends with two log scales: the group scale and the family's (models/hier_scale_glm.h)
    const int J = data->num_groups;
    const long long P = static_cast<long long>(num_params) - J - 2;
    if (J < 1 || P < 1)
      throw std::invalid_argument("a grouped model with a scale parameter needs num_params == P + num_groups + 2 with P >= 1 "
                                  "and num_groups >= 1, got num_params " + std::to_string(num_params) + ", num_groups " +
                                  std::to_string(J));
    plan.cols = static_cast<int>(P);
    plan.num_varying = 1;
  } else if (ops.uses_groups) {
    const int J = data->num_groups;
    if (J < 1 || num_params - J - 1 < 1)
      throw std::invalid_argument("a grouped model needs num_params == P + num_groups + 1 with P >= 1 and num_groups >= 1, "
                                  "got num_params " + std::to_string(num_params) + ", num_groups " + std::to_string(J));
    plan.cols = num_params - J - 1;
    plan.num_varying = 1;
  }
  if (data->obs_offsets != nullptr) {
    const int G = data->num_datasets;
    if (G < 1) throw std::invalid_argument("num_datasets must be positive");
    if (num_chains % static_cast<size_t>(G) != 0)
      throw std::invalid_argument("num_chains must be a multiple of num_datasets (chain c reads dataset c / (num_chains / "
                                  "num_datasets))");
    if (data->obs_offsets[0] != 0) throw std::invalid_argument("obs_offsets must start at 0");
    for (int g = 0; g < G; ++g) {
      const int64_t n = data->obs_offsets[g + 1] - data->obs_offsets[g];
      if (n < 1)
        throw std::invalid_argument("obs_offsets must be strictly increasing (every dataset needs at least one observation)");
      if (n > INT32_MAX) throw std::invalid_argument("a dataset holds more than 2^31 - 1 observations");
    }
    plan.total_obs = static_cast<size_t>(data->obs_offsets[G]);
    plan.num_datasets = G;
    plan.chains_per_dataset = static_cast<int>(num_chains / static_cast<size_t>(G));
  } else {
    if (data->num_obs < 1) throw std::invalid_argument("num_obs must be positive");
    plan.total_obs = static_cast<size_t>(data->num_obs);
    plan.num_datasets = plan.weight_sets;
    if (plan.weight_sets > 1) plan.chains_per_dataset = static_cast<int>(num_chains / static_cast<size_t>(plan.weight_sets));
  }
  check_observation_values(*data, plan);
  check_with_model(ops, *data, plan);
  return plan;
}

// the device, its size and the engine's stream
void open_device(wn_engine& e) {
  e.use_device();
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, e.device));
  e.num_cus = prop.multiProcessorCount;
  HIP_OK(hipStreamCreateWithFlags(&e.stream, hipStreamNonBlocking));
}

int required_pool(const wn_config& c) {
  // other end of the accumulated span 3 + its selection 1, one entry (<= 3 vectors) per stack level
  // 1..max_depth-2, the span under construction 3, the parked state of a reversibility check 3, slack
  const int levels = std::max(1, c.max_trajectory_doublings - 1);
  return 4 + 3 * levels + 3 + 3 + 2;
}

// residency: how many chains (workgroups) share a CU, and how much of the span pool sits in LDS -> workgroups per CU
int plan_residency(wn_engine& e, const wn::ModelOps& ops, const wn_config& cfg) {
  const int num_params = e.D;
  const size_t lds_per_cu = 160 * 1024;
  e.pool_total = required_pool(cfg) + (e.geo.mem ? wn::kMemRoleVectors : 0);
  if (e.pool_total > wn::kMaxPool)
    throw std::invalid_argument("max_trajectory_doublings needs more span-pool vectors than the device free mask holds");
  const int wps = wn::waves_per_simd(e.model, e.geo);
  const int hold_tiles = e.geo.mem ? ops.hold_tiles(e.geo.nw) : 0;
  const bool hold_fits = hold_tiles > 0 && num_params <= 2 * 64 * e.geo.nw * hold_tiles;
  const size_t vec_bytes = sizeof(double) * e.Dp;
  int wg_per_cu = 0;
  // residency for `want` workgroups per CU (0: the default for this geometry) -> whether the moving end is held
  auto residency = [&](int want) {
    wg_per_cu = want > 0 ? want : wn::default_workgroups_per_cu(e.geo, wps);
    wg_per_cu = std::max(1, std::min(wg_per_cu, 32 / e.geo.nw));
    if (!e.geo.mem) wg_per_cu = std::min(wg_per_cu, std::max(1, 4 * wps / e.geo.nw));
    const size_t fixed = wn::transition_smem_bytes(e.geo.nw, 0, e.Dp);
    const size_t budget = lds_per_cu / wg_per_cu;
    if (fixed > budget) throw std::invalid_argument("workgroups_per_cu too high for the LDS-resident state");
    int lds_vecs = budget > fixed + 256 ? static_cast<int>((budget - fixed - 256) / vec_bytes) : 0;
    if (cfg.lds_vectors >= 0 && cfg.lds_vectors < lds_vecs) lds_vecs = cfg.lds_vectors;
    if (e.geo.mem) lds_vecs = 0;  // streaming backend: vectors are far larger than LDS
    e.pool_lds = std::min(lds_vecs, e.pool_total);
    e.smem = wn::transition_smem_bytes(e.geo.nw, e.pool_lds, e.Dp);
    e.im_in_lds = false;
    e.hold_moving_end = false;
    if (e.geo.mem) {
      // one more vector per workgroup, if the CU's LDS holds it for every resident workgroup: the inverse mass
      const char* off = std::getenv("WALNUTS_AMD_NO_LDS_MASS");
      const char* nf = std::getenv("WALNUTS_AMD_NO_FAR_END_SUMS");
      e.no_far_end_sums = nf != nullptr && nf[0] == '1';
      if (e.smem + vec_bytes <= budget && !(off != nullptr && off[0] == '1')) {
        e.im_in_lds = true;
        e.smem += vec_bytes;
        // ... and, if the chain's vectors fit the registers the kernels set aside for it, the moving end (TrajMem, HOLD)
        const char* nh = std::getenv("WALNUTS_AMD_NO_HELD_STATE");
        // (such a kernel keeps the exp / log tables in LDS too, and a halo model's wavefront-edge elements)
        const size_t tables = sizeof(double) * (wn::kLdsTableDoubles + 2 * 2 * wn::kMemHoldTiles * e.geo.nw);  // (two copies of the edges)
        e.hold_moving_end = hold_fits && e.smem + tables <= budget && !(nh != nullptr && nh[0] == '1');
        if (e.hold_moving_end) e.smem += tables;
      }
    }
    return e.hold_moving_end;
  };
  if (cfg.workgroups_per_cu > 0) {
    residency(cfg.workgroups_per_cu);
  } else if (hold_fits) {
    // a streaming kernel that can hold the moving end in registers wants the CU -- its LDS for the inverse mass, a
    // wavefront's full register budget -- for ONE chain; if the hold is then refused (no room for the inverse mass
    // and the tables, or switched off), the kernel that streams both ends gets its usual residency back
    if (!residency(1)) residency(0);
  } else {
    residency(0);
  }
  return wg_per_cu;
}

// every chain's planes and vectors
void allocate_chain_state(wn_engine& e) {
  const size_t num_chains = e.C;
  const size_t plane = num_chains * static_cast<size_t>(e.Dp);
  for (DevBuf<double>* b : {&e.theta, &e.mass, &e.inv_mass, &e.chol_mass, &e.draw_mean, &e.draw_ssd, &e.score_mean, &e.score_ssd})
    b->alloc(plane);
  e.step_init.alloc(num_chains);
  e.step_size.alloc(num_chains);
  e.adam.alloc(6 * num_chains);
  e.est_weight.alloc(2 * num_chains);
  e.mm_state.alloc(2 * num_chains);
  e.logp.alloc(num_chains);
  e.min_micro.alloc(num_chains);
  e.depth.alloc(num_chains);
  e.rng_draws.alloc(num_chains);
  e.failed_ext.alloc(num_chains);
  e.grad_evals.alloc(num_chains);
}

// the launch grid, and the chain groups: as configured, or two when there are more chains than resident workgroups
// (with at most one chain per workgroup there is no tail to fill: 1024 and 256 chains measured the same with 1-4
// groups); host-fed variates and an adopted stream (wn_engine_set_stream) go back to one
void plan_chain_groups(wn_engine& e, const wn_config& cfg, int wg_per_cu) {
  const size_t num_chains = e.C;
  const int usable_cus = std::max(1, e.num_cus - std::max(0, cfg.reserved_cus));
  e.grid = static_cast<int>(std::min<size_t>(num_chains, static_cast<size_t>(usable_cus) * wg_per_cu));
  {
    int want = cfg.chain_groups;
    if (const char* v = std::getenv("WALNUTS_AMD_CHAIN_GROUPS")) want = std::atoi(v);
    // (... and one when a CU holds a single workgroup of this kernel -- the streaming kernels with the inverse mass in
    // LDS --: the second group's workgroups then start only as the first group's retire, i.e. two tails instead of one;
    // config #4 measured 15.3 ms per step with one group against 15.9 ms with two)
    if (want <= 0) want = (num_chains > static_cast<size_t>(e.grid) && !(e.geo.mem && wg_per_cu == 1)) ? 2 : 1;
    e.groups = std::max(1, std::min({want, wn_engine::kMaxGroups, static_cast<int>(num_chains)}));
  }
  for (int g = 0; g <= e.groups; ++g) e.group_begin[g] = num_chains * static_cast<size_t>(g) / static_cast<size_t>(e.groups);
  e.gstream[0] = e.stream;
  for (int g = 0; g < e.groups; ++g) {
    e.group_grid[g] = static_cast<int>(std::min<size_t>(e.group_begin[g + 1] - e.group_begin[g], static_cast<size_t>(e.grid)));
    if (g > 0) {
      HIP_OK(hipStreamCreateWithFlags(&e.gstream[g], hipStreamNonBlocking));
      HIP_OK(hipEventCreateWithFlags(&e.gdone[g], hipEventDisableTiming));
    }
  }
  if (e.groups > 1) HIP_OK(hipEventCreateWithFlags(&e.main_point, hipEventDisableTiming));
}

// what the launches share (one chain counter and arena slice per group), and every buffer's initial fill
void allocate_launch_state(wn_engine& e) {
  const size_t num_chains = e.C;
  const size_t plane = num_chains * static_cast<size_t>(e.Dp);
  e.counter.alloc(wn_engine::kMaxGroups);
  HIP_OK(hipMemsetAsync(e.counter.p, 0, wn_engine::kMaxGroups * sizeof(uint32_t), e.stream));
  e.error_flags.alloc(1);
  HIP_OK(hipMemsetAsync(e.error_flags.p, 0, sizeof(uint32_t), e.stream));
  e.lp_stats.alloc(3 * num_chains);
  e.mon_rel_mass.alloc(num_chains);
  e.mon_rel_step.alloc(num_chains);
  e.scratch64.alloc(1);
  // what LDS does not hold (deep trees only) overflows to a per-workgroup HBM arena
  const size_t arena_vecs = static_cast<size_t>(std::max(0, e.pool_total - e.pool_lds)) +
                            (e.geo.mem ? wn::kMemScratchVectors : 0);
  e.arena_stride = static_cast<int64_t>(arena_vecs) * e.Dp;
  e.arena.alloc(std::max<size_t>(1, static_cast<size_t>(e.groups) * static_cast<size_t>(e.grid) * arena_vecs * e.Dp));
  e.model_params.alloc(e.Dp);

  // InitConfigBuilder defaults (config.hpp:197-207): step 0.1, positions 0, masses 1
  HIP_OK(hipMemsetAsync(e.theta.p, 0, plane * sizeof(double), e.stream));
  e.fill(e.mass, 1.0);
  e.fill(e.inv_mass, 1.0);
  e.fill(e.step_init, 0.1);
  HIP_OK(hipMemsetAsync(e.grad_evals.p, 0, num_chains * sizeof(int64_t), e.stream));
  HIP_OK(hipMemsetAsync(e.depth.p, 0, num_chains * sizeof(int32_t), e.stream));
  HIP_OK(hipMemsetAsync(e.rng_draws.p, 0, num_chains * sizeof(int32_t), e.stream));
  HIP_OK(hipMemsetAsync(e.failed_ext.p, 0, num_chains * sizeof(int32_t), e.stream));
  HIP_OK(hipMemsetAsync(e.logp.p, 0, num_chains * sizeof(double), e.stream));
  HIP_OK(hipMemsetAsync(e.lp_stats.p, 0, 3 * num_chains * sizeof(double), e.stream));
}

void upload_model_params(wn_engine& e, const wn::ModelOps& ops, const double* model_params, const ObservationPlan& plan) {
  const int num_params = e.D;
  std::vector<double> mp(e.Dp, 1.0);
  if (model_params) std::copy(model_params, model_params + num_params, mp.begin());
  // the model's own validation / transformation (wn_models.h); with varying slopes it is told Q
  if (ops.host_params_varying != nullptr)
    ops.host_params_varying(mp.data(), num_params, plan.num_varying);
  else
    ops.host_params(mp.data(), num_params);
  HIP_OK(hipMemcpyAsync(e.model_params.p, mp.data(), mp.size() * sizeof(double), hipMemcpyHostToDevice, e.stream));
  HIP_OK(hipStreamSynchronize(e.stream));
}

// x [rows][obs.stride] (rows padded with zeros), y, the row constants, groups, offsets, weights and dataset offsets
void upload_observations(wn_engine& e, const wn::ModelOps& ops, const wn_observations* data, const ObservationPlan& plan) {
  const int cols = plan.cols;
  // rows padded with zeros to the stride Dx: Dp, the layout of a theta row (lane tid's slot j holds coordinate index(j));
  // for a grouped model 128 * ceil(P / 128), the slot pairs of theta that hold x's P columns
  e.obs.stride = ops.uses_groups ? 128 * ((cols + 127) / 128) : e.Dp;
  if (data == nullptr) return;
  // the padded copy goes up in slices of at most 64 MiB (a block of many datasets may be larger than what is
  // sensible to double in host memory)
  const size_t N = plan.total_obs, Dx = static_cast<size_t>(e.obs.stride);
  e.data_x.alloc(N * Dx);
  e.data_y.alloc(N);
  const size_t slice = std::max<size_t>(1, (size_t{64} << 20) / (Dx * sizeof(double)));
  std::vector<double> xp(std::min(N, slice) * Dx, 0.0);
  for (size_t n0 = 0; n0 < N; n0 += slice) {
    const size_t rows = std::min(slice, N - n0);
    for (size_t n = 0; n < rows; ++n)
      std::memcpy(&xp[n * Dx], data->x + (n0 + n) * cols, sizeof(double) * cols);
    HIP_OK(hipMemcpyAsync(e.data_x.p + n0 * Dx, xp.data(), rows * Dx * sizeof(double), hipMemcpyHostToDevice, e.stream));
    HIP_OK(hipStreamSynchronize(e.stream));  // (before the staging slice is refilled)
  }
  HIP_OK(hipMemcpyAsync(e.data_y.p, data->y, N * sizeof(double), hipMemcpyHostToDevice, e.stream));
  e.obs.x = e.data_x.p;
  e.obs.y = e.data_y.p;
  e.data_rows = N;
  if (ops.pointwise != nullptr) {
    std::vector<double> cn(N);
    ops.pointwise->row_consts(data->y, N, cn.data());
    e.data_const.alloc(N);
    HIP_OK(hipMemcpyAsync(e.data_const.p, cn.data(), N * sizeof(double), hipMemcpyHostToDevice, e.stream));
    HIP_OK(hipStreamSynchronize(e.stream));  // (before the staging vector goes)
  }
  if (data->group != nullptr) {
    e.data_group.alloc(N);
    HIP_OK(hipMemcpyAsync(e.data_group.p, data->group, N * sizeof(int32_t), hipMemcpyHostToDevice, e.stream));
    e.obs.group = e.data_group.p;
    e.obs.num_groups = data->num_groups;
    e.obs.num_varying = plan.num_varying;
  }
  if (data->offset != nullptr) {
    e.data_offset.alloc(N);
    HIP_OK(hipMemcpyAsync(e.data_offset.p, data->offset, N * sizeof(double), hipMemcpyHostToDevice, e.stream));
    e.obs.offset = e.data_offset.p;
  }
  if (plan.weighted) {
    const size_t nw = N * static_cast<size_t>(plan.weight_sets);
    e.data_weight.alloc(nw);
    HIP_OK(hipMemcpyAsync(e.data_weight.p, data->weight, nw * sizeof(double), hipMemcpyHostToDevice, e.stream));
    e.obs.weight = e.data_weight.p;
  }
  e.obs.chains_per_dataset = plan.chains_per_dataset;
  if (plan.weight_sets > 1) {
    // the rows are shared and the kernels take set c / k of the weights (bind_data: chains_per_dataset > 0 without
    // an offsets array); above the kernels the sets are the engine's datasets
    e.obs.num_obs = data->num_obs;
  } else if (data->obs_offsets != nullptr) {
    // the datasets one after another; the kernels take every chain's row count from the offsets (obs.num_obs = 0)
    const size_t G = static_cast<size_t>(plan.num_datasets);
    e.data_offsets.alloc(G + 1);
    HIP_OK(hipMemcpyAsync(e.data_offsets.p, data->obs_offsets, (G + 1) * sizeof(int64_t), hipMemcpyHostToDevice, e.stream));
    e.obs.offsets = e.data_offsets.p;
  } else {
    e.obs.num_obs = data->num_obs;
  }
  HIP_OK(hipStreamSynchronize(e.stream));
}

void build_engine(wn_engine& e, int model, int num_params, const double* model_params, size_t num_chains,
                  const wn_config& cfg, const wn_observations* data = nullptr) {
  if (num_params < 1) throw std::invalid_argument("num_params must be positive");
  if (num_chains < 1) throw std::invalid_argument("num_chains must be positive");
  if (!wn::registry_error().empty()) throw std::invalid_argument(wn::registry_error());
  const wn::ModelOps& ops = wn::model_ops(model);  // throws for an id no model registered
  check_config(cfg);
  check_model_inputs(ops, num_params, model_params, data);
  const ObservationPlan plan = plan_observations(ops, num_params, num_chains, data);

  e.model = model;
  e.D = num_params;
  e.C = num_chains;
  e.cfg = cfg;
  e.device = cfg.device;
  e.num_datasets = plan.num_datasets;
  e.geo = wn::choose_geometry(num_params, cfg.waves_per_chain, cfg.elems_per_lane, ops.uses_params, ops.preferred_epl(num_params),
                              ops.hold_tiles(wn::kHeldWaves), ops.register_dim_limit);
  e.Dp = wn::padded_dim(e.geo, num_params);
  if (ops.uses_data && (e.geo.mem || e.geo.nw != 1))
    throw std::invalid_argument(std::string(ops.name) + ": a data model runs one wavefront per chain (num_params <= 1024, "
                                "waves_per_chain 0 or 1, elems_per_lane 0, 2, 4, 8 or 16)");
  open_device(e);
  const int wg_per_cu = plan_residency(e, ops, cfg);
  allocate_chain_state(e);
  plan_chain_groups(e, cfg, wg_per_cu);  // (before the arena, which has a slice per group)
  allocate_launch_state(e);
  upload_model_params(e, ops, model_params, plan);
  upload_observations(e, ops, data, plan);
  e.alloc_monitors();
  wn::prepare_kernels(model, e.geo, e.smem);
}

}  // namespace

extern "C" {

int wn_model_data_columns(int model, int num_params, int num_groups) {
  if (model < 0 || model >= wn::kMaxModels) return -1;
  const wn::ModelOps* ops = wn::model_table()[model];
  if (ops == nullptr || !ops->uses_data) return -1;
  if (ops->uses_groups) return num_groups >= 1 ? num_params - num_groups - (ops->scale_param ? 2 : 1) : -1;
  return ops->scale_param ? num_params - 1 : num_params;
}

int wn_model_num_scale_params(int model) {
  if (model < 0 || model >= wn::kMaxModels) return -1;
  const wn::ModelOps* ops = wn::model_table()[model];
  if (ops == nullptr) return -1;
  return ops->scale_param ? 1 : 0;
}

int wn_model_data_columns_varying(int model, int num_params, int num_groups, int num_varying) {
  if (model < 0 || model >= wn::kMaxModels) return -1;
  const wn::ModelOps* ops = wn::model_table()[model];
  if (ops == nullptr || !ops->uses_data) return -1;
  if (ops->host_params_varying == nullptr) return num_varying > 1 ? -1 : wn_model_data_columns(model, num_params, num_groups);
  const int Q = num_varying == 0 ? 1 : num_varying;
  if (Q < 1 || Q > wn::kMaxVaryingCoefficients || num_groups < 1) return -1;
  const long long P = static_cast<long long>(num_params) - static_cast<long long>(Q) * (static_cast<long long>(num_groups) + 1) -
                      (ops->scale_param ? 1 : 0);
  return P >= 1 && Q - 1 <= P ? static_cast<int>(P) : -1;
}

int wn_model_id(const char* name) {
  if (name == nullptr) return -1;
  for (int i = 0; i < wn::kMaxModels; ++i) {
    const wn::ModelOps* ops = wn::model_table()[i];
    if (ops != nullptr && std::strcmp(ops->name, name) == 0) return i;
  }
  return -1;
}

// ---- device models compiled at run time (walnuts_amd/models.py; INTEGRATION.md "Adding a device model") --------------
// the registration of a model's own shared object, called from its static initialiser when it is loaded
int wn_plugin_register_model(const void* ops, const void* abi) {
  const auto* theirs = static_cast<const wn::ModelAbi*>(abi);
  const wn::ModelAbi ours = wn::model_abi();
  const auto* m = static_cast<const wn::ModelOps*>(ops);
  if (theirs == nullptr || m == nullptr || theirs->version != ours.version || theirs->sizeof_ops != ours.sizeof_ops ||
      theirs->sizeof_params != ours.sizeof_params || theirs->sizeof_geometry != ours.sizeof_geometry) {
    wn::registry_error() = "a device model was compiled against other headers than this library (wn_launch.h "
                           "kModelAbiVersion / struct sizes differ): rebuild it with walnuts_amd.build_device_model";
    return -1;
  }
  return wn::register_model_here(m) ? 0 : -1;
}
// what went wrong in the last registration ("" if nothing has); the message stays until the next failure
const char* wn_model_error(void) { return wn::registry_error().c_str(); }
// forget a failed registration (a run-time model whose id was taken is reported once, not by every later engine)
void wn_model_clear_error(void) { wn::registry_error().clear(); }
// Launch geometries.  The engine's choice depends on the MODEL as well as on num_params and the wn_config's requests:
// a model with held streaming kernels (ModelOps::hold_tiles) leaves the register kernels at its register_dim_limit.
// wn_geometry_for_model: the ONE geometry build_engine picks for a REGISTERED model (the same choose_geometry call).
int wn_geometry_for_model(int model, int num_params, int waves_per_chain, int elems_per_lane, int* nw, int* epl,
                          int* streaming, WalnutpyError** err) {
  return guarded(err, [&] {
    if (num_params < 1) throw std::invalid_argument("num_params must be positive");
    const wn::ModelOps& ops = wn::model_ops(model);
    const wn::Geometry g = wn::choose_geometry(num_params, waves_per_chain, elems_per_lane, ops.uses_params, ops.preferred_epl(num_params),
                                               ops.hold_tiles(wn::kHeldWaves), ops.register_dim_limit);
    if (nw != nullptr) *nw = g.nw;
    if (epl != nullptr) *epl = g.epl;
    if (streaming != nullptr) *streaming = g.mem ? 1 : 0;
  });
}
// wn_geometry_candidates: EVERY geometry build_engine may pick for these requests, over all traits a model can have
// (no held streaming kernels; held kernels with the register kernels up to 4 096 or up to 8 192 parameters) -- what a
// model that is compiled at run time, and therefore not registered yet, has to instantiate.  out: triples
// (waves per chain, elements per lane, streaming), at most `max` of them; *count = how many there are.
int wn_geometry_candidates(int num_params, int waves_per_chain, int elems_per_lane, int preferred_elems_per_lane,
                           int* out, int max, int* count, WalnutpyError** err) {
  return guarded(err, [&] {
    if (num_params < 1) throw std::invalid_argument("num_params must be positive");
    if (count == nullptr) throw std::invalid_argument("null argument");
    const int traits[3][2] = {{0, wn::kMaxRegisterDim}, {wn::kMemHoldTiles, 4096}, {wn::kMemHoldTiles, 8192}};
    int n = 0;
    wn::Geometry seen[3];
    for (const auto& t : traits) {
      const wn::Geometry g = wn::choose_geometry(num_params, waves_per_chain, elems_per_lane, false,
                                                 preferred_elems_per_lane, t[0], t[1]);
      bool dup = false;
      for (int i = 0; i < n; ++i) dup = dup || (seen[i].nw == g.nw && seen[i].epl == g.epl && seen[i].mem == g.mem);
      if (dup) continue;
      seen[n] = g;
      if (out != nullptr && n < max) {
        out[3 * n] = g.nw;
        out[3 * n + 1] = g.epl;
        out[3 * n + 2] = g.mem ? 1 : 0;
      }
      ++n;
    }
    *count = n;
  });
}
// (kept: the choice for a model WITHOUT held streaming kernels and with the default register limit)
int wn_geometry_for(int num_params, int waves_per_chain, int elems_per_lane, int preferred_elems_per_lane, int* nw,
                    int* epl, int* streaming, WalnutpyError** err) {
  return guarded(err, [&] {
    if (num_params < 1) throw std::invalid_argument("num_params must be positive");
    const wn::Geometry g = wn::choose_geometry(num_params, waves_per_chain, elems_per_lane, false, preferred_elems_per_lane);
    if (nw != nullptr) *nw = g.nw;
    if (epl != nullptr) *epl = g.epl;
    if (streaming != nullptr) *streaming = g.mem ? 1 : 0;
  });
}

// WALNUTS_AMD_FMA=0/1 overrides the library default (fused) for callers that do not build a wn_config themselves
// (walnutpie_sample_device keeps the reference's argument list)
static int default_fma() {
  const char* v = std::getenv("WALNUTS_AMD_FMA");
  return (v != nullptr && v[0] == '0') ? 0 : 1;
}

void wn_default_config(wn_config* c) {
  c->max_trajectory_doublings = 5;
  c->max_step_halvings = 5;
  c->min_micro_steps = 1;
  c->device = 0;
  c->max_hamiltonian_error = 0.5;
  c->mass_init_count = 4.0;
  c->max_macro_steps_target = 15.0;
  c->step_accept_rate_target = 0.8;
  c->step_learning_rate = 0.05;
  c->step_gradient_decay = 0.8;
  c->step_sq_gradient_decay = 0.9;
  c->step_stabilization = 1e-4;
  c->step_learn_rate_decay = 0.5;
  c->waves_per_chain = 0;
  c->elems_per_lane = 0;
  c->workgroups_per_cu = 0;
  c->lds_vectors = -1;
  c->fused_multiply_add = default_fma();
  c->reserved_cus = 0;
  c->chain_groups = 0;
}

int wn_engine_create(wn_engine** out, int model, int num_params, const double* model_params, size_t num_chains,
                     const wn_config* cfg, WalnutpyError** err) {
  return guarded(err, [&] {
    if (out == nullptr || cfg == nullptr) throw std::invalid_argument("null argument");
    auto e = std::make_unique<wn_engine>();
    build_engine(*e, model, num_params, model_params, num_chains, *cfg);
    *out = e.release();
  });
}
int wn_engine_create_observed(wn_engine** out, int model, int num_params, const double* model_params,
                              const wn_observations* obs, size_t num_chains, const wn_config* cfg, WalnutpyError** err) {
  return guarded(err, [&] {
    if (out == nullptr || cfg == nullptr || obs == nullptr) throw std::invalid_argument("null argument");
    auto e = std::make_unique<wn_engine>();
    build_engine(*e, model, num_params, model_params, num_chains, *cfg, obs);
    *out = e.release();
  });
}

int wn_lanes_for_model_dim(int model, int num_params, int waves_per_chain, int elems_per_lane) {
  try {
    return 64 * wn::choose_geometry(num_params, waves_per_chain, elems_per_lane, wn::model_ops(model).uses_params,
                                    wn::model_ops(model).preferred_epl(num_params), wn::model_ops(model).hold_tiles(wn::kHeldWaves),
                                    wn::model_ops(model).register_dim_limit).nw;
  } catch (...) {
    return -1;
  }
}
int wn_lanes_for_dim(int num_params, int waves_per_chain, int elems_per_lane) {
  return wn_lanes_for_model_dim(WN_MODEL_STD_NORMAL, num_params, waves_per_chain, elems_per_lane);
}

}  // extern "C"
