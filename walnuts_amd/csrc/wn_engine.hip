// wn_engine.hip -- host side of the C ABI in include/walnuts_hip.h: drives the persistent transition kernel and the
// initialisation kernels over the engine's chain-major HBM planes (wn_engine.h), and holds the plain entry points:
// setters, getters, timing, streams.  The other units around the same state: wn_engine_build.hip (wn_engine_create*),
// wn_engine_elementwise.hip (adapter start / freeze, cross-chain monitors), wn_engine_pointwise.hip (pointwise scoring),
// wn_engine_predict.hip (predictions).
#include "wn_engine.h"

#include "wn_init.h"

wn::Params wn_engine::make_params(bool warm, double* draws_dev, int64_t draws_stride, int fused, int64_t draws_tstride) {
  wn::Params P{};
  P.num_chains = static_cast<int32_t>(C);
  P.dim = D;
  P.dim_padded = Dp;
  P.warmup = warm ? 1 : 0;
  P.theta = theta.p;
  P.inv_mass = inv_mass.p;
  P.chol_mass = chol_mass.p;
  P.est_draw_mean = draw_mean.p;
  P.est_draw_ssd = draw_ssd.p;
  P.est_score_mean = score_mean.p;
  P.est_score_ssd = score_ssd.p;
  P.step_size = step_size.p;
  P.min_micro = min_micro.p;
  P.adam = adam.p;
  P.est_weight = est_weight.p;
  P.mm_state = mm_state.p;
  P.logp_out = logp.p;
  P.depth_out = depth.p;
  P.grad_evals = grad_evals.p;
  P.rng_draws = rng_draws.p;
  P.failed_ext = failed_ext.p;
  P.lp_stats = lp_stats.p;
  P.draws_out = draws_dev;
  P.draws_stride = draws_stride;
  P.draws_tstride = draws_tstride;
  P.fused = fused;
  P.model_params = model_params.p;
  P.max_depth = cfg.max_trajectory_doublings;
  P.max_halvings = cfg.max_step_halvings;
  P.cfg_min_micro = cfg.min_micro_steps;
  P.fma = cfg.fused_multiply_add ? 1 : 0;
  P.max_error = cfg.max_hamiltonian_error;
  P.mass_init_count = cfg.mass_init_count;
  P.macro_target = cfg.max_macro_steps_target;
  P.adam_target = cfg.step_accept_rate_target;
  P.adam_lr = cfg.step_learning_rate;
  P.adam_b1 = cfg.step_gradient_decay;
  P.adam_b2 = cfg.step_sq_gradient_decay;
  P.adam_eps = cfg.step_stabilization;
  P.adam_decay = cfg.step_learn_rate_decay;
  P.seed = seed;
  P.chain_offset = chain_offset;
  P.transition = transition;
  P.rng_mode = variates_pending ? wn::kRngBuffer : wn::kRngPhilox;
  P.u_stride = u_stride;
  P.z_buf = z_buf.p;
  P.u_buf = u_buf.p;
  P.warmup_iter = warmup_iter;
  P.arena = arena.p;
  P.arena_stride = arena_stride;
  P.pool_lds = pool_lds;
  P.im_in_lds = (im_in_lds ? 1u : 0u) | (no_far_end_sums ? 2u : 0u) | (hold_moving_end ? 4u : 0u);
  P.pool_total = pool_total;
  P.est_mode = (warm && est_pending) ? 1 : 0;
  P.work_counter = counter.p;
  P.error_flags = error_flags.p;
  P.obs = obs;
  return P;
}

void wn_engine::step(bool warm, double* draws_dev, int64_t draws_stride, int fused, int64_t draws_tstride,
                     bool flush_only) {
  if (fused < 1) throw std::invalid_argument("transitions per launch must be at least 1");
  if (fused > 1 && (ref_streams || variates_pending))
    throw std::invalid_argument("host-fed variates cover one transition: transitions per launch must be 1");
  // (a sampling launch reads the frozen planes; freeze has applied a pending observation -- a caller that samples
  // without freezing gets it applied here)
  if (!flush_only && !warm && est_pending) flush_pending_observation();
  in_step = !ref_streams;  // (a transition launch does not make `stream` wait for the groups -- unless variates are
                           // fed from the host first, which writes buffers the groups' previous launches read)
  struct Leave {
    bool& flag;
    ~Leave() { flag = false; }
  } leave{in_step};
  use_device();
  if (ref_streams && !flush_only) feed_reference_streams();
  in_step = true;
  wn::Params P = make_params(warm, draws_dev, draws_stride, fused, draws_tstride);
  if (flush_only) P.est_mode = 2;
  if (groups > 1 && main_moved) {  // the group streams catch up with what `stream` did since their last launches
    HIP_OK(hipEventRecord(main_point, stream));
    for (int g = 1; g < groups; ++g) HIP_OK(hipStreamWaitEvent(gstream[g], main_point, 0));
    main_moved = false;
  }
  std::pair<hipEvent_t, hipEvent_t>* timed = (timing && !flush_only) ? &next_events() : nullptr;
  for (int g = 0; g < groups; ++g) {
    // The chain counter is never reset: every launch performs exactly as many fetches as it has chains (one per
    // processed chain), so a group's launch n starts at n * its chain count (mod 2^32) -- one memset per transition
    // less between two kernels.  (The first chain of the group is folded into the base: fetched = begin + ...)
    const uint32_t count = static_cast<uint32_t>(group_begin[g + 1] - group_begin[g]);
    P.chain_begin = static_cast<int32_t>(group_begin[g]);
    P.num_chains = static_cast<int32_t>(group_begin[g + 1]);
    P.work_counter = counter.p + g;
    P.work_base = work_base[g] - static_cast<uint32_t>(group_begin[g]);
    P.arena = arena.p + static_cast<size_t>(g) * static_cast<size_t>(grid) * static_cast<size_t>(arena_stride);
    hipStream_t s = g == 0 ? stream : gstream[g];
    try {
      // (per-launch HIP events: only between wn_engine_timing_reset and the read-back)
      if (timed != nullptr && g == 0) HIP_OK(hipEventRecord(timed->first, s));
      wn::launch_transition(model, geo, group_grid[g], smem, s, P);
      HIP_OK(hipGetLastError());
    } catch (...) {
      // a launch that did not happen fetched nothing: counter and base start over together (a kernel that did start
      // and then failed leaves the device in an error state anyway; the memset then fails too and is ignored)
      (void)hipMemsetAsync(counter.p + g, 0, sizeof(uint32_t), s);
      work_base[g] = 0;
      if (timed != nullptr) --events_used;  // (the pair taken for this launch has no end event: hand it back)
      throw;
    }
    work_base[g] += count;  // (only once the launch is known to be queued)
    if (g > 0) {
      HIP_OK(hipEventRecord(gdone[g], s));
      groups_ahead = true;
    }
  }
  if (timed != nullptr) {
    // the launch has ended when its LAST kernel has: the end event waits for every group (per-launch timing is a
    // diagnostic mode -- it joins the groups' streams at every launch, which the plain mode never does)
    for (int g = 1; g < groups; ++g) HIP_OK(hipStreamWaitEvent(stream, gdone[g], 0));
    HIP_OK(hipEventRecord(timed->second, stream));
  }
  if (flush_only) return;  // (not a transition: the stream keys and the iteration counts stay)
  ++region_launches;
  variates_pending = false;
  transition += static_cast<uint32_t>(fused);
  iteration += fused;
  if (warm) {
    warmup_iter += fused;
    est_pending = !geo.mem;  // (register kernels: the launch's last observation waits for the next prologue)
  }
  if (ref_streams) advance_reference_streams();
}

// the pending observation by itself: one launch of the warmup kernel in its observe-only mode, over every chain group
void wn_engine::flush_pending_observation() {
  if (!est_pending || in_flush) return;
  in_flush = true;
  struct Leave {
    wn_engine& e;
    ~Leave() {
      e.in_flush = false;
      e.in_step = false;
    }
  } leave{*this};
  step(true, nullptr, 0, 1, 0, /*flush_only=*/true);
  est_pending = false;
}

void wn_engine::feed_reference_streams() {
  ReferenceStreams& r = *ref_streams;
  const size_t Dn = static_cast<size_t>(D);
  for (size_t m = 0; m < C; ++m) {
    for (size_t i = 0; i < Dn; ++i) r.z[m * Dn + i] = r.normal[m](r.eng[m]);  // util.hpp:124-127, index order
    r.after_normals[m] = r.eng[m];
    std::mt19937_64 look = r.eng[m];
    // uniform_real_distribution(0,1) and bernoulli_distribution(0.5) both draw one generate_canonical value
    for (int j = 0; j < r.pool; ++j) r.u[m * r.pool + j] = std::generate_canonical<double, 53>(look);
  }
  if (z_buf.n == 0) z_buf.alloc(C * static_cast<size_t>(Dp));
  if (u_buf.n < C * static_cast<size_t>(r.pool)) u_buf.alloc(C * static_cast<size_t>(r.pool));
  HIP_OK(hipMemsetAsync(z_buf.p, 0, z_buf.n * sizeof(double), stream));
  upload_rows(z_buf, r.z.data(), 0.0);
  HIP_OK(hipMemcpyAsync(u_buf.p, r.u.data(), C * static_cast<size_t>(r.pool) * sizeof(double), hipMemcpyHostToDevice,
                        stream));
  HIP_OK(hipStreamSynchronize(stream));
  u_stride = r.pool;
  variates_pending = true;
}

void wn_engine::advance_reference_streams() {
  ReferenceStreams& r = *ref_streams;
  download(rng_draws, r.used.data(), C);
  for (size_t m = 0; m < C; ++m) {
    if (r.used[m] > r.pool) throw std::runtime_error("reference-stream pool exhausted");
    r.eng[m] = r.after_normals[m];
    r.eng[m].discard(static_cast<unsigned long long>(r.used[m]));
  }
}

namespace {

// what every launch of wn_init.h's kernels takes from the engine; the caller adds the planes it reads and writes
wn::InitParams init_params(const wn_engine& e) {
  wn::InitParams Q{};
  Q.num_chains = static_cast<int32_t>(e.C);
  Q.dim = e.D;
  Q.dim_padded = e.Dp;
  Q.model_params = e.model_params.p;
  Q.scratch = e.arena.p;
  Q.scratch_stride = e.arena_stride;
  Q.obs = e.obs;
  return Q;
}
int init_grid(const wn_engine& e) {
  return e.geo.mem ? e.grid : static_cast<int>(std::min<size_t>(e.C, static_cast<size_t>(e.num_cus) * 8));
}

void run_init(wn_engine& e, bool pos, bool masses, bool step, double scale, double smoothing, uint64_t pos_seed,
              uint32_t pos_off, uint64_t step_seed, uint32_t step_off, const double* z_dev = nullptr) {
  e.use_device();
  wn::InitParams Q = init_params(e);
  Q.do_positions = pos;
  Q.do_masses = masses;
  Q.do_step = step;
  Q.theta = e.theta.p;
  Q.mass = e.mass.p;
  Q.step_init = e.step_init.p;
  Q.grad_evals = e.grad_evals.p;
  Q.z_buf = z_dev;
  Q.scale = scale;
  Q.smoothing = smoothing;
  Q.pos_seed = pos_seed;
  Q.step_seed = step_seed;
  Q.pos_chain_offset = pos_off;
  Q.step_chain_offset = step_off;
  wn::launch_init(e.model, e.geo, init_grid(e), wn::transition_smem_bytes(e.geo.nw, 0, e.Dp), e.stream, Q);
  HIP_OK(hipGetLastError());
  e.adapters_ready = false;
}

}  // namespace

extern "C" {

const char* walnutpie_get_error_message(const WalnutpyError* err) {
  if (err == nullptr) return "Something went wrong: No error found";
  return err->msg.c_str();
}
WalnutpyErrorType walnutpie_get_error_type(const WalnutpyError* err) { return err == nullptr ? generic : err->type; }
void walnutpie_destroy_error(WalnutpyError* err) { delete err; }

// which counter-based stream definition this build draws from (wn_devmath.h kStreamVersion: the map from
// (seed, chain, transition, index) to variates; results at a fixed seed are comparable only within one version)
int wn_stream_version(void) { return wnd::kStreamVersion; }
// the code-generation flags this library was compiled with (Makefile CODEGEN_FLAGS): run-time models use the same
#ifndef WN_CODEGEN_FLAGS
#define WN_CODEGEN_FLAGS ""
#endif
const char* wn_build_flags(void) { return WN_CODEGEN_FLAGS; }
#ifndef WN_COMPILER_VERSION
#define WN_COMPILER_VERSION ""
#endif
const char* wn_build_compiler(void) { return WN_COMPILER_VERSION; }

int wn_engine_num_datasets(const wn_engine* e) { return e->num_datasets; }
void wn_engine_destroy(wn_engine* e) { delete e; }

int wn_engine_eval(wn_engine* e, const double* theta, double* logp_out, double* grad_out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || theta == nullptr || logp_out == nullptr || grad_out == nullptr)
      throw std::invalid_argument("null argument");
    const size_t C = e->C, D = static_cast<size_t>(e->D), Dp = static_cast<size_t>(e->Dp);
    e->use_device();
    // the engine's own planes stay untouched: positions and gradients go through buffers of this call
    DevBuf<double> th, grad, lp;
    th.alloc(C * Dp);
    grad.alloc(C * Dp);
    lp.alloc(C);
    const std::vector<double> padded = e->padded_rows(theta, 0.0);
    HIP_OK(hipMemcpyAsync(th.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
    wn::InitParams Q = init_params(*e);
    Q.theta = th.p;
    Q.logp_out = lp.p;
    Q.grad_out = grad.p;
    wn::launch_eval(e->model, e->geo, init_grid(*e), wn::transition_smem_bytes(e->geo.nw, 0, e->Dp), e->stream,
                    e->cfg.fused_multiply_add != 0, Q);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy2DAsync(grad_out, sizeof(double) * D, grad.p, sizeof(double) * Dp, sizeof(double) * D, C,
                            hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(logp_out, lp.p, C * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}

int wn_engine_set_positions(wn_engine* e, const double* positions, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || positions == nullptr) throw std::invalid_argument("null argument"); e->upload_rows(e->theta, positions, 0.0); });
}
int wn_engine_set_masses(wn_engine* e, const double* masses, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || masses == nullptr) throw std::invalid_argument("null argument");
    for (size_t i = 0; i < e->C * static_cast<size_t>(e->D); ++i)
      if (!(masses[i] > 0) || !std::isfinite(masses[i])) throw std::invalid_argument("masses must be positive and finite");
    e->fill(e->mass, 1.0);
    e->upload_rows(e->mass, masses, 1.0);
    e->adapters_ready = false;
  });
}
int wn_engine_set_step_sizes(wn_engine* e, const double* steps, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || steps == nullptr) throw std::invalid_argument("null argument");
    for (size_t i = 0; i < e->C; ++i)
      if (!(steps[i] > 0) || !std::isfinite(steps[i])) throw std::invalid_argument("step size must be positive and finite");
    e->use_device();
    HIP_OK(hipMemcpyAsync(e->step_init.p, steps, e->C * sizeof(double), hipMemcpyHostToDevice, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    e->adapters_ready = false;
  });
}
int wn_engine_init_positions(wn_engine* e, uint64_t seed, uint32_t chain_offset, double scale, WalnutpyError** err) {
  return guarded(err, [&] {
    if (!(scale > 0) || !std::isfinite(scale)) throw std::invalid_argument("init_scale must be positive and finite");
    run_init(*e, true, false, false, scale, 0.0, seed, chain_offset, 0, 0);
  });
}
int wn_engine_init_masses_from_grad(wn_engine* e, double smoothing, WalnutpyError** err) {
  return guarded(err, [&] {
    if (!(smoothing > 0 && smoothing < 1)) throw std::invalid_argument("mass_smoothing must be in (0, 1)");
    run_init(*e, false, true, false, 1.0, smoothing, 0, 0, 0, 0);
  });
}
int wn_engine_get_masses(wn_engine* e, double* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument"); e->download_rows(e->mass, out); });
}
int wn_engine_adapt_step(wn_engine* e, uint64_t seed, uint32_t chain_offset, WalnutpyError** err) {
  return guarded(err, [&] { run_init(*e, false, false, true, 1.0, 0.0, 0, 0, seed, chain_offset); });
}
int wn_engine_adapt_step_with_normals(wn_engine* e, const double* normals, WalnutpyError** err) {
  return guarded(err, [&] {
    e->use_device();
    if (e->z_buf.n == 0) e->z_buf.alloc(e->C * static_cast<size_t>(e->Dp));
    HIP_OK(hipMemsetAsync(e->z_buf.p, 0, e->z_buf.n * sizeof(double), e->stream));
    e->upload_rows(e->z_buf, normals, 0.0);
    run_init(*e, false, false, true, 1.0, 0.0, 0, 0, 0, 0, e->z_buf.p);
  });
}
void* wn_internal_make_error(const char* msg, int type) {
  return new WalnutpyError{msg, static_cast<WalnutpyErrorType>(type)};
}
int wn_engine_seed(wn_engine* e, uint64_t seed, uint32_t chain_offset, WalnutpyError** err) {
  return guarded(err, [&] {
    e->seed = seed;
    e->chain_offset = chain_offset;
    e->transition = 0;
  });
}
int wn_engine_seed_reference_streams(wn_engine* e, uint64_t seed, WalnutpyError** err) {
  return guarded(err, [&] {
    auto r = std::make_unique<ReferenceStreams>();
    r->eng.reserve(e->C);
    for (size_t m = 0; m < e->C; ++m) {
      std::seed_seq ss{static_cast<size_t>(seed), m + 1u};  // api.hpp:48-49
      r->eng.emplace_back(ss);
    }
    r->normal.assign(e->C, std::normal_distribution<double>(0.0, 1.0));
    r->after_normals = r->eng;
    r->z.assign(e->C * static_cast<size_t>(e->D), 0.0);
    // scalar draws per transition: one bernoulli + one Metropolis uniform per doubling, one Barker uniform
    // per inner merge: at most 2^max_depth - 1 + max_depth
    const int md = e->cfg.max_trajectory_doublings;
    if (md > 16) throw std::invalid_argument("reference streams support max_trajectory_doublings <= 16");
    r->pool = (1 << md) - 1 + md;
    r->u.assign(e->C * static_cast<size_t>(r->pool), 0.0);
    r->used.assign(e->C, 0);
    e->ref_streams = std::move(r);
    e->seed = seed;
    e->transition = 0;
  });
}
int wn_engine_set_variates(wn_engine* e, const double* normals, const double* uniforms, int u_per_chain,
                           WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || normals == nullptr || uniforms == nullptr) throw std::invalid_argument("null argument");
    if (u_per_chain < 1) throw std::invalid_argument("u_per_chain must be positive");
    e->use_device();
    if (e->z_buf.n == 0) e->z_buf.alloc(e->C * static_cast<size_t>(e->Dp));
    if (e->u_buf.n < e->C * static_cast<size_t>(u_per_chain)) e->u_buf.alloc(e->C * static_cast<size_t>(u_per_chain));
    HIP_OK(hipMemsetAsync(e->z_buf.p, 0, e->z_buf.n * sizeof(double), e->stream));
    e->upload_rows(e->z_buf, normals, 0.0);
    HIP_OK(hipMemcpyAsync(e->u_buf.p, uniforms, e->C * static_cast<size_t>(u_per_chain) * sizeof(double),
                          hipMemcpyHostToDevice, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    e->u_stride = u_per_chain;
    e->variates_pending = true;
  });
}

int wn_engine_warmup_step(wn_engine* e, double* draws_dev, int64_t draws_stride, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e->frozen) throw std::runtime_error("warmup_step after freeze");
    e->ensure_adapters();
    e->step(true, draws_dev, draws_stride);
  });
}
int wn_engine_warmup_steps(wn_engine* e, int transitions, double* draws_dev, int64_t draws_stride,
                           int64_t draws_transition_stride, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr) throw std::invalid_argument("null argument");
    if (e->frozen) throw std::runtime_error("warmup_step after freeze");
    e->ensure_adapters();
    e->step(true, draws_dev, draws_stride, transitions, draws_transition_stride);
  });
}
int wn_engine_sample_step(wn_engine* e, double* draws_dev, int64_t draws_stride, WalnutpyError** err) {
  return guarded(err, [&] {
    if (!e->frozen) throw std::runtime_error("sample_step before freeze");
    e->step(false, draws_dev, draws_stride);
  });
}
int wn_engine_sample_steps(wn_engine* e, int transitions, double* draws_dev, int64_t draws_stride,
                           int64_t draws_transition_stride, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr) throw std::invalid_argument("null argument");
    if (!e->frozen) throw std::runtime_error("sample_step before freeze");
    e->step(false, draws_dev, draws_stride, transitions, draws_transition_stride);
  });
}
int wn_engine_synchronize(wn_engine* e, WalnutpyError** err) {
  return guarded(err, [&] {
    e->use_device();
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}
int wn_engine_check(wn_engine* e, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr) throw std::invalid_argument("null argument"); e->check_transitions(); });
}

int wn_engine_get_positions(wn_engine* e, double* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument"); e->download_rows(e->theta, out); });
}
int wn_engine_get_step_sizes(wn_engine* e, double* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument");
    if (e->frozen) {
      e->download(e->step_size, out, e->C);
    } else if (e->adapters_ready) {
      std::vector<double> a(6 * e->C);
      e->download(e->adam, a.data(), a.size());
      for (size_t c = 0; c < e->C; ++c) out[c] = wnd::dexp(a[6 * c]);
    } else {
      e->download(e->step_init, out, e->C);
    }
  });
}
int wn_engine_get_logp(wn_engine* e, double* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument"); e->download(e->logp, out, e->C); });
}
int wn_engine_get_min_micro(wn_engine* e, int32_t* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument");
    if (e->frozen) {
      e->download(e->min_micro, out, e->C);
    } else {
      std::vector<double> mm(2 * e->C);
      e->download(e->mm_state, mm.data(), mm.size());
      for (size_t c = 0; c < e->C; ++c) {
        const long long est = std::llround(mm[2 * c] / mm[2 * c + 1] / e->cfg.max_macro_steps_target);
        out[c] = static_cast<int32_t>(std::max<long long>(est, e->cfg.min_micro_steps));
      }
    }
  });
}
int wn_engine_get_depths(wn_engine* e, int32_t* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument"); e->download(e->depth, out, e->C); });
}
int wn_engine_get_grad_evals(wn_engine* e, int64_t* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument"); e->download(e->grad_evals, out, e->C); });
}
int wn_engine_get_failed_extensions(wn_engine* e, int32_t* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument");
    e->download(e->failed_ext, out, e->C);
  });
}
int wn_engine_get_rng_draws(wn_engine* e, int32_t* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument"); e->download(e->rng_draws, out, e->C); });
}
int wn_engine_get_adam(wn_engine* e, double* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || out == nullptr) throw std::invalid_argument("null argument"); e->download(e->adam, out, 6 * e->C); });
}
int wn_engine_get_estimator(wn_engine* e, double* dm, double* ds, double* sm, double* ss, double* w,
                            WalnutpyError** err) {
  return guarded(err, [&] {
    e->download_rows(e->draw_mean, dm);
    e->download_rows(e->draw_ssd, ds);
    e->download_rows(e->score_mean, sm);
    e->download_rows(e->score_ssd, ss);
    e->download(e->est_weight, w, 2 * e->C);
  });
}

int wn_engine_lanes(const wn_engine* e) { return 64 * e->geo.nw; }
int wn_engine_is_streaming(const wn_engine* e) { return e->geo.mem ? 1 : 0; }
int wn_engine_dim_padded(const wn_engine* e) { return e->Dp; }
int wn_engine_workgroups(const wn_engine* e) { return e->grid; }
int wn_engine_chain_groups(const wn_engine* e) { return e->groups; }
int wn_engine_held_tiles(const wn_engine* e) {
  return (e->geo.mem && e->hold_moving_end) ? wn::model_ops(e->model).hold_tiles(e->geo.nw) : 0;
}
int wn_engine_lds_vectors(const wn_engine* e) { return e->pool_lds; }
int64_t wn_engine_iteration(const wn_engine* e) { return e->iteration; }
void* wn_engine_stream(const wn_engine* e) { return reinterpret_cast<void*>(e->stream); }
double* wn_engine_positions_device(const wn_engine* e) { return e->theta.p; }
int wn_engine_last_kernel_ms(wn_engine* e, float* ms, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e->events_used == 0) throw std::runtime_error("no transition has been timed: call wn_engine_timing_reset first");
    e->use_device();
    auto& ev = e->events[e->events_used - 1];
    HIP_OK(hipEventSynchronize(ev.second));
    HIP_OK(hipEventElapsedTime(ms, ev.first, ev.second));
  });
}
int wn_engine_timing_reset(wn_engine* e, WalnutpyError** err) {
  return guarded(err, [&] {
    e->events_used = 0;
    e->timing = true;
  });
}
int wn_engine_kernel_times(wn_engine* e, float* ms_out, int max_launches, int* num_launches, WalnutpyError** err) {
  return guarded(err, [&] {
    e->use_device();
    // the last min(launches, ring) launches since the reset, oldest first
    const size_t have = std::min(e->events_used, wn_engine::kEventRing);
    const int n = static_cast<int>(have);
    if (num_launches) *num_launches = n;
    for (int i = 0; i < n && i < max_launches; ++i) {
      const size_t slot = (e->events_used - have + static_cast<size_t>(i)) % wn_engine::kEventRing;
      HIP_OK(hipEventSynchronize(e->events[slot].second));
      HIP_OK(hipEventElapsedTime(&ms_out[i], e->events[slot].first, e->events[slot].second));
    }
  });
}
int wn_engine_region_begin(wn_engine* e, WalnutpyError** err) {
  return guarded(err, [&] {
    e->use_device();
    if (e->region_begin == nullptr) {
      HIP_OK(hipEventCreate(&e->region_begin));
      HIP_OK(hipEventCreate(&e->region_end));
    }
    e->timing = false;  // one pair of events for the whole region instead of one pair per launch
    e->region_launches = 0;
    HIP_OK(hipEventRecord(e->region_begin, e->stream));
  });
}
int wn_engine_region_ms(wn_engine* e, float* total_ms, int* launches, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e->region_begin == nullptr) throw std::runtime_error("wn_engine_region_begin has not been called");
    e->use_device();
    HIP_OK(hipEventRecord(e->region_end, e->stream));
    HIP_OK(hipEventSynchronize(e->region_end));
    HIP_OK(hipEventElapsedTime(total_ms, e->region_begin, e->region_end));
    if (launches) *launches = static_cast<int>(e->region_launches);
  });
}
int wn_engine_set_stream(wn_engine* e, void* stream, WalnutpyError** err) {
  return guarded(err, [&] {
    e->use_device();
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->own_stream && e->stream) HIP_OK(hipStreamDestroy(e->stream));
    e->stream = reinterpret_cast<hipStream_t>(stream);
    e->own_stream = false;
    // the caller orders its own work (collectives on the draws) behind the launches on THIS stream: one chain group
    e->groups = 1;
    e->gstream[0] = e->stream;
    e->group_begin[1] = e->C;
    e->group_grid[0] = static_cast<int>(std::min<size_t>(e->C, static_cast<size_t>(e->grid)));
    e->groups_ahead = false;
  });
}
int wn_engine_wait_stream(wn_engine* e, void* stream, WalnutpyError** err) {
  return guarded(err, [&] {
    HIP_OK(hipSetDevice(e->device));  // (not use_device(): the groups are not joined, they only get one more wait each)
    if (e->ext_point == nullptr) HIP_OK(hipEventCreateWithFlags(&e->ext_point, hipEventDisableTiming));
    HIP_OK(hipEventRecord(e->ext_point, reinterpret_cast<hipStream_t>(stream)));
    for (int g = 0; g < e->groups; ++g) HIP_OK(hipStreamWaitEvent(e->gstream[g], e->ext_point, 0));
  });
}
int wn_engine_wait_event(wn_engine* e, void* event, WalnutpyError** err) {
  return guarded(err, [&] {
    HIP_OK(hipSetDevice(e->device));
    for (int g = 0; g < e->groups; ++g) HIP_OK(hipStreamWaitEvent(e->gstream[g], reinterpret_cast<hipEvent_t>(event), 0));
  });
}
int wn_engine_release_stream(wn_engine* e, void* stream, WalnutpyError** err) {
  return guarded(err, [&] {
    HIP_OK(hipSetDevice(e->device));
    if (e->rel_point == nullptr) HIP_OK(hipEventCreateWithFlags(&e->rel_point, hipEventDisableTiming));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_OK(hipEventRecord(e->rel_point, e->stream));
    HIP_OK(hipStreamWaitEvent(s, e->rel_point, 0));
    // (gdone[g] was recorded behind group g's last launch; a group that has not launched yet has nothing to wait for)
    if (e->groups_ahead)
      for (int g = 1; g < e->groups; ++g) HIP_OK(hipStreamWaitEvent(s, e->gdone[g], 0));
  });
}

}  // extern "C"

// An emulation build that lists this file as the engine's only source (the build script of the test suite before the
// engine was split into units) compiles the other units as part of this one.  tests/cpusim/build.py compiles every
// wn_*.hip by itself, as the Makefile does, and says so with WN_ENGINE_UNITS.
#if defined(WN_CPU_SIM) && !defined(WN_ENGINE_UNITS)
#include "wn_engine_build.hip"
#include "wn_engine_elementwise.hip"
#include "wn_engine_pointwise.hip"
#include "wn_engine_predict.hip"
#include "wn_probes.hip"
#endif
