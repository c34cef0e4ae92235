// wn_engine_predict.hip -- predictions on the engine's observation block (wn_predict.h): wn_engine_predict, the linear
// predictor, expected response and variance of every row at given parameter vectors; wn_engine_predict_fold, their
// moments over the draws of a wn_chains; wn_engine_predict_chains, one of them per draw as a wn_chains of its own.
#include "wn_engine.h"

#include "wn_predict.h"

namespace {
// the engine's model as the predict entry points need it: a data model with the hook, or a `config` error
const wn::PredictOps& predict_ops(const wn_engine* e) {
  const wn::ModelOps& ops = wn::model_ops(e->model);
  if (!ops.uses_data || e->obs.x == nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model: this engine holds no data, there are no rows to predict "
                                "(create it with wn_engine_create_observed)");
  if (ops.predict == nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model declares no predictions (wn_model_api.h: kPredict, "
                                "predict())");
  return *ops.predict;
}
// what every mode hands the kernel about block b; num_items = `units` (parameter vectors, or chains) x the block's tiles
wn::PredictParams predict_params(const wn_engine* e, const RowBlock& b, int mode, size_t units) {
  wn::PredictParams Q{};
  Q.obs = e->obs;
  Q.dim = e->D;
  Q.mode = mode;
  Q.row0 = b.row0;
  Q.num_rows = b.rows;
  Q.num_tiles = (b.rows + wn::kPointwiseTile - 1) / wn::kPointwiseTile;
  Q.num_items = static_cast<int64_t>(units) * Q.num_tiles;
  return Q;
}
// the chains as the engine can read them: G * k chains of the model's dimension on the engine's device -> k
size_t chains_per_block(const wn_engine* e, const wn_chains_layout& ch) {
  if (ch.dims != static_cast<size_t>(e->D))
    throw std::invalid_argument("the chains hold draws of " + std::to_string(ch.dims) + " dimensions, the engine's model has " +
                                std::to_string(e->D) + " parameters");
  const size_t G = static_cast<size_t>(e->num_datasets);
  if (ch.num_chains % G != 0)
    throw std::invalid_argument("the number of chains (" + std::to_string(ch.num_chains) + ") must be a multiple of the "
                                "engine's datasets / weight sets (" + std::to_string(G) + "): block g of the chains is "
                                "predicted on dataset g");
  if (ch.device != e->device) throw std::invalid_argument("the chains live on another device than the engine");
  return ch.num_chains / G;
}
bool shares_rows(const wn_engine* e) { return e->obs.chains_per_dataset > 0 && e->obs.offsets == nullptr; }
}  // namespace

extern "C" {

int wn_engine_predict(wn_engine* e, const double* theta, size_t num_theta, int dataset, double* eta_out, double* mean_out,
                      double* var_out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || theta == nullptr) throw std::invalid_argument("null argument");
    const wn::PredictOps& pr = predict_ops(e);
    if (eta_out == nullptr && mean_out == nullptr && var_out == nullptr)
      throw std::invalid_argument("every output is NULL: ask for at least one of eta_out, mean_out, var_out");
    if (num_theta < 1 || num_theta > 0x7fffffffull) throw std::invalid_argument("num_theta must be in [1, 2^31)");
    const bool sets = shares_rows(e);
    if (dataset < 0 || dataset >= (sets ? 1 : e->num_datasets))
      throw std::invalid_argument(sets ? "weight sets share one block of rows: dataset must be 0"
                                       : "dataset must be in [0, wn_engine_num_datasets)");
    e->use_device();
    const RowBlock b = row_block(e, host_offsets(e), dataset);
    const size_t T = num_theta, D = static_cast<size_t>(e->D), N = static_cast<size_t>(b.rows);
    double* const host[3] = {eta_out, mean_out, var_out};
    DevBuf<double> th, out[3];
    th.alloc(T * D);
    for (int i = 0; i < 3; ++i)
      if (host[i] != nullptr) out[i].alloc(T * N);
    HIP_OK(hipMemcpyAsync(th.p, theta, T * D * sizeof(double), hipMemcpyHostToDevice, e->stream));
    wn::PredictParams Q = predict_params(e, b, wn::kPredictMatrix, T);
    Q.theta = th.p;
    Q.eta_out = out[0].p;
    Q.mu_out = out[1].p;
    Q.v_out = out[2].p;
    pr.launch(e->geo, pointwise_grid(Q.num_items), e->stream, e->cfg.fused_multiply_add != 0, Q);
    HIP_OK(hipGetLastError());
    for (int i = 0; i < 3; ++i)
      if (host[i] != nullptr)
        HIP_OK(hipMemcpyAsync(host[i], out[i].p, T * N * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}

int wn_engine_predict_fold(wn_engine* e, wn_chains* chains, const uint8_t* row_mask, double* eta_mean, double* eta_var,
                           double* mean, double* mean_var, double* noise_var, int64_t* count, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || chains == nullptr || eta_mean == nullptr || eta_var == nullptr || mean == nullptr ||
        mean_var == nullptr || noise_var == nullptr || count == nullptr)
      throw std::invalid_argument("null argument");
    const wn::PredictOps& pr = predict_ops(e);
    wn_chains_layout ch{};
    wn_chains_layout_of(chains, &ch);
    const size_t k = chains_per_block(e, ch);
    const size_t G = static_cast<size_t>(e->num_datasets);
    e->use_device();
    HIP_OK(hipStreamSynchronize(ch.stream));  // (uploads queued on the handle's own stream)
    const std::vector<int64_t> offsets = host_offsets(e);
    const size_t total = shares_rows(e) ? G * static_cast<size_t>(e->obs.num_obs) : e->data_rows;
    constexpr size_t A = wn::kPredictAccumulators;
    double* const host[A] = {eta_mean, eta_var, mean, mean_var, noise_var};
    DevBuf<double> d_out[A], partial, state;
    DevBuf<long long> d_count;
    DevBuf<uint8_t> d_mask;
    for (size_t i = 0; i < A; ++i) d_out[i].alloc(total);
    d_count.alloc(total);
    if (row_mask != nullptr) {
      d_mask.alloc(total);
      HIP_OK(hipMemcpyAsync(d_mask.p, row_mask, total, hipMemcpyHostToDevice, e->stream));
    }
    // the per-chain partials of one SLAB of chains at a time, as in wn_engine_log_predictive
    const size_t budget = pointwise_workspace_bytes();
    for (size_t g = 0; g < G; ++g) {
      const RowBlock b = row_block(e, offsets, static_cast<int>(g));
      const size_t N = static_cast<size_t>(b.rows);
      const size_t slab = std::max<size_t>(1, std::min(k, budget / (A * sizeof(double) * N)));
      if (partial.n < A * slab * N) partial.alloc(A * slab * N);
      if (slab < k && state.n < (A + 1) * N) state.alloc((A + 1) * N);
      for (size_t c0 = 0; c0 < k; c0 += slab) {
        const size_t nc = std::min(slab, k - c0);
        wn::PredictParams Q = predict_params(e, b, wn::kPredictFold, nc);
        Q.draws = ch.draws;
        Q.chain_off = ch.off;
        Q.chain_len = ch.len;
        Q.chain0 = static_cast<int32_t>(g * k + c0);
        Q.slab_chains = static_cast<int32_t>(nc);
        Q.mask = row_mask != nullptr ? d_mask.p + b.out0 : nullptr;
        Q.partial = partial.p;
        pr.launch(e->geo, pointwise_grid(Q.num_items), e->stream, e->cfg.fused_multiply_add != 0, Q);
        HIP_OK(hipGetLastError());
        wn::PredictCombineParams R{};
        R.partial = partial.p;
        R.chain_len = ch.len;
        R.chain0 = Q.chain0;
        R.slab_chains = Q.slab_chains;
        R.num_rows = b.rows;
        R.first = c0 == 0 ? 1 : 0;
        R.last = c0 + nc == k ? 1 : 0;
        R.mask = Q.mask;
        R.state = state.p;
        R.eta_mean = d_out[0].p + b.out0;
        R.eta_var = d_out[1].p + b.out0;
        R.mean = d_out[2].p + b.out0;
        R.mean_var = d_out[3].p + b.out0;
        R.noise_var = d_out[4].p + b.out0;
        R.count = d_count.p + b.out0;
        pr.launch_combine(static_cast<int>((N + wn::kPointwiseCombineBlock - 1) / wn::kPointwiseCombineBlock), e->stream, R);
        HIP_OK(hipGetLastError());
      }
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "count goes out as int64");
    for (size_t i = 0; i < A; ++i)
      HIP_OK(hipMemcpyAsync(host[i], d_out[i].p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(count, d_count.p, total * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}

int wn_engine_predict_chains(wn_engine* e, wn_chains* chains, int block, int what, wn_chains** out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || chains == nullptr || out == nullptr) throw std::invalid_argument("null argument");
    const wn::PredictOps& pr = predict_ops(e);
    if (what != 0 && what != 1)
      throw std::invalid_argument("what must be 0 (eta, the linear predictor) or 1 (the expected response), got " +
                                  std::to_string(what));
    wn_chains_layout ch{};
    wn_chains_layout_of(chains, &ch);
    const size_t k = chains_per_block(e, ch);
    if (block < 0 || block >= e->num_datasets)
      throw std::invalid_argument("block must be in [0, wn_engine_num_datasets): it selects the chains of one dataset / "
                                  "weight set, got " + std::to_string(block));
    e->use_device();
    HIP_OK(hipStreamSynchronize(ch.stream));  // (uploads queued on the handle's own stream)
    const RowBlock b = row_block(e, host_offsets(e), block);
    const size_t N = static_cast<size_t>(b.rows), c0 = static_cast<size_t>(block) * k;
    std::vector<int64_t> lengths(k);
    int64_t max_len = 0;
    for (size_t c = 0; c < k; ++c) {
      lengths[c] = ch.host_len[c0 + c];
      max_len = std::max(max_len, lengths[c]);
    }
    if (max_len > 0x7fffffffll) throw std::invalid_argument("chain too long");
    const size_t count = k * static_cast<size_t>(max_len) * N;
    double* gen = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&gen), count * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      throw std::runtime_error("wn_engine_predict_chains: could not allocate " + std::to_string(count * sizeof(double)) +
                               " bytes on the device for " + std::to_string(k) + " chains x " + std::to_string(max_len) +
                               " draws x " + std::to_string(N) + " rows");
    }
    struct Guard {
      double* p;
      ~Guard() {
        if (p != nullptr) (void)hipFree(p);
      }
    } guard{gen};
    wn::PredictParams Q = predict_params(e, b, wn::kPredictChains, k);
    Q.draws = ch.draws;
    Q.chain_off = ch.off;
    Q.chain_len = ch.len;
    Q.chain0 = static_cast<int32_t>(c0);
    Q.slab_chains = static_cast<int32_t>(k);
    Q.what = what;
    Q.max_len = static_cast<int32_t>(max_len);
    Q.gen = gen;
    pr.launch(e->geo, pointwise_grid(Q.num_items), e->stream, e->cfg.fused_multiply_add != 0, Q);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(e->stream));
    // the block changes hands: a wn_chains of N dimensions that keeps the source chains' lengths and frees it
    WalnutpyError* inner = nullptr;
    if (wn_chains_adopt(out, gen, k, static_cast<size_t>(max_len), N, max_len * static_cast<int64_t>(N), lengths.data(),
                        e->device, &inner) != 0) {
      const std::string msg = inner != nullptr ? inner->msg : "wn_chains_adopt failed";
      const bool cfg = inner != nullptr && inner->type == config;
      delete inner;
      if (cfg) throw std::invalid_argument(msg);
      throw std::runtime_error(msg);
    }
    guard.p = nullptr;
  });
}

}  // extern "C"
