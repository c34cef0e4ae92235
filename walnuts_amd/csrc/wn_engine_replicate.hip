// wn_engine_replicate.hip -- simulated replicates on the engine's observation block (wn_replicate.h, wn_devrand.h):
// wn_engine_replicate, y_rep of every row at given parameter vectors; wn_engine_replicate_chains, one replicate per draw
// of a wn_chains as a wn_chains of its own; wn_engine_replicate_check, the posterior predictive statistics per draw.
#include "wn_engine.h"

#include "wn_replicate.h"

namespace {
// the engine's model as the replicate entry points need it: a data model with the hook, or a `config` error
const wn::ReplicateOps& replicate_ops(const wn_engine* e) {
  const wn::ModelOps& ops = wn::model_ops(e->model);
  if (!ops.uses_data || e->obs.x == nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model: this engine holds no data, there are no rows to replicate "
                                "(create it with wn_engine_create_observed)");
  if (ops.replicate == nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model declares no replicates (wn_model_api.h: kReplicate, "
                                "replicate())");
  return *ops.replicate;
}
wn::ReplicateParams replicate_params(const wn_engine* e, const RowBlock& b, int mode, uint64_t seed) {
  wn::ReplicateParams Q{};
  Q.obs = e->obs;
  Q.dim = e->D;
  Q.mode = mode;
  Q.row0 = b.row0;
  Q.num_rows = b.rows;
  Q.num_tiles = (b.rows + wn::kPointwiseTile - 1) / wn::kPointwiseTile;
  Q.seed = seed;
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
                                "replicated on dataset g");
  if (ch.device != e->device) throw std::invalid_argument("the chains live on another device than the engine");
  if (ch.num_chains > 0x7fffffffull) throw std::invalid_argument("too many chains");
  return ch.num_chains / G;
}
bool shares_rows(const wn_engine* e) { return e->obs.chains_per_dataset > 0 && e->obs.offsets == nullptr; }
}  // namespace

extern "C" {

int wn_engine_replicate(wn_engine* e, const double* theta, size_t num_theta, int dataset, uint64_t seed, double* out,
                        WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || theta == nullptr || out == nullptr) throw std::invalid_argument("null argument");
    const wn::ReplicateOps& rp = replicate_ops(e);
    if (num_theta < 1 || num_theta > 0x7fffffffull) throw std::invalid_argument("num_theta must be in [1, 2^31)");
    const bool sets = shares_rows(e);
    if (dataset < 0 || dataset >= (sets ? 1 : e->num_datasets))
      throw std::invalid_argument(sets ? "weight sets share one block of rows: dataset must be 0"
                                       : "dataset must be in [0, wn_engine_num_datasets)");
    e->use_device();
    const RowBlock b = row_block(e, host_offsets(e), dataset);
    const size_t T = num_theta, D = static_cast<size_t>(e->D), N = static_cast<size_t>(b.rows);
    DevBuf<double> th, d_out;
    th.alloc(T * D);
    d_out.alloc(T * N);
    HIP_OK(hipMemcpyAsync(th.p, theta, T * D * sizeof(double), hipMemcpyHostToDevice, e->stream));
    wn::ReplicateParams Q = replicate_params(e, b, wn::kReplicateMatrix, seed);
    Q.num_items = static_cast<int64_t>(T) * Q.num_tiles;
    Q.theta = th.p;
    Q.out = d_out.p;
    rp.launch(e->geo, pointwise_grid(Q.num_items), e->stream, e->cfg.fused_multiply_add != 0, Q);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out, d_out.p, T * N * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}

int wn_engine_replicate_chains(wn_engine* e, wn_chains* chains, int block, uint64_t seed, wn_chains** out,
                               WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || chains == nullptr || out == nullptr) throw std::invalid_argument("null argument");
    const wn::ReplicateOps& rp = replicate_ops(e);
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
      throw std::runtime_error("wn_engine_replicate_chains: could not allocate " + std::to_string(count * sizeof(double)) +
                               " bytes on the device for " + std::to_string(k) + " chains x " + std::to_string(max_len) +
                               " draws x " + std::to_string(N) + " rows");
    }
    struct Guard {
      double* p;
      ~Guard() {
        if (p != nullptr) (void)hipFree(p);
      }
    } guard{gen};
    wn::ReplicateParams Q = replicate_params(e, b, wn::kReplicateChains, seed);
    Q.num_items = static_cast<int64_t>(k) * Q.num_tiles;
    Q.draws = ch.draws;
    Q.chain_off = ch.off;
    Q.chain_len = ch.len;
    Q.chain0 = static_cast<int32_t>(c0);
    Q.slab_chains = static_cast<int32_t>(k);
    Q.max_len = static_cast<int32_t>(max_len);
    Q.gen = gen;
    rp.launch(e->geo, pointwise_grid(Q.num_items), e->stream, e->cfg.fused_multiply_add != 0, Q);
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

int wn_engine_replicate_check(wn_engine* e, wn_chains* chains, const uint8_t* row_mask, uint64_t seed, double* stat_rep,
                              double* stat_obs, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || chains == nullptr || stat_rep == nullptr || stat_obs == nullptr)
      throw std::invalid_argument("null argument");
    const wn::ReplicateOps& rp = replicate_ops(e);
    wn_chains_layout ch{};
    wn_chains_layout_of(chains, &ch);
    const size_t k = chains_per_block(e, ch);
    const size_t G = static_cast<size_t>(e->num_datasets);
    e->use_device();
    HIP_OK(hipStreamSynchronize(ch.stream));  // (uploads queued on the handle's own stream)
    const std::vector<int64_t> offsets = host_offsets(e);
    const size_t total = shares_rows(e) ? G * static_cast<size_t>(e->obs.num_obs) : e->data_rows;
    int64_t max_len = 0;
    for (size_t c = 0; c < ch.num_chains; ++c) max_len = std::max<int64_t>(max_len, ch.host_len[c]);
    if (max_len > 0x7fffffffll) throw std::invalid_argument("chain too long");
    if (max_len == 0) return;  // no draw: the outputs hold no entry
    const size_t plane = ch.num_chains * static_cast<size_t>(max_len), count = wn::kReplicateStats * plane;
    DevBuf<double> d_rep, d_obs;
    DevBuf<uint8_t> d_mask;
    d_rep.alloc(count);
    d_obs.alloc(count);
    if (row_mask != nullptr) {
      d_mask.alloc(total);
      HIP_OK(hipMemcpyAsync(d_mask.p, row_mask, total, hipMemcpyHostToDevice, e->stream));
    }
    for (size_t g = 0; g < G; ++g) {
      const RowBlock b = row_block(e, offsets, static_cast<int>(g));
      wn::ReplicateParams Q = replicate_params(e, b, wn::kReplicateCheck, seed);
      Q.num_items = static_cast<int64_t>(k) * max_len;
      Q.draws = ch.draws;
      Q.chain_off = ch.off;
      Q.chain_len = ch.len;
      Q.chain0 = static_cast<int32_t>(g * k);
      Q.slab_chains = static_cast<int32_t>(k);
      Q.max_len = static_cast<int32_t>(max_len);
      Q.mask = row_mask != nullptr ? d_mask.p + b.out0 : nullptr;
      Q.total_chains = static_cast<int32_t>(ch.num_chains);
      Q.stat_rep = d_rep.p;
      Q.stat_obs = d_obs.p;
      rp.launch(e->geo, pointwise_grid(Q.num_items), e->stream, e->cfg.fused_multiply_add != 0, Q);
      HIP_OK(hipGetLastError());
    }
    HIP_OK(hipMemcpyAsync(stat_rep, d_rep.p, count * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(stat_obs, d_obs.p, count * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}

}  // extern "C"
