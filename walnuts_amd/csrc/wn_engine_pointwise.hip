// wn_engine_pointwise.hip -- pointwise scoring on the engine's observation block (wn_pointwise.h): wn_engine_log_lik,
// the log-likelihood of every row at given parameter vectors, and wn_engine_log_predictive, the log predictive density
// of every row over the draws of a wn_chains.
#include "wn_engine.h"

#include "wn_engine_pointwise.h"

extern "C" {

int wn_engine_log_lik(wn_engine* e, const double* theta, size_t num_theta, int dataset, double* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || theta == nullptr || out == nullptr) throw std::invalid_argument("null argument");
    const wn::PointwiseOps& pw = pointwise_ops(e);
    if (num_theta < 1 || num_theta > 0x7fffffffull) throw std::invalid_argument("num_theta must be in [1, 2^31)");
    const bool sets = e->obs.chains_per_dataset > 0 && e->obs.offsets == nullptr;
    if (dataset < 0 || dataset >= (sets ? 1 : e->num_datasets))
      throw std::invalid_argument(sets ? "weight sets share one block of rows: dataset must be 0"
                                       : "dataset must be in [0, wn_engine_num_datasets)");
    e->use_device();
    const RowBlock b = row_block(e, host_offsets(e), dataset);
    const size_t T = num_theta, D = static_cast<size_t>(e->D), N = static_cast<size_t>(b.rows);
    DevBuf<double> th, ll;
    th.alloc(T * D);
    ll.alloc(T * N);
    HIP_OK(hipMemcpyAsync(th.p, theta, T * D * sizeof(double), hipMemcpyHostToDevice, e->stream));
    wn::PointwiseParams Q = pointwise_params(e, b, /*predictive=*/false, T);
    Q.theta = th.p;
    Q.out = ll.p;
    pw.launch(e->geo, pointwise_grid(Q.num_items), e->stream, e->cfg.fused_multiply_add != 0, Q);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out, ll.p, T * N * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}

int wn_engine_log_predictive(wn_engine* e, wn_chains* chains, const uint8_t* row_mask, double* lpd, double* mean,
                             double* var, int64_t* count, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || chains == nullptr || lpd == nullptr || mean == nullptr || var == nullptr || count == nullptr)
      throw std::invalid_argument("null argument");
    const wn::PointwiseOps& pw = pointwise_ops(e);
    wn_chains_layout ch{};
    wn_chains_layout_of(chains, &ch);
    if (ch.dims != static_cast<size_t>(e->D))
      throw std::invalid_argument("the chains hold draws of " + std::to_string(ch.dims) + " dimensions, the engine's model has " +
                                  std::to_string(e->D) + " parameters");
    const size_t G = static_cast<size_t>(e->num_datasets);
    if (ch.num_chains % G != 0)
      throw std::invalid_argument("the number of chains (" + std::to_string(ch.num_chains) + ") must be a multiple of the "
                                  "engine's datasets / weight sets (" + std::to_string(G) + "): block g of the chains is "
                                  "scored on dataset g");
    if (ch.device != e->device) throw std::invalid_argument("the chains live on another device than the engine");
    const size_t k = ch.num_chains / G;
    e->use_device();
    HIP_OK(hipStreamSynchronize(ch.stream));  // (uploads queued on the handle's own stream)
    const std::vector<int64_t> offsets = host_offsets(e);
    const bool sets = e->obs.chains_per_dataset > 0 && e->obs.offsets == nullptr;
    const size_t total = sets ? G * static_cast<size_t>(e->obs.num_obs) : e->data_rows;
    DevBuf<double> d_lpd, d_mean, d_var, partial, state;
    DevBuf<long long> d_count;
    DevBuf<uint8_t> d_mask;
    d_lpd.alloc(total);
    d_mean.alloc(total);
    d_var.alloc(total);
    d_count.alloc(total);
    if (row_mask != nullptr) {
      d_mask.alloc(total);
      HIP_OK(hipMemcpyAsync(d_mask.p, row_mask, total, hipMemcpyHostToDevice, e->stream));
    }
    // the per-chain partials of one SLAB of chains at a time: the merge carries its state from slab to slab in chain
    // order, so the workspace's size changes nothing
    const size_t budget = pointwise_workspace_bytes();
    for (size_t g = 0; g < G; ++g) {
      const RowBlock b = row_block(e, offsets, static_cast<int>(g));
      const size_t N = static_cast<size_t>(b.rows);
      const size_t slab = std::max<size_t>(1, std::min(k, budget / (4 * sizeof(double) * N)));
      if (partial.n < 4 * slab * N) partial.alloc(4 * slab * N);
      if (slab < k && state.n < 5 * N) state.alloc(5 * N);
      for (size_t c0 = 0; c0 < k; c0 += slab) {
        const size_t nc = std::min(slab, k - c0);
        wn::PointwiseParams Q = pointwise_params(e, b, /*predictive=*/true, nc);
        Q.draws = ch.draws;
        Q.chain_off = ch.off;
        Q.chain_len = ch.len;
        Q.chain0 = static_cast<int32_t>(g * k + c0);
        Q.slab_chains = static_cast<int32_t>(nc);
        Q.mask = row_mask != nullptr ? d_mask.p + b.out0 : nullptr;
        Q.partial = partial.p;
        pw.launch(e->geo, pointwise_grid(Q.num_items), e->stream, e->cfg.fused_multiply_add != 0, Q);
        HIP_OK(hipGetLastError());
        wn::PointwiseCombineParams R{};
        R.partial = partial.p;
        R.chain_len = ch.len;
        R.chain0 = Q.chain0;
        R.slab_chains = Q.slab_chains;
        R.num_rows = b.rows;
        R.first = c0 == 0 ? 1 : 0;
        R.last = c0 + nc == k ? 1 : 0;
        R.mask = Q.mask;
        R.state = state.p;
        R.lpd = d_lpd.p + b.out0;
        R.mean = d_mean.p + b.out0;
        R.var = d_var.p + b.out0;
        R.count = d_count.p + b.out0;
        pw.launch_combine(static_cast<int>((N + wn::kPointwiseCombineBlock - 1) / wn::kPointwiseCombineBlock), e->stream, R);
        HIP_OK(hipGetLastError());
      }
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "count goes out as int64");
    HIP_OK(hipMemcpyAsync(lpd, d_lpd.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(mean, d_mean.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(var, d_var.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(count, d_count.p, total * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}

}  // extern "C"
