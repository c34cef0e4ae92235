// wn_engine_psis.hip -- PSIS-LOO on the engine's observation block (wn_psis.h): wn_engine_psis_loo, per row the
// leave-one-out log predictive density by Pareto-smoothed importance sampling and the Pareto shape of its ratios, over
// the draws of a wn_chains.  Stage 1 is pointwise_kernel's matrix mode, stage 2 psis_row_kernel.
#include "wn_engine_pointwise.h"

#include "wn_psis.h"

namespace {
// what the row kernel is told about a block of S draws: M = min(floor(S / 5), ceil(3 sqrt(S))) and m = 30 +
// floor(sqrt(M)) in integers, M's power of two, the position of the fit's quartile
struct PsisSizes {
  int64_t tail, candidates, padded, quartile;
};
int64_t floor_sqrt(int64_t v) {
  int64_t r = static_cast<int64_t>(std::sqrt(static_cast<double>(v)));
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}
PsisSizes psis_sizes(int64_t S) {
  const int64_t root = floor_sqrt(9 * S);                       // ceil(3 sqrt(S)) = ceil(sqrt(9 S))
  const int64_t three_roots = root * root == 9 * S ? root : root + 1;
  PsisSizes z{};
  z.tail = std::min(S / 5, three_roots);
  z.candidates = 30 + floor_sqrt(z.tail);
  z.padded = 1;
  while (z.padded < z.tail) z.padded *= 2;
  z.quartile = (z.tail + 2) / 4 - 1;                            // floor(M / 4 + 0.5), 1-based
  return z;
}
constexpr size_t kPsisDefaultWorkspace = size_t{1} << 30;
// a block's chains and their first columns: draw0 [num_chains] (restarting at every block), draws [G]
void block_columns(const wn_chains_layout& ch, size_t G, std::vector<long long>& draw0, std::vector<int64_t>& draws) {
  const size_t k = ch.num_chains / G;
  draw0.assign(ch.num_chains, 0);
  draws.assign(G, 0);
  for (size_t g = 0; g < G; ++g)
    for (size_t c = g * k; c < (g + 1) * k; ++c) {
      draw0[c] = draws[g];
      draws[g] += ch.host_len[c];
    }
}
void check_chains(const wn_engine* e, const wn_chains_layout& ch) {
  if (ch.dims != static_cast<size_t>(e->D))
    throw std::invalid_argument("the chains hold draws of " + std::to_string(ch.dims) + " dimensions, the engine's model has " +
                                std::to_string(e->D) + " parameters");
  const size_t G = static_cast<size_t>(e->num_datasets);
  if (ch.num_chains % G != 0)
    throw std::invalid_argument("the number of chains (" + std::to_string(ch.num_chains) + ") must be a multiple of the "
                                "engine's datasets / weight sets (" + std::to_string(G) + "): block g of the chains is "
                                "scored on dataset g");
  if (ch.device != e->device) throw std::invalid_argument("the chains live on another device than the engine");
}
// stage 1 for the rows `part` of a block and the chains [chain0, chain0 + k): lmat [part.rows][ld]
wn::PointwiseParams launch_matrix(wn_engine* e, const wn::PointwiseOps& pw, const wn_chains_layout& ch, size_t chain0, size_t k,
                                  const RowBlock& part, const uint8_t* mask, double* lmat, size_t ld, const long long* draw0) {
  wn::PointwiseParams Q = pointwise_params(e, part, /*predictive=*/true, k);
  Q.predictive = wn::kPointwiseMatrix;
  Q.draws = ch.draws;
  Q.chain_off = ch.off;
  Q.chain_len = ch.len;
  Q.chain0 = static_cast<int32_t>(chain0);
  Q.slab_chains = static_cast<int32_t>(k);
  Q.mask = mask;
  Q.out = lmat;
  Q.draw0 = draw0;
  Q.ld = static_cast<int64_t>(ld);
  pw.launch(e->geo, pointwise_grid(Q.num_items), e->stream, e->cfg.fused_multiply_add != 0, Q);
  HIP_OK(hipGetLastError());
  return Q;
}
}  // namespace

extern "C" {

int wn_engine_psis_loo(wn_engine* e, wn_chains* chains, const uint8_t* row_mask, size_t workspace_bytes, double* elpd_loo,
                       double* pareto_k, double* ess, double* lpd, int64_t* count, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || chains == nullptr || elpd_loo == nullptr || pareto_k == nullptr || ess == nullptr || lpd == nullptr ||
        count == nullptr)
      throw std::invalid_argument("null argument");
    const wn::PointwiseOps& pw = pointwise_ops(e);
    wn_chains_layout ch{};
    wn_chains_layout_of(chains, &ch);
    check_chains(e, ch);
    const size_t G = static_cast<size_t>(e->num_datasets);
    const size_t k = ch.num_chains / G;
    // per block: its draws S (the chains' lengths), each chain's first column, and the sizes the row kernel takes
    std::vector<long long> draw0;
    std::vector<int64_t> draws;
    block_columns(ch, G, draw0, draws);
    for (size_t g = 0; g < G; ++g) {
      if (draws[g] < 1) throw std::invalid_argument("block " + std::to_string(g) + " of the chains holds no draw");
      const PsisSizes z = psis_sizes(draws[g]);
      if (z.tail > wn::kPsisMaxTail)
        throw std::invalid_argument("PSIS-LOO sorts the tail of a row's importance ratios on chip: " + std::to_string(z.tail) +
                                    " of the block's " + std::to_string(draws[g]) + " draws, and at most " +
                                    std::to_string(wn::kPsisMaxTail) + " (1864135 draws) are supported; keep fewer draws "
                                    "(thin=)");
    }
    e->use_device();
    HIP_OK(hipStreamSynchronize(ch.stream));  // (uploads queued on the handle's own stream)
    const std::vector<int64_t> offsets = host_offsets(e);
    const bool sets = e->obs.chains_per_dataset > 0 && e->obs.offsets == nullptr;
    const size_t total = sets ? G * static_cast<size_t>(e->obs.num_obs) : e->data_rows;
    DevBuf<double> d_elpd, d_k, d_ess, d_lpd, lmat;
    DevBuf<long long> d_count, d_draw0;
    DevBuf<uint8_t> d_mask;
    d_elpd.alloc(total);
    d_k.alloc(total);
    d_ess.alloc(total);
    d_lpd.alloc(total);
    d_count.alloc(total);
    d_draw0.alloc(draw0.size());
    HIP_OK(hipMemcpyAsync(d_draw0.p, draw0.data(), draw0.size() * sizeof(long long), hipMemcpyHostToDevice, e->stream));
    if (row_mask != nullptr) {
      d_mask.alloc(total);
      HIP_OK(hipMemcpyAsync(d_mask.p, row_mask, total, hipMemcpyHostToDevice, e->stream));
    }
    // the matrix of one SLAB of rows at a time (a multiple of 64 rows, one tile at least): a row's result depends on its
    // own column alone, so the workspace's size changes nothing
    const size_t budget = workspace_bytes != 0 ? workspace_bytes : kPsisDefaultWorkspace;
    for (size_t g = 0; g < G; ++g) {
      const RowBlock b = row_block(e, offsets, static_cast<int>(g));
      const size_t N = static_cast<size_t>(b.rows), S = static_cast<size_t>(draws[g]);
      const size_t ld = (S + 7) / 8 * 8;  // columns start on 64-byte lines
      const size_t tile = wn::kPointwiseTile;
      const size_t slab = std::min((N + tile - 1) / tile * tile, std::max<size_t>(1, budget / (ld * sizeof(double) * tile)) * tile);
      if (lmat.n < slab * ld) lmat.alloc(slab * ld);
      const PsisSizes z = psis_sizes(draws[g]);
      for (size_t r0 = 0; r0 < N; r0 += slab) {
        const size_t rows = std::min(slab, N - r0);
        const RowBlock part{b.row0 + static_cast<int64_t>(r0), b.out0 + static_cast<int64_t>(r0), static_cast<int32_t>(rows)};
        const wn::PointwiseParams Q = launch_matrix(e, pw, ch, g * k, k, part, row_mask != nullptr ? d_mask.p + part.out0 : nullptr,
                                                    lmat.p, ld, d_draw0.p);
        wn::PsisParams R{};
        R.lmat = lmat.p;
        R.ld = Q.ld;
        R.num_rows = part.rows;
        R.num_draws = static_cast<int32_t>(S);
        R.tail = static_cast<int32_t>(z.tail);
        R.candidates = static_cast<int32_t>(z.candidates);
        R.tail_padded = static_cast<int32_t>(z.padded);
        R.quartile = static_cast<int32_t>(z.quartile);
        R.mask = Q.mask;
        R.elpd_loo = d_elpd.p + part.out0;
        R.pareto_k = d_k.p + part.out0;
        R.ess = d_ess.p + part.out0;
        R.lpd = d_lpd.p + part.out0;
        R.count = d_count.p + part.out0;
        hipLaunchKernelGGL(wn::psis_row_kernel, dim3(pointwise_grid(part.rows)), dim3(wn::kPsisBlock), 0, e->stream, R);
        HIP_OK(hipGetLastError());
      }
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "count goes out as int64");
    HIP_OK(hipMemcpyAsync(elpd_loo, d_elpd.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(pareto_k, d_k.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(ess, d_ess.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(lpd, d_lpd.p, total * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipMemcpyAsync(count, d_count.p, total * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}

// (internal, tests) stage 1 alone: out [rows of the block][num_draws] (host), the matrix of block `dataset` in one slab
int wn_internal_psis_matrix(wn_engine* e, wn_chains* chains, int dataset, size_t num_draws, double* out, WalnutpyError** err) {
  return guarded(err, [&] {
    if (e == nullptr || chains == nullptr || out == nullptr) throw std::invalid_argument("null argument");
    const wn::PointwiseOps& pw = pointwise_ops(e);
    wn_chains_layout ch{};
    wn_chains_layout_of(chains, &ch);
    check_chains(e, ch);
    const size_t G = static_cast<size_t>(e->num_datasets), k = ch.num_chains / G;
    if (dataset < 0 || static_cast<size_t>(dataset) >= G) throw std::invalid_argument("dataset must be in [0, wn_engine_num_datasets)");
    std::vector<long long> draw0;
    std::vector<int64_t> draws;
    block_columns(ch, G, draw0, draws);
    if (static_cast<size_t>(draws[dataset]) != num_draws)
      throw std::invalid_argument("the block holds " + std::to_string(draws[dataset]) + " draws, not " + std::to_string(num_draws));
    e->use_device();
    HIP_OK(hipStreamSynchronize(ch.stream));
    const RowBlock b = row_block(e, host_offsets(e), dataset);
    const size_t N = static_cast<size_t>(b.rows), S = static_cast<size_t>(draws[dataset]);
    DevBuf<double> lmat;
    DevBuf<long long> d_draw0;
    lmat.alloc(N * S);
    d_draw0.alloc(draw0.size());
    HIP_OK(hipMemcpyAsync(d_draw0.p, draw0.data(), draw0.size() * sizeof(long long), hipMemcpyHostToDevice, e->stream));
    launch_matrix(e, pw, ch, static_cast<size_t>(dataset) * k, k, b, nullptr, lmat.p, S, d_draw0.p);
    HIP_OK(hipMemcpyAsync(out, lmat.p, N * S * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  });
}

}  // extern "C"
