// wn_engine_pointwise.h -- what the entry points that launch pointwise_kernel share (wn_engine_pointwise.hip: log_lik and
// the predictive fold; wn_engine_psis.hip: the matrix of PSIS-LOO).
#ifndef WN_ENGINE_POINTWISE_H
#define WN_ENGINE_POINTWISE_H
#include "wn_engine.h"

#include "wn_pointwise.h"

// the engine's model as the pointwise entry points need it: a data model with the hook, or a `config` error
inline const wn::PointwiseOps& pointwise_ops(const wn_engine* e) {
  const wn::ModelOps& ops = wn::model_ops(e->model);
  if (!ops.uses_data || e->obs.x == nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model: this engine holds no data, there is no pointwise "
                                "log-likelihood to evaluate (create it with wn_engine_create_observed)");
  if (ops.pointwise == nullptr || e->data_const.p == nullptr)
    throw std::invalid_argument(std::string(ops.name) + " model declares no pointwise log-likelihood (wn_model_api.h: "
                                "kPointwise, pointwise(), pointwise_const())");
  return *ops.pointwise;
}
// what both passes hand the kernel about block b; num_items = `units` (parameter vectors, or chains) x the block's tiles
inline wn::PointwiseParams pointwise_params(const wn_engine* e, const RowBlock& b, bool predictive, size_t units) {
  wn::PointwiseParams Q{};
  Q.obs = e->obs;
  Q.row_const = e->data_const.p;
  Q.dim = e->D;
  Q.predictive = predictive ? 1 : 0;
  Q.row0 = b.row0;
  Q.num_rows = b.rows;
  Q.num_tiles = (b.rows + wn::kPointwiseTile - 1) / wn::kPointwiseTile;
  Q.num_items = static_cast<int64_t>(units) * Q.num_tiles;
  return Q;
}

#endif  // WN_ENGINE_POINTWISE_H
