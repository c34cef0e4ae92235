// wn_kernels.inc -- included through WN_REGISTER_MODEL (wn_model_api.h) with WN_MODEL_TYPE / WN_MODEL_TAG /
// WN_MODEL_ID defined: instantiates the transition and init kernels of one model for every launch geometry and
// enters them into the model registry (wn_launch.h).
#include "wn_hip.h"

#include <stdexcept>

#include "wn_chip.h"
#include "wn_init.h"
#include "wn_launch.h"
#include "wn_pointwise.h"
#include "wn_predict.h"
#include "wn_replicate.h"
#include "wn_traj.h"

#define WN_CAT2(a, b) a##b
#define WN_CAT(a, b) WN_CAT2(a, b)

namespace wn {

// streaming (num_params > 8192) kernels exist for element-wise gradients and for models that state their streaming form
static constexpr bool kHasStreaming = WN_MODEL_TYPE::kElementwise || is_streamable<WN_MODEL_TYPE>::value;
// a data model (kUsesData) runs one wavefront per chain: no kernels are built for wider register geometries
static constexpr bool kUsesData = uses_data<WN_MODEL_TYPE>::value;
static_assert(!(kUsesData && kHasStreaming), "a data model has no streaming form (wn_model_api.h)");
static_assert(!uses_groups<WN_MODEL_TYPE>::value || kUsesData, "kUsesGroups needs kUsesData (wn_model_api.h)");
static_assert(!scale_param<WN_MODEL_TYPE>::value || kUsesData, "kScaleParam needs kUsesData (wn_model_api.h)");
static_assert(!uses_row_terms<WN_MODEL_TYPE>::value || kUsesData, "kUsesRowTerms needs kUsesData (wn_model_api.h)");
static_assert(!varying_slopes<WN_MODEL_TYPE>::value || uses_groups<WN_MODEL_TYPE>::value,
              "kVaryingSlopes needs kUsesGroups (wn_model_api.h)");
static constexpr bool geometry_built(int nw) { return !kUsesData || nw == 1; }
// the pointwise log-likelihood kernels (wn_pointwise.h) exist for data models that declare the hook
static constexpr bool kPointwise = is_pointwise<WN_MODEL_TYPE>::value;
static_assert(!kPointwise || kUsesData, "kPointwise needs kUsesData (wn_model_api.h)");
// ... and the prediction kernels (wn_predict.h)
static constexpr bool kPredict = is_predict<WN_MODEL_TYPE>::value;
static_assert(!kPredict || kUsesData, "kPredict needs kUsesData (wn_model_api.h)");
// ... and the replicate kernels (wn_replicate.h)
static constexpr bool kReplicate = is_replicate<WN_MODEL_TYPE>::value;
static_assert(!kReplicate || kPredict, "kReplicate needs kPredict (wn_model_api.h)");

void WN_CAT(launch_transition_, WN_MODEL_TAG)(const Geometry& g, int grid, size_t smem, hipStream_t stream,
                                               const Params& p) {
  if (g.mem) {
    if constexpr (kHasStreaming) {
#define WN_LAUNCH_MEM(NW, FMA, HOLD) \
  hipLaunchKernelGGL((transition_kernel_mem<WN_MODEL_TYPE, NW, FMA, HOLD>), dim3(grid), dim3(64 * NW), smem, stream, p)
#define WN_X(NW)                                                                  \
  if (g.nw == NW) {                                                               \
    constexpr int kHold = mem_hold_tiles<WN_MODEL_TYPE>(NW);                      \
    if (kHold > 0 && (p.im_in_lds & 4u)) {                                        \
      if (p.fma)                                                                  \
        WN_LAUNCH_MEM(NW, true, kHold);                                           \
      else                                                                        \
        WN_LAUNCH_MEM(NW, false, kHold);                                          \
    } else if (p.fma) {                                                           \
      WN_LAUNCH_MEM(NW, true, 0);                                                 \
    } else {                                                                      \
      WN_LAUNCH_MEM(NW, false, 0);                                                \
    }                                                                             \
    return;                                                                       \
  }
      WN_FOR_EACH_MEM_GEOMETRY(WN_X)
#undef WN_X
    }
    throw std::invalid_argument("this model has no streaming (large num_params) kernel");
  }
#define WN_LAUNCH_CHIP(NW, EPL, WARM, FMA) \
  hipLaunchKernelGGL((transition_kernel_chip<WN_MODEL_TYPE, NW, EPL, WARM, FMA>), dim3(grid), dim3(64 * NW), smem, stream, p)
#define WN_X(NW, EPL)                           \
  if constexpr (geometry_built(NW)) {           \
    if (g.nw == NW && g.epl == EPL) {           \
      if (p.warmup && p.fma)                    \
        WN_LAUNCH_CHIP(NW, EPL, true, true);    \
      else if (p.warmup)                        \
        WN_LAUNCH_CHIP(NW, EPL, true, false);   \
      else if (p.fma)                           \
        WN_LAUNCH_CHIP(NW, EPL, false, true);   \
      else                                      \
        WN_LAUNCH_CHIP(NW, EPL, false, false);  \
      return;                                   \
    }                                           \
  }
  WN_FOR_EACH_GEOMETRY(WN_X)
#undef WN_X
  throw std::invalid_argument("no kernel for this geometry");
}

void WN_CAT(launch_init_, WN_MODEL_TAG)(const Geometry& g, int grid, size_t smem, hipStream_t stream,
                                         const InitParams& q) {
  if (g.mem) {
    if constexpr (kHasStreaming) {
#define WN_X(NW)                                                                                           \
  if (g.nw == NW) {                                                                                        \
    hipLaunchKernelGGL((init_kernel_mem<WN_MODEL_TYPE, NW>), dim3(grid), dim3(64 * NW), smem, stream, q);  \
    return;                                                                                                \
  }
      WN_FOR_EACH_MEM_GEOMETRY(WN_X)
#undef WN_X
    }
    throw std::invalid_argument("this model has no streaming (large num_params) kernel");
  }
#define WN_X(NW, EPL)                                                                                         \
  if constexpr (geometry_built(NW)) {                                                                         \
    if (g.nw == NW && g.epl == EPL) {                                                                         \
      hipLaunchKernelGGL((init_kernel<WN_MODEL_TYPE, NW, EPL>), dim3(grid), dim3(64 * NW), smem, stream, q);  \
      return;                                                                                                 \
    }                                                                                                         \
  }
  WN_FOR_EACH_GEOMETRY(WN_X)
#undef WN_X
  throw std::invalid_argument("no kernel for this geometry");
}

// wn_engine_eval: the model at positions the caller chose (eval_kernel / eval_kernel_mem, wn_init.h)
void WN_CAT(launch_eval_, WN_MODEL_TAG)(const Geometry& g, int grid, size_t smem, hipStream_t stream, bool fma,
                                         const InitParams& q) {
  if (g.mem) {
    if constexpr (kHasStreaming) {
#define WN_X(NW)                                                                                                 \
  if (g.nw == NW) {                                                                                              \
    if (fma)                                                                                                     \
      hipLaunchKernelGGL((eval_kernel_mem<WN_MODEL_TYPE, NW, true>), dim3(grid), dim3(64 * NW), smem, stream, q);  \
    else                                                                                                         \
      hipLaunchKernelGGL((eval_kernel_mem<WN_MODEL_TYPE, NW, false>), dim3(grid), dim3(64 * NW), smem, stream, q); \
    return;                                                                                                      \
  }
      WN_FOR_EACH_MEM_GEOMETRY(WN_X)
#undef WN_X
    }
    throw std::invalid_argument("this model has no streaming (large num_params) kernel");
  }
#define WN_X(NW, EPL)                                                                                              \
  if constexpr (geometry_built(NW)) {                                                                              \
    if (g.nw == NW && g.epl == EPL) {                                                                              \
      if (fma)                                                                                                     \
        hipLaunchKernelGGL((eval_kernel<WN_MODEL_TYPE, NW, EPL, true>), dim3(grid), dim3(64 * NW), smem, stream, q);  \
      else                                                                                                         \
        hipLaunchKernelGGL((eval_kernel<WN_MODEL_TYPE, NW, EPL, false>), dim3(grid), dim3(64 * NW), smem, stream, q); \
      return;                                                                                                      \
    }                                                                                                              \
  }
  WN_FOR_EACH_GEOMETRY(WN_X)
#undef WN_X
  throw std::invalid_argument("no kernel for this geometry");
}

// wn_engine_log_lik / wn_engine_log_predictive: one wavefront per work item, the engine's elements per lane and
// arithmetic mode (pointwise_kernel / pointwise_combine_kernel, wn_pointwise.h).  Instantiated for a model that declares
// the hook only.
namespace {
template <class M, bool kOn = is_pointwise<M>::value>
struct PointwiseLaunch {
  static void launch(const Geometry&, int, hipStream_t, bool, const PointwiseParams&) {}
  static void combine(int, hipStream_t, const PointwiseCombineParams&) {}
  static void consts(const double*, size_t, double*) {}
};
template <class M>
struct PointwiseLaunch<M, true> {
  static void launch(const Geometry& g, int grid, hipStream_t stream, bool fma, const PointwiseParams& q) {
#define WN_X(NW, EPL)                                                                            \
  if constexpr (NW == 1) {                                                                       \
    if (!g.mem && g.nw == 1 && g.epl == EPL) {                                                   \
      if (fma)                                                                                   \
        hipLaunchKernelGGL((pointwise_kernel<M, EPL, true>), dim3(grid), dim3(64), 0, stream, q);  \
      else                                                                                       \
        hipLaunchKernelGGL((pointwise_kernel<M, EPL, false>), dim3(grid), dim3(64), 0, stream, q); \
      return;                                                                                    \
    }                                                                                            \
  }
    WN_FOR_EACH_GEOMETRY(WN_X)
#undef WN_X
    throw std::invalid_argument("no pointwise kernel for this geometry");
  }
  static void combine(int grid, hipStream_t stream, const PointwiseCombineParams& q) {
    hipLaunchKernelGGL((pointwise_combine_kernel<kPointwiseCombineBlock>), dim3(grid), dim3(kPointwiseCombineBlock), 0,
                       stream, q);
  }
  static void consts(const double* y, size_t n, double* out) {
    for (size_t i = 0; i < n; ++i) out[i] = static_cast<double>(M::pointwise_const(y[i]));
  }
};
}  // namespace
void WN_CAT(launch_pointwise_, WN_MODEL_TAG)(const Geometry& g, int grid, hipStream_t stream, bool fma,
                                              const PointwiseParams& q) {
  PointwiseLaunch<WN_MODEL_TYPE>::launch(g, grid, stream, fma, q);
}
void WN_CAT(launch_pointwise_combine_, WN_MODEL_TAG)(int grid, hipStream_t stream, const PointwiseCombineParams& q) {
  PointwiseLaunch<WN_MODEL_TYPE>::combine(grid, stream, q);
}
void WN_CAT(pointwise_consts_, WN_MODEL_TAG)(const double* y, size_t n, double* out) {
  PointwiseLaunch<WN_MODEL_TYPE>::consts(y, n, out);
}
static const PointwiseOps WN_CAT(kPointwiseOps_, WN_MODEL_TAG) = {&WN_CAT(launch_pointwise_, WN_MODEL_TAG),
                                                                  &WN_CAT(launch_pointwise_combine_, WN_MODEL_TAG),
                                                                  &WN_CAT(pointwise_consts_, WN_MODEL_TAG)};

// wn_engine_predict / wn_engine_predict_fold / wn_engine_predict_chains: one wavefront per work item, the engine's
// elements per lane and arithmetic mode (predict_kernel / predict_combine_kernel, wn_predict.h).  Instantiated for a
// model that declares the hook only.
namespace {
template <class M, bool kOn = is_predict<M>::value>
struct PredictLaunch {
  static void launch(const Geometry&, int, hipStream_t, bool, const PredictParams&) {}
  static void combine(int, hipStream_t, const PredictCombineParams&) {}
};
template <class M>
struct PredictLaunch<M, true> {
  static void launch(const Geometry& g, int grid, hipStream_t stream, bool fma, const PredictParams& q) {
#define WN_X(NW, EPL)                                                                          \
  if constexpr (NW == 1) {                                                                     \
    if (!g.mem && g.nw == 1 && g.epl == EPL) {                                                 \
      if (fma)                                                                                 \
        hipLaunchKernelGGL((predict_kernel<M, EPL, true>), dim3(grid), dim3(64), 0, stream, q);  \
      else                                                                                     \
        hipLaunchKernelGGL((predict_kernel<M, EPL, false>), dim3(grid), dim3(64), 0, stream, q); \
      return;                                                                                  \
    }                                                                                          \
  }
    WN_FOR_EACH_GEOMETRY(WN_X)
#undef WN_X
    throw std::invalid_argument("no predict kernel for this geometry");
  }
  static void combine(int grid, hipStream_t stream, const PredictCombineParams& q) {
    hipLaunchKernelGGL((predict_combine_kernel<kPointwiseCombineBlock>), dim3(grid), dim3(kPointwiseCombineBlock), 0,
                       stream, q);
  }
};
}  // namespace
void WN_CAT(launch_predict_, WN_MODEL_TAG)(const Geometry& g, int grid, hipStream_t stream, bool fma,
                                            const PredictParams& q) {
  PredictLaunch<WN_MODEL_TYPE>::launch(g, grid, stream, fma, q);
}
void WN_CAT(launch_predict_combine_, WN_MODEL_TAG)(int grid, hipStream_t stream, const PredictCombineParams& q) {
  PredictLaunch<WN_MODEL_TYPE>::combine(grid, stream, q);
}
static const PredictOps WN_CAT(kPredictOps_, WN_MODEL_TAG) = {&WN_CAT(launch_predict_, WN_MODEL_TAG),
                                                              &WN_CAT(launch_predict_combine_, WN_MODEL_TAG)};

// wn_engine_replicate / wn_engine_replicate_chains / wn_engine_replicate_check: one wavefront per work item, the engine's
// elements per lane and arithmetic mode (replicate_kernel, wn_replicate.h).  Instantiated for a model that declares the
// hook only.
namespace {
template <class M, bool kOn = is_replicate<M>::value>
struct ReplicateLaunch {
  static void launch(const Geometry&, int, hipStream_t, bool, const ReplicateParams&) {}
};
template <class M>
struct ReplicateLaunch<M, true> {
  static void launch(const Geometry& g, int grid, hipStream_t stream, bool fma, const ReplicateParams& q) {
#define WN_X(NW, EPL)                                                                            \
  if constexpr (NW == 1) {                                                                       \
    if (!g.mem && g.nw == 1 && g.epl == EPL) {                                                   \
      if (fma)                                                                                   \
        hipLaunchKernelGGL((replicate_kernel<M, EPL, true>), dim3(grid), dim3(64), 0, stream, q);  \
      else                                                                                       \
        hipLaunchKernelGGL((replicate_kernel<M, EPL, false>), dim3(grid), dim3(64), 0, stream, q); \
      return;                                                                                    \
    }                                                                                            \
  }
    WN_FOR_EACH_GEOMETRY(WN_X)
#undef WN_X
    throw std::invalid_argument("no replicate kernel for this geometry");
  }
};
}  // namespace
void WN_CAT(launch_replicate_, WN_MODEL_TAG)(const Geometry& g, int grid, hipStream_t stream, bool fma,
                                              const ReplicateParams& q) {
  ReplicateLaunch<WN_MODEL_TYPE>::launch(g, grid, stream, fma, q);
}
static const ReplicateOps WN_CAT(kReplicateOps_, WN_MODEL_TAG) = {&WN_CAT(launch_replicate_, WN_MODEL_TAG)};

void WN_CAT(prepare_, WN_MODEL_TAG)(const Geometry& g, size_t smem) {
  if (g.mem) {
    if constexpr (!kHasStreaming) {
      throw std::invalid_argument("this model has no streaming (large num_params) kernel");
    } else {
      // (the inverse mass parked in LDS can take the dynamic part beyond the default limit)
#define WN_SET_SMEM_MEM(NW, FMA, HOLD)                                                                       \
  if (e == hipSuccess)                                                                                       \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&transition_kernel_mem<WN_MODEL_TYPE, NW, FMA, HOLD>), \
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem));
#define WN_X(NW)                                                                                                \
  if (g.nw == NW) {                                                                                             \
    constexpr int kHold = mem_hold_tiles<WN_MODEL_TYPE>(NW);                                                    \
    hipError_t e = hipSuccess;                                                                                  \
    WN_SET_SMEM_MEM(NW, true, 0)                                                                                \
    WN_SET_SMEM_MEM(NW, false, 0)                                                                               \
    if (kHold > 0) {                                                                                            \
      WN_SET_SMEM_MEM(NW, true, kHold)                                                                          \
      WN_SET_SMEM_MEM(NW, false, kHold)                                                                         \
    }                                                                                                           \
    if (e != hipSuccess) throw std::runtime_error(std::string("hipFuncSetAttribute: ") + hipGetErrorString(e)); \
    return;                                                                                                     \
  }
      WN_FOR_EACH_MEM_GEOMETRY(WN_X)
#undef WN_X
    }
    return;
  }
#define WN_SET_SMEM(NW, EPL, WARM, FMA)                                                                   \
  if (e == hipSuccess)                                                                                    \
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&transition_kernel_chip<WN_MODEL_TYPE, NW, EPL, WARM, FMA>), \
                            hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem));
#define WN_X(NW, EPL)                                                                                         \
  if constexpr (geometry_built(NW)) {                                                                         \
    if (g.nw == NW && g.epl == EPL) {                                                                         \
      hipError_t e = hipSuccess;                                                                              \
      WN_SET_SMEM(NW, EPL, true, true)                                                                        \
      WN_SET_SMEM(NW, EPL, true, false)                                                                       \
      WN_SET_SMEM(NW, EPL, false, true)                                                                       \
      WN_SET_SMEM(NW, EPL, false, false)                                                                      \
      if (e != hipSuccess) throw std::runtime_error(std::string("hipFuncSetAttribute: ") + hipGetErrorString(e)); \
      return;                                                                                                 \
    }                                                                                                         \
  }
  WN_FOR_EACH_GEOMETRY(WN_X)
#undef WN_X
  throw std::invalid_argument("no kernel for this geometry");
}

int WN_CAT(waves_per_simd_, WN_MODEL_TAG)(const Geometry& g) {
  if (g.mem) return 8;
#define WN_X(NW, EPL) \
  if (g.nw == NW && g.epl == EPL) return chip_waves_per_simd<WN_MODEL_TYPE, EPL>();
  WN_FOR_EACH_GEOMETRY(WN_X)
#undef WN_X
  throw std::invalid_argument("no kernel for this geometry");
}

namespace {
template <class M>
auto call_host_params(double* p, int n, int) -> decltype(M::host_params(p, n), void()) { M::host_params(p, n); }
template <class M>
void call_host_params(double*, int, long) {}
// (a model with varying slopes takes num_varying as a third argument, and is called through this one only)
template <class M>
auto call_host_params_varying(double* p, int n, int q, int) -> decltype(M::host_params(p, n, q), void()) {
  M::host_params(p, n, q);
}
template <class M>
void call_host_params_varying(double*, int, int, long) {}
template <class M>
auto call_validate(int n, int) -> decltype(M::validate(n), void()) { M::validate(n); }
template <class M>
void call_validate(int, long) {}
// the model's geometry hint (wn_model_api.h): a function of num_params, or a constant, or none
template <class M>
constexpr auto preferred_epl_of(int n, int, int) -> decltype(M::preferred_elems_per_lane(n), 0) {
  return M::preferred_elems_per_lane(n);
}
template <class M>
constexpr auto preferred_epl_of(int, int, long) -> decltype(M::kPreferredElemsPerLane, 0) { return M::kPreferredElemsPerLane; }
template <class M>
constexpr int preferred_epl_of(int, long, long) { return 0; }
int WN_CAT(preferred_epl_, WN_MODEL_TAG)(int num_params) { return preferred_epl_of<WN_MODEL_TYPE>(num_params, 0, 0); }
int WN_CAT(hold_tiles_, WN_MODEL_TAG)(int nw) {
#define WN_X(NW) \
  if (nw == NW) return mem_hold_tiles<WN_MODEL_TYPE>(NW);
  WN_FOR_EACH_MEM_GEOMETRY(WN_X)
#undef WN_X
  return 0;
}
void WN_CAT(host_params_, WN_MODEL_TAG)(double* p, int n) { call_host_params<WN_MODEL_TYPE>(p, n, 0); }
void WN_CAT(host_params_varying_, WN_MODEL_TAG)(double* p, int n, int q) {
  call_host_params_varying<WN_MODEL_TYPE>(p, n, q, 0);
}
void WN_CAT(validate_, WN_MODEL_TAG)(int n) { call_validate<WN_MODEL_TYPE>(n, 0); }
// (a model whose checks depend on whether the engine carries weights takes the flag as a fifth argument)
template <class M>
auto call_host_data(const double* x, const double* y, int n, int d, bool w, int, int)
    -> decltype(M::host_data(x, y, n, d, w), void()) {
  M::host_data(x, y, n, d, w);
}
template <class M>
auto call_host_data(const double* x, const double* y, int n, int d, bool, int, long)
    -> decltype(M::host_data(x, y, n, d), void()) {
  M::host_data(x, y, n, d);
}
template <class M>
void call_host_data(const double*, const double*, int, int, bool, long, long) {}
void WN_CAT(host_data_, WN_MODEL_TAG)(const double* x, const double* y, int n, int d, bool weighted) {
  call_host_data<WN_MODEL_TYPE>(x, y, n, d, weighted, 0, 0);
}
}  // namespace

#define WN_STR2(x) #x
#define WN_STR(x) WN_STR2(x)
static const ModelOps WN_CAT(kOps_, WN_MODEL_TAG) = {
    WN_MODEL_ID,
    WN_STR(WN_MODEL_TAG),
    WN_MODEL_TYPE::kUsesParams,
    kHasStreaming,
    &WN_CAT(preferred_epl_, WN_MODEL_TAG),
    &WN_CAT(launch_transition_, WN_MODEL_TAG),
    &WN_CAT(launch_init_, WN_MODEL_TAG),
    &WN_CAT(prepare_, WN_MODEL_TAG),
    &WN_CAT(waves_per_simd_, WN_MODEL_TAG),
    &WN_CAT(host_params_, WN_MODEL_TAG),
    &WN_CAT(validate_, WN_MODEL_TAG),
    &WN_CAT(hold_tiles_, WN_MODEL_TAG),
    mem_register_dim_limit<WN_MODEL_TYPE>(),
    kUsesData,
    &WN_CAT(launch_eval_, WN_MODEL_TAG),
    &WN_CAT(host_data_, WN_MODEL_TAG),
    uses_groups<WN_MODEL_TYPE>::value,
    scale_param<WN_MODEL_TYPE>::value,
    uses_row_terms<WN_MODEL_TYPE>::value,
    kPointwise ? &WN_CAT(kPointwiseOps_, WN_MODEL_TAG) : nullptr,
    kPredict ? &WN_CAT(kPredictOps_, WN_MODEL_TAG) : nullptr,
    kReplicate ? &WN_CAT(kReplicateOps_, WN_MODEL_TAG) : nullptr,
    varying_slopes<WN_MODEL_TYPE>::value ? &WN_CAT(host_params_varying_, WN_MODEL_TAG) : nullptr};
static const bool WN_CAT(kRegistered_, WN_MODEL_TAG) = register_model(&WN_CAT(kOps_, WN_MODEL_TAG));

}  // namespace wn

#if defined(WN_TIMELINE)
// probe build only (tests/gpu_probes/timeline.py): workgroup 0's (clock << 6 | mark) records of the last launch
extern "C" __attribute__((visibility("default"))) void WN_CAT(wn_debug_timeline_, WN_MODEL_TAG)(
    unsigned long long* out, int n) {
  static unsigned long long h[wn::kTimelineMarks];
  (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(wn::wn_timeline), sizeof(h));
  for (int i = 0; i < n && i < wn::kTimelineMarks; ++i) out[i] = h[i];
}
#endif
#if defined(WN_COUNT_POOL)
// probe build only (tests/gpu_probes/pool_traffic.py): the span pool's traffic counters, read and cleared
extern "C" __attribute__((visibility("default"))) void WN_CAT(wn_debug_pool_counts_, WN_MODEL_TAG)(unsigned long long* out) {
  unsigned long long zero[5] = {0, 0, 0, 0, 0};
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(wn::wn_pool_counts), sizeof(zero));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(wn::wn_pool_counts), zero, sizeof(zero));
}
#endif
