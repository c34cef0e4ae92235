// wn_probes.hip -- (internal, for the tests) the device maths of wn_devmath.h run on arguments handed in from the host:
// the wn_internal_*_probe entry points and their kernels.  Nothing of the engine is used here.
#include "wn_hip.h"

#include <algorithm>

#include "../../include/walnuts_hip.h"
#include "wn_devrand.h"
#include "wn_traj.h"

#include "wn_host.h"

// (internal, for the tests) wnd::sqrt_normal on the device for arguments handed in from the host
static __global__ void sqrt_probe_kernel(const double* x, double* y, long long n, int checked) {
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x)
    y[i] = checked ? wnd::sqrt_normal<true>(x[i]) : wnd::sqrt_normal<false>(x[i]);
}

// (internal, for the tests) the count models' maths on the device (wnd::dlog1p, dsoftplus, dlgamma_diff, ddigamma_diff)
static __global__ void count_math_probe_kernel(const double* x, const double* phi, double* y, long long n, int fn) {
  const wnd::ArrayTables tab = wnd::array_tables();
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    if (fn == 0) {
      y[i] = wnd::dlog1p(x[i], tab);
    } else if (fn == 1) {
      y[i] = wnd::dsoftplus(x[i], tab);
    } else if (fn == 2) {
      y[i] = wnd::dlgamma_diff(x[i], phi[i], tab);
    } else {
      y[i] = wnd::ddigamma_diff(x[i], phi[i], tab);
    }
  }
}

// (internal, for the tests) the rest of wn_devmath.h on the device, for arguments handed in from the host, under each of
// the three table providers: `tab` 0 ArrayTables, one argument per lane; 1 UniformTab, one argument per wavefront
// iteration (made wave-uniform first), all 64 lanes store their result (out[64 * i + lane]); 2 GatherTab, one argument
// per lane, every lane takes part in every iteration: the last, partial wavefront runs with clamped indices and masks
// only its store.  fn: kProbe* below.  dpow_pos returns early on y, ahead of its table reads, so under the lane tables
// the wavefront shares the y of its first argument.  Launched with whole wavefronts only (blocks of 256).
enum { kProbeExp = 0, kProbeLog, kProbeLogNormal, kProbeExpWeight, kProbePow, kProbeSinCosPi, kProbeSharedDiv,
       kProbeUniform, kProbeNormalPair, kProbeFunctions };
struct MathProbeArgs {
  const double* x;
  const double* y;
  double* o0;
  double* o1;
  long long n;
  int fn;
  unsigned long long seed;
  uint32_t chain, transition, stream, first;
};
template <class Tab>
static __device__ __forceinline__ void math_probe_eval(const MathProbeArgs& A, double x, double y, uint32_t index,
                                                       const Tab& tab, double& r0, double& r1) {
  r0 = r1 = 0.0;
  switch (A.fn) {
    case kProbeExp: r0 = wnd::dexp(x, tab); break;
    case kProbeLog: r0 = wnd::dlog(x, tab); break;
    case kProbeLogNormal: r0 = wnd::dlog_normal(x, tab); break;
    case kProbeExpWeight: r0 = wnd::dexp_weight(x, tab); break;
    case kProbePow: r0 = wnd::dpow_pos(x, y, tab); break;
    case kProbeSinCosPi: wnd::dsincospi(x, r0, r1); break;
    case kProbeSharedDiv: r0 = x / wnd::SharedDivisor(y); break;
    case kProbeUniform: r0 = wnd::stream_uniform(A.seed, A.chain, A.transition, A.stream, index); break;
    default: wnd::stream_normal_pair(A.seed, A.chain, A.transition, A.stream, index, r0, r1, tab); break;
  }
}
template <int TAB>
static __global__ void math_probe_kernel(MathProbeArgs A) {
  const bool reads_x = A.fn < kProbeUniform, reads_y = A.fn == kProbePow || A.fn == kProbeSharedDiv;
  const bool two = A.fn == kProbeSinCosPi || A.fn == kProbeNormalPair;
  const long long thread = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  const long long threads = static_cast<long long>(gridDim.x) * blockDim.x;
  if constexpr (TAB == 0) {
    const wnd::ArrayTables tab = wnd::array_tables();
    for (long long i = thread; i < A.n; i += threads) {
      double r0, r1;
      math_probe_eval(A, reads_x ? A.x[i] : 0.0, reads_y ? A.y[i] : 0.0, A.first + static_cast<uint32_t>(i), tab, r0, r1);
      A.o0[i] = r0;
      if (two) A.o1[i] = r1;
    }
  } else {
    const int lane = wn::opaque_lane_id();
    wn::LaneTables tabs;
    tabs.load(lane);
    const long long wave = thread >> 6, waves = threads >> 6;
    if constexpr (TAB == 1) {
      const wn::UniformTab tab{tabs};
      for (long long i = wave; i < A.n; i += waves) {   // (the bound is wave-uniform: whole wavefronts iterate)
        const double x = wn::uni(reads_x ? A.x[i] : 0.0), y = wn::uni(reads_y ? A.y[i] : 0.0);
        const uint32_t index = static_cast<uint32_t>(wn::uni(static_cast<int>(A.first + static_cast<uint32_t>(i))));
        double r0, r1;
        math_probe_eval(A, x, y, index, tab, r0, r1);
        A.o0[i * 64 + lane] = r0;
        if (two) A.o1[i * 64 + lane] = r1;
      }
    } else {
      const wn::GatherTab tab{tabs};
      for (long long base = wave * 64; base < A.n; base += waves * 64) {
        const long long i = base + lane, ic = i < A.n ? i : A.n - 1;
        const double y = A.fn == kProbePow ? wn::uni(A.y[base]) : (reads_y ? A.y[ic] : 0.0);
        double r0, r1;
        math_probe_eval(A, reads_x ? A.x[ic] : 0.0, y, A.first + static_cast<uint32_t>(ic), tab, r0, r1);
        if (i < A.n) {
          A.o0[i] = r0;
          if (two) A.o1[i] = r1;
        }
      }
    }
  }
}
// (internal, for the tests) the samplers of wn_devrand.h alone: argument i (mu[i], shape[i]) is drawn on the counter
// stream of (row0 + i, draw, chain).  `tab` 0: ArrayTables, one argument per thread, every loop the lane's own (LaneAny);
// 2: GatherTab, one argument per lane, ALL 64 lanes of a wavefront take part in every loop (WaveAny): a last, partial
// wavefront runs with clamped indices -- copies of the last argument on its row -- and masks only its store.  kind:
// wn::kSample*.  shape: the normal's sd, the gamma's shape, the negative binomial's kappa; unread otherwise.
struct SamplerProbeArgs {
  const double* mu;
  const double* shape;
  double* out;
  int* calls;
  long long n;
  int kind;
  unsigned long long seed;
  uint32_t chain, draw, row0;
};
template <class Tab, class Any>
static __device__ __forceinline__ double sampler_probe_eval(int kind, double mu, double shape, wn::RepStream& s,
                                                            const Tab& tab, const Any& any) {
  switch (kind) {   // (wave-uniform)
    case wn::kSampleNormal: return wn::sample_normal(mu, shape, s, tab);
    case wn::kSampleBernoulli: return wn::sample_bernoulli(mu, s);
    case wn::kSamplePoisson: return wn::sample_poisson(mu, s, tab, any);
    case wn::kSampleGamma: return wn::sample_gamma(shape, s, tab, any);
    default: return wn::sample_negbin(mu, shape, s, tab, any);
  }
}
template <int TAB>
static __global__ void sampler_probe_kernel(SamplerProbeArgs A) {
  const long long thread = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x;
  const long long threads = static_cast<long long>(gridDim.x) * blockDim.x;
  if constexpr (TAB == 0) {
    const wnd::ArrayTables tab = wnd::array_tables();
    for (long long i = thread; i < A.n; i += threads) {
      wn::RepStream s{A.seed, A.row0 + static_cast<uint32_t>(i), A.draw, A.chain, 0u};
      A.out[i] = sampler_probe_eval(A.kind, A.mu[i], A.shape[i], s, tab, wn::LaneAny{});
      A.calls[i] = static_cast<int>(s.call);
    }
  } else {
    const int lane = wn::opaque_lane_id();
    wn::LaneTables tabs;
    tabs.load(lane);
    const wn::GatherTab tab{tabs};
    const long long wave = thread >> 6, waves = threads >> 6;
    for (long long base = wave * 64; base < A.n; base += waves * 64) {   // (the bound is wave-uniform)
      const long long i = base + lane, ic = i < A.n ? i : A.n - 1;
      wn::RepStream s{A.seed, A.row0 + static_cast<uint32_t>(ic), A.draw, A.chain, 0u};
      const double y = sampler_probe_eval(A.kind, A.mu[ic], A.shape[ic], s, tab, wn::WaveAny{});
      if (i < A.n) {
        A.out[i] = y;
        A.calls[i] = static_cast<int>(s.call);
      }
    }
  }
}
// (internal, for the tests) raw wnd::philox<7> / <10>: counter words ctr[4 i ..], key words key[2 i ..] -> out[4 i ..]
static __global__ void philox_probe_kernel(const uint32_t* ctr, const uint32_t* key, uint32_t* out, long long n,
                                           int rounds) {
  for (long long i = blockIdx.x * static_cast<long long>(blockDim.x) + threadIdx.x; i < n;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const uint32_t* c = ctr + 4 * i;
    const wnd::U4 r = rounds == 10 ? wnd::philox<10>(c[0], c[1], c[2], c[3], key[2 * i], key[2 * i + 1])
                                   : wnd::philox<7>(c[0], c[1], c[2], c[3], key[2 * i], key[2 * i + 1]);
    out[4 * i] = r.x;
    out[4 * i + 1] = r.y;
    out[4 * i + 2] = r.z;
    out[4 * i + 3] = r.w;
  }
}

extern "C" {

int wn_internal_sqrt_probe(const double* x, double* y, size_t n, int checked) {
  DevBuf<double> dx, dy;
  try {
    dx.alloc(n);
    dy.alloc(n);
    HIP_OK(hipMemcpyAsync(dx.p, x, n * sizeof(double), hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(sqrt_probe_kernel, dim3(1024), dim3(256), 0, nullptr, dx.p, dy.p, static_cast<long long>(n), checked);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(y, dy.p, n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    HIP_OK(hipStreamSynchronize(nullptr));
  } catch (...) {
    return -1;
  }
  return 0;
}

int wn_internal_count_math_probe(const double* x, const double* phi, double* y, size_t n, int fn) {
  DevBuf<double> dx, dp, dy;
  try {
    dx.alloc(n);
    dp.alloc(n);
    dy.alloc(n);
    HIP_OK(hipMemcpyAsync(dx.p, x, n * sizeof(double), hipMemcpyHostToDevice, nullptr));
    HIP_OK(hipMemcpyAsync(dp.p, phi, n * sizeof(double), hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(count_math_probe_kernel, dim3(1024), dim3(256), 0, nullptr, dx.p, dp.p, dy.p,
                       static_cast<long long>(n), fn);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(y, dy.p, n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    HIP_OK(hipStreamSynchronize(nullptr));
  } catch (...) {
    return -1;
  }
  return 0;
}

static int run_math_probe(MathProbeArgs A, const double* x, const double* y, double* out0, double* out1, int tab) {
  if (A.fn < 0 || A.fn >= kProbeFunctions || tab < 0 || tab > 2 || A.n < 0 || out0 == nullptr) return -2;
  if (A.n == 0) return 0;
  const size_t n = static_cast<size_t>(A.n), n_out = tab == 1 ? 64 * n : n;
  const bool reads_x = A.fn < kProbeUniform, reads_y = A.fn == kProbePow || A.fn == kProbeSharedDiv;
  const bool two = A.fn == kProbeSinCosPi || A.fn == kProbeNormalPair;
  if ((reads_x && x == nullptr) || (reads_y && y == nullptr) || (two && out1 == nullptr)) return -2;
  DevBuf<double> dx, dy, d0, d1;
  try {
    if (reads_x) {
      dx.alloc(n);
      HIP_OK(hipMemcpyAsync(dx.p, x, n * sizeof(double), hipMemcpyHostToDevice, nullptr));
    }
    if (reads_y) {
      dy.alloc(n);
      HIP_OK(hipMemcpyAsync(dy.p, y, n * sizeof(double), hipMemcpyHostToDevice, nullptr));
    }
    d0.alloc(n_out);
    if (two) d1.alloc(n_out);
    A.x = dx.p;
    A.y = dy.p;
    A.o0 = d0.p;
    A.o1 = d1.p;
    // whole wavefronts, and no more of them than there is work: one lane per argument (tab 1: one wavefront)
    const size_t work = tab == 1 ? 64 * n : n;
    const dim3 grid(static_cast<unsigned>(std::min<size_t>(1024, (work + 255) / 256))), block(256);
    if (tab == 0) {
      hipLaunchKernelGGL(math_probe_kernel<0>, grid, block, 0, nullptr, A);
    } else if (tab == 1) {
      hipLaunchKernelGGL(math_probe_kernel<1>, grid, block, 0, nullptr, A);
    } else {
      hipLaunchKernelGGL(math_probe_kernel<2>, grid, block, 0, nullptr, A);
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out0, d0.p, n_out * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    if (two) HIP_OK(hipMemcpyAsync(out1, d1.p, n_out * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    HIP_OK(hipStreamSynchronize(nullptr));
  } catch (...) {
    return -1;
  }
  return 0;
}

int wn_internal_math_probe(const double* x, const double* y, double* out0, double* out1, size_t n, int fn, int tab) {
  if (fn > kProbeSharedDiv) return -2;   // (the streams have their own entry point; run_math_probe checks the rest)
  MathProbeArgs A{};
  A.n = static_cast<long long>(n);
  A.fn = fn;
  return run_math_probe(A, x, y, out0, out1, tab);
}

int wn_internal_stream_probe(unsigned long long seed, unsigned int chain, unsigned int transition, unsigned int stream,
                             unsigned int first, size_t n, int normals, int tab, double* out0, double* out1) {
  if (static_cast<unsigned long long>(first) + n > 0x100000000ULL) return -2;
  MathProbeArgs A{};
  A.n = static_cast<long long>(n);
  A.fn = normals ? kProbeNormalPair : kProbeUniform;
  A.seed = seed;
  A.chain = chain;
  A.transition = transition;
  A.stream = stream;
  A.first = first;
  return run_math_probe(A, nullptr, nullptr, out0, out1, tab);
}

int wn_internal_sampler_probe(int kind, const double* mu, const double* shape, unsigned long long seed, unsigned int chain,
                               unsigned int draw, unsigned int row0, size_t n, int tab, double* out, int* calls_out) {
  if (kind < 0 || kind > wn::kSampleNegBin || (tab != 0 && tab != 2) || mu == nullptr || shape == nullptr ||
      out == nullptr || calls_out == nullptr || static_cast<unsigned long long>(row0) + n > 0x100000000ULL)
    return -2;
  if (n == 0) return 0;
  DevBuf<double> dm, ds, dout;
  DevBuf<int> dcalls;
  try {
    dm.alloc(n);
    ds.alloc(n);
    dout.alloc(n);
    dcalls.alloc(n);
    HIP_OK(hipMemcpyAsync(dm.p, mu, n * sizeof(double), hipMemcpyHostToDevice, nullptr));
    HIP_OK(hipMemcpyAsync(ds.p, shape, n * sizeof(double), hipMemcpyHostToDevice, nullptr));
    SamplerProbeArgs A{dm.p, ds.p, dout.p, dcalls.p, static_cast<long long>(n), kind, seed, chain, draw, row0};
    // whole wavefronts, and no more of them than there is work
    const dim3 grid(static_cast<unsigned>(std::min<size_t>(1024, (n + 255) / 256))), block(256);
    if (tab == 0) {
      hipLaunchKernelGGL(sampler_probe_kernel<0>, grid, block, 0, nullptr, A);
    } else {
      hipLaunchKernelGGL(sampler_probe_kernel<2>, grid, block, 0, nullptr, A);
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    HIP_OK(hipMemcpyAsync(calls_out, dcalls.p, n * sizeof(int), hipMemcpyDeviceToHost, nullptr));
    HIP_OK(hipStreamSynchronize(nullptr));
  } catch (...) {
    return -1;
  }
  return 0;
}

int wn_internal_philox_probe(const unsigned int* ctr, const unsigned int* key, unsigned int* out, size_t n, int rounds) {
  if ((rounds != 7 && rounds != 10) || ctr == nullptr || key == nullptr || out == nullptr) return -2;
  if (n == 0) return 0;
  DevBuf<uint32_t> dc, dk, dout;
  try {
    dc.alloc(4 * n);
    dk.alloc(2 * n);
    dout.alloc(4 * n);
    HIP_OK(hipMemcpyAsync(dc.p, ctr, 4 * n * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
    HIP_OK(hipMemcpyAsync(dk.p, key, 2 * n * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(philox_probe_kernel, dim3(static_cast<unsigned>(std::min<size_t>(1024, (n + 255) / 256))),
                       dim3(256), 0, nullptr, dc.p, dk.p, dout.p, static_cast<long long>(n), rounds);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out, dout.p, 4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
    HIP_OK(hipStreamSynchronize(nullptr));
  } catch (...) {
    return -1;
  }
  return 0;
}

}  // extern "C"
