// wn_host.h -- host-side helpers shared by the translation units behind the C ABI (include/walnuts_hip.h):
// the error object, HIP status checks, exception -> error-code mapping, a device buffer.
#ifndef WN_HOST_H
#define WN_HOST_H
#include "wn_hip.h"

#include <sstream>
#include <stdexcept>
#include <string>

#include "../../include/walnuts_hip.h"

// ---- errors (python/src/walnutpie/errors.hpp:10-72) --------------------------------------
struct WalnutpyError {
  std::string msg;
  WalnutpyErrorType type;
};

// Where a wn_chains keeps its draws (wn_summary.hip), for the translation units that read them in kernels of their own
// (wn_engine_log_predictive): chain c's draw i is `dims` doubles at draws + off[c] + i * dims, i < len[c].
struct wn_chains_layout {
  const double* draws;
  const long long* off;  // device [num_chains]
  const int* len;        // device [num_chains]
  const int* host_len;   // host [num_chains]
  size_t num_chains, dims;
  int device;
  hipStream_t stream;    // work queued on the handle's own stream
};
void wn_chains_layout_of(const wn_chains* chains, wn_chains_layout* out);

// (inline and plain templates, not an anonymous namespace: struct wn_engine (wn_engine.h) holds DevBufs and is one type
// across the engine's translation units, and a unit that uses only some of these stays quiet under -Wall)
inline void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) {
    std::stringstream ss;
    ss << "HIP error in " << what << ": " << hipGetErrorString(e);
    throw std::runtime_error(ss.str());
  }
}
#define HIP_OK(expr) hip_check((expr), #expr)

template <class F>
int guarded(WalnutpyError** err, F f) {
  try {
    f();
    return 0;
  } catch (const std::invalid_argument& e) {
    if (err) *err = new WalnutpyError{e.what(), config};
  } catch (const std::exception& e) {
    if (err) *err = new WalnutpyError{e.what(), generic};
  } catch (...) {
    if (err) *err = new WalnutpyError{"Unknown error", generic};
  }
  return -1;
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    release();
    n = count;
    if (count) HIP_OK(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevBuf() { release(); }
};

#endif  // WN_HOST_H
