// Device-memory basics of the host layer: the error a failed HIP call becomes, and an owning device buffer.
#pragma once
#include <cstddef>
#include <cstdio>
#include <stdexcept>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

namespace dpgo {

// thrown by the host layer when a HIP call fails; the C ABI catches it and returns -1
struct DeviceError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// A failed HIP call never aborts the host process (this is a shared library): it is logged and thrown as
// DeviceError, which every entry point of the C ABI (capi.cpp) turns into the reference's `return -1`.
#define HIP_CHECK(x)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) {                                                                       \
      fprintf(stderr, "[dpgo_amd] ERROR: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      throw DeviceError(hipGetErrorString(e_));                                                   \
    }                                                                                             \
  } while (0)

// After this, DevBuf never calls hipFree again in this process: a stuck RCCL kernel that cannot be aborted would make
// every hipFree wait for ever (comm.cpp: Comm::abandon).
void dev_leak_buffers(bool on);
template <class T>
struct DevBuf {   // (defined and instantiated in group.cpp)
  T *p = nullptr;
  size_t n = 0;
  DevBuf() {}
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release();
  void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); }
  void alloc(size_t count, bool zero = true);
  void upload(const std::vector<T> &h);
  void download(std::vector<T> &h) const;
};

}  // namespace dpgo
