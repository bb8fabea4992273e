// The one way to launch a kernel: sf_launch<&kernel, LDS_CAP>(name, grid, block, lds_bytes, stream, args...) registers
// the kernel's dynamic-LDS cap with the runtime where it needs one, launches, checks the launch, and returns the
// library's error code.  Host-side; reaches every source through sf_common.h.
#pragma once
#include <atomic>
#include <cstdint>

// ---- layer 1, plain C++ (no HIP: a host program can test it): on which devices a kernel's LDS cap is registered.
// The cap (hipFuncAttributeMaxDynamicSharedMemorySize) is a property of (kernel, device), so each kernel owns one
// record with a bit per device ordinal.  Lock-free: two racing first calls may both register, which is harmless;
// fetch_or loses neither's bit, and the release / acquire pair orders the registration before any launch that relies
// on it.  A failed registration is not recorded, so the next call tries again.  Ordinals outside the record register
// on every call.
struct sf_lds_record {
  static constexpr int DEVICES = 64;
  std::atomic<uint64_t> done{0};
};

// `set` registers the cap on `device` and returns 0 or the runtime's error code, which is passed on
template <typename Set>
inline int sf_lds_register(sf_lds_record& r, int device, Set&& set) {
  const bool tracked = device >= 0 && device < sf_lds_record::DEVICES;
  if (tracked && (r.done.load(std::memory_order_acquire) >> device & 1)) return 0;
  const int rc = set();
  if (rc == 0 && tracked) r.done.fetch_or((uint64_t)1 << device, std::memory_order_release);
  return rc;
}

// ---- layer 2: the launch
#ifdef __HIPCC__
template <auto KERNEL>
inline sf_lds_record sf_lds_record_of;   // one per kernel instantiation

// LDS_CAP: the most dynamic LDS any launch of KERNEL asks for, where that is more than the 64 KiB a kernel may use
// unregistered; 0 otherwise, and then nothing stands in front of the launch.  lds_bytes is what this launch asks for.
template <auto KERNEL, int LDS_CAP = 0, typename... Args>
inline int sf_launch(const char* name, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const Args&... args) {
  if constexpr (LDS_CAP > 64 * 1024) {
    int device = -1;
    hipError_t e = hipGetDevice(&device);
    if (e == hipSuccess)
      e = (hipError_t)sf_lds_register(sf_lds_record_of<KERNEL>, device, [] {
        return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_CAP);
      });
    if (e != hipSuccess) {
      sf_set_error("%s: registering %d bytes of LDS failed: %s", name, LDS_CAP, hipGetErrorString(e));
      return -2;
    }
  }
  hipLaunchKernelGGL(KERNEL, grid, block, lds_bytes, stream, args...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    sf_set_error("%s: launch failed: %s", name, hipGetErrorString(e));
    return -2;
  }
  return 0;
}
#endif
