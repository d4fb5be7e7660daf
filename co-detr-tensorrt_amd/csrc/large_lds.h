// Host helpers the kernels' launchers share, each said once: the opt-in of a kernel that needs more than 64 KB of dynamic
// LDS, and the CU count of the current device (the grid of every persistent kernel).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace {

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the CURRENT device's function object, so it is remembered per
// (device, kernel function) -- a process-wide "already set" flag would skip it when the process moves to a second GPU.
// One table per kernel instantiation (the kernel is the template argument: the fp16 and bf16 forms of a kernel never
// share a flag).  A device ordinal outside the table uses slot 0 and sets the attribute again on every call.  The
// HIP status is the caller's return value.
template <auto Kernel>
hipError_t allow_large_lds(int bytes) {
  static std::atomic<bool> done[64];   // index = device ordinal
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0, done[0].store(false);
  if (done[dev].load(std::memory_order_acquire)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done[dev].store(true, std::memory_order_release);
  return e;
}

// compute units of the current device, asked once per device; 256 (an MI355X) where the runtime does not say
int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

}  // namespace
