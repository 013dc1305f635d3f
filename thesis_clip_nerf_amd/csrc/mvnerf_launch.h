// Host-side launch set-up shared by the launch functions: nothing in here is seen by device code.
// "First launch on this device: raise the dynamic-LDS limit of these kernels and remember the CU count."
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <initializer_list>
#include <mutex>

namespace mvnerf {

constexpr int kMaxDevices = 16;

struct KernelLds {
    const void* kernel;         // host address of a __global__ function
    int lds_bytes;              // its hipFuncAttributeMaxDynamicSharedMemorySize
    template <class... Args>
    KernelLds(void (*k)(Args...), int bytes) : kernel(reinterpret_cast<const void*>(k)), lds_bytes(bytes) {}
};

// One per launch function (a function-local static).  device_setup() returns the CU count of the current device in *cus;
// on the first call per device it sets the kernels' dynamic-LDS limits and reads that count (one thread does, the others
// wait for it), afterwards it costs hipGetDevice and one acquire load.  A device index outside the table is
// hipErrorInvalidDevice: launching without the raised limit would fail on the LDS request anyway.
struct DeviceSetup {
    std::atomic<bool> done[kMaxDevices] = {};
    int cus[kMaxDevices] = {};
    std::mutex mtx;
};

inline hipError_t device_setup(DeviceSetup& s, std::initializer_list<KernelLds> kernels, int* cus = nullptr) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    if (!s.done[dev].load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lock(s.mtx);
        if (!s.done[dev].load(std::memory_order_relaxed)) {
            hipDeviceProp_t prop;
            if ((e = hipGetDeviceProperties(&prop, dev)) != hipSuccess) return e;
            s.cus[dev] = prop.multiProcessorCount;
            for (const KernelLds& k : kernels)
                if ((e = hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes)) != hipSuccess) return e;
            s.done[dev].store(true, std::memory_order_release);
        }
    }
    if (cus) *cus = s.cus[dev];
    return hipSuccess;
}

}  // namespace mvnerf
