// Every entry point of the library runs on the GPU its handle was created on and leaves the caller's
// current device as it found it: one host process can own the 8 GPUs of a node (one settings object /
// MSM handle / NTT handle per device) and call into any of them from any thread.
#pragma once
#include <hip/hip_runtime.h>

namespace kzgamd {

struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            changed = err == hipSuccess;
            // a refused device is reported through `err` only: the runtime's sticky last-error must not fail the
            // next, unrelated call's hipGetLastError() check
            if (!changed) (void)hipGetLastError();
        }
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// The allocator of a handle's staging slots (combine.h: SlotPool): page-locked host memory that kernels on any device
// read and write in place.  NULL on failure, with the runtime's sticky last-error cleared.
struct PinnedMapped {
    int device = 0;  // the handle's
    void* alloc(size_t bytes) const {
        DeviceGuard on_device(device);
        void* p = nullptr;
        if (on_device.err != hipSuccess || hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        return p;
    }
    void free(void* p) const { (void)hipHostFree(p); }
};

}  // namespace kzgamd
