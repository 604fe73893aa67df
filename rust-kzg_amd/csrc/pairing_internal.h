// Batched pairing checks on the GPU (pairing.hip), the forms other translation units of the library use: device-resident
// inputs, stream-ordered, no synchronisation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>

#include "../../include/kzg_mi355x.h"

namespace kzgamd {
namespace pairing_gpu {

// checks per launch of the public entry point (kzgamd_pairing_info)
constexpr size_t SLICE = 4096;

// What a launch needs besides its inputs, on ONE device: the program of the Miller loop and the final exponentiation,
// the Frobenius constants (built once per device, never freed) and the line table of a G2 point (68 x (lambda, c) in
// fp28 limb form, from pairing::LineTable; cached per (device, point), kept alive by the shared_ptr while in use).
struct DeviceTable {
    const uint32_t* words = nullptr;  // nullptr: the point at infinity (every pair against it is skipped)
    std::shared_ptr<void> hold;
};
// on the calling thread's current device; hipSuccess or the error of the allocation / copy.  A miss allocates and copies
// synchronously, and so does the FIRST device_table or check_on_stream call on a device (the program and the constants):
// call device_table for both points before the stream-ordered part of a caller begins, as kzg.hip does.
hipError_t device_table(DeviceTable* out, const blst_p2* q);

// ok[i] = e(a1[i], A2) == e(b1[i], B2) for i < count as one byte each, everything device-resident, enqueued on `st` of
// the current device: one wave per check.  The tables must stay alive until the stream has passed the launch.
hipError_t check_on_stream(uint8_t* ok, const blst_p1* a1, const blst_p1* b1, const DeviceTable& ta, const DeviceTable& tb,
                           size_t count, hipStream_t st);

}  // namespace pairing_gpu
}  // namespace kzgamd
