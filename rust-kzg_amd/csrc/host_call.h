// The host side of every layer: the one error type of a failed device call and the one owner of device memory (the MSM
// engine and the c-kzg layer included), and the frames a call and a handle creation run in for the generic handles (Poly,
// ZeroPoly, KZG, FK20, the NTT handle) and the handle-less group multiplication.
// Host-only: nothing here launches a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <mutex>
#include <type_traits>

#include "device_guard.h"

namespace kzgamd {

// a failed device call, in every layer: the code, and what was being done (a string literal, never allocated)
struct DevErr {
    hipError_t e;
    const char* what = "";
};
#define DEV_TRY(x)                                         \
    do {                                                   \
        hipError_t _e = (x);                               \
        if (_e != hipSuccess) throw kzgamd::DevErr{_e, #x}; \
    } while (0)

// what a call returns for a failed HIP call: -(100 + hipError_t)
inline int dev_code(hipError_t e) { return -(100 + (int)e); }

// The one owner of device memory (every handle, every call): `cap` elements of T at `p`, grown when more are asked for,
// freed by drop() or when the owner goes.  Move-only.  Never a member of an object with static storage duration: its
// hipFree would run during the runtime's own teardown.
template <class T>
struct DevArray {
    T* p = nullptr;
    size_t cap = 0;  // elements
    DevArray() = default;
    DevArray(const DevArray&) = delete;
    DevArray& operator=(const DevArray&) = delete;
    DevArray(DevArray&& o) noexcept : p(o.p), cap(o.cap) {
        o.p = nullptr;
        o.cap = 0;
    }
    DevArray& operator=(DevArray&& o) noexcept {
        if (this != &o) {
            drop();
            p = o.p;
            cap = o.cap;
            o.p = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~DevArray() { drop(); }
    // after a failure the array is empty
    void ensure(size_t n) {
        if (n <= cap) return;
        drop();
        void* q = nullptr;
        DEV_TRY(hipMalloc(&q, n * sizeof(T)));
        p = (T*)q;
        cap = n;
    }
    void drop() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class U>
    U* as() const {
        return (U*)p;
    }
};
using DevBuf = DevArray<unsigned char>;  // untyped, counted in bytes

// a group of arrays is released as a whole before any of it is allocated again: the peak while it grows is the new size
template <class... A>
void drop_all(A&... a) {
    (a.drop(), ...);
}

// workspace of one call: freed when the call ends, whichever way
struct ScopedBuf {
    void* p = nullptr;
    ~ScopedBuf() {
        if (p) (void)hipFree(p);
    }
    void alloc(size_t bytes) { DEV_TRY(hipMalloc(&p, bytes ? bytes : 1)); }
    ScopedBuf() = default;
    ScopedBuf(const ScopedBuf&) = delete;
    ScopedBuf& operator=(const ScopedBuf&) = delete;
};

// the stream of one handle-less call: created with the call, drained and destroyed when it ends, whichever way
struct CallStream {
    hipStream_t st = nullptr;
    CallStream() { DEV_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); }
    ~CallStream() {
        if (st) {
            (void)hipStreamSynchronize(st);
            (void)hipStreamDestroy(st);
        }
    }
    CallStream(const CallStream&) = delete;
    CallStream& operator=(const CallStream&) = delete;
};

inline unsigned blocks(size_t total, unsigned per = 256) { return (unsigned)((total + per - 1) / per); }
inline size_t next_pow2(size_t v) {
    size_t n = 1;
    while (n < v) n <<= 1;
    return n;
}

// the status of `body`, which returns nothing (0) or a status of its own: a DevErr it throws becomes dev_code, anything
// else -2.  The whole frame of the calls that have no handle (groupmul.hip: a stream per call).
template <class F>
int status_of(F&& body) {
    try {
        if constexpr (std::is_void_v<decltype(body())>) {
            body();
            return 0;
        } else {
            return body();
        }
    } catch (const DevErr& e) {
        return dev_code(e.e);
    } catch (...) {
        return -2;
    }
}

// one call on a handle (anything with `mu`, `device` and `st`): its lock, its GPU, everything `body` enqueues, one
// synchronisation; the status as status_of gives it
template <class Ctx, class F>
int run_call(Ctx* c, F&& body) {
    std::lock_guard<std::mutex> lk(c->mu);
    return status_of([&]() -> int {
        DeviceGuard on_device(c->device);
        DEV_TRY(on_device.err);
        int rc = 0;
        try {
            if constexpr (std::is_void_v<decltype(body())>) body();
            else rc = body();
        } catch (...) {
            (void)hipStreamSynchronize(c->st);  // a copy into the caller's buffer may be in flight
            throw;
        }
        DEV_TRY(hipStreamSynchronize(c->st));
        return rc;
    });
}

// the creation of a handle that lives on the device of its NTT handle: `init` fills the new Ctx with that device
// current.  When `init` throws: NULL with *err = dev_code for a DevErr and -4 for anything else, the Ctx that did not
// make it deleted with its device current.
template <class Ctx, class F>
Ctx* create_handle(int ntt_device, int* err, F&& init) {
    Ctx* c = nullptr;
    try {
        c = new Ctx();
        DeviceGuard on_device(ntt_device);
        DEV_TRY(on_device.err);
        c->device = ntt_device;
        init(c);
        return c;
    } catch (const DevErr& e) {
        *err = dev_code(e.e);
    } catch (...) {
        *err = -4;
    }
    DeviceGuard on_device(ntt_device);
    delete c;
    return nullptr;
}

}  // namespace kzgamd
