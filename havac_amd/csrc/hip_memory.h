// hip_memory.h -- who frees what: the owners of the HIP memory of libhavac_dev.so's host code, and its one error check.
//
// Internal to havac_dev.hip, havac_pipe.hip, havac_gather.hip and havac_windows.hip (not ABI: include/ holds that).  No other code of theirs
// calls hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipHostRegister / hipHostUnregister: every array below is freed
// once, on every path, by the object that owns it.
#pragma once

#include <cstddef>
#include <string>
#include <utility>

#include <hip/hip_runtime.h>

#include "../../include/havac_dev.h"

namespace havac {

inline std::string hip_msg(const char* what, hipError_t e) { return std::string(what) + ": " + hipGetErrorString(e); }

// `expr` is a HIP call: on failure `err` (a std::string) gets "<expr>: <HIP's message>" and the enclosing function returns
// HAVAC_E_NOMEM (out of memory) or HAVAC_E_RUNTIME
#define HIP_TRY(err, expr)                                                            \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            (err) = ::havac::hip_msg(#expr, _e);                                      \
            return _e == hipErrorOutOfMemory ? HAVAC_E_NOMEM : HAVAC_E_RUNTIME;       \
        }                                                                             \
    } while (0)

// A move-only array of `capacity()` T's (no copies: a move constructor is declared), freed by `Free` when it is destroyed,
// reset or assigned to.
template <typename T, hipError_t (*Free)(void*)>
class HipArray {
public:
    HipArray() = default;
    HipArray(HipArray&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    HipArray& operator=(HipArray&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~HipArray() { reset(); }

    T* get() const { return p_; }
    size_t capacity() const { return n_; }      // elements
    void reset() { if (p_) (void)Free(p_); p_ = nullptr; n_ = 0; }

protected:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// Device memory (hipMalloc).
template <typename T>
class DeviceBuffer : public HipArray<T, hipFree> {
public:
    // Makes room for `want` elements: the old array is freed, a new one allocated.  The contents are not kept.  On failure the
    // buffer is left empty, capacity 0.
    hipError_t grow(size_t want) {
        this->reset();
        T* q = nullptr;
        const hipError_t e = hipMalloc(&q, want * sizeof(T));
        if (e == hipSuccess) { this->p_ = q; this->n_ = want; }
        return e;
    }
    // The same, once `drain` has run dry: work queued there may still use the old array.  (A failed drain frees nothing.)
    hipError_t grow(size_t want, hipStream_t drain) {
        if (const hipError_t e = hipStreamSynchronize(drain); e != hipSuccess) return e;
        return grow(want);
    }
    // Makes room for `want` elements keeping the first `keep_bytes` bytes, copied on `stream`, which is drained.  On failure the
    // buffer is left as it was.
    hipError_t grow_keeping(size_t want, size_t keep_bytes, hipStream_t stream) {
        DeviceBuffer bigger;
        hipError_t e = bigger.grow(want);
        if (e == hipSuccess && keep_bytes) e = hipMemcpyAsync(bigger.get(), this->p_, keep_bytes, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e == hipSuccess) *this = std::move(bigger);
        return e;
    }
    // Exactly `n` elements copied from the host array `src` on `stream` (a temporary: nothing is allocated when n is 0).
    hipError_t copy_from(const T* src, size_t n, hipStream_t stream) {
        this->reset();
        if (n == 0) return hipSuccess;
        hipError_t e = grow(n);
        if (e == hipSuccess) e = hipMemcpyAsync(this->p_, src, n * sizeof(T), hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) this->reset();
        return e;
    }
};

// Pinned host memory (hipHostMalloc).
template <typename T>
class PinnedBuffer : public HipArray<T, hipHostFree> {
public:
    hipError_t allocate(size_t n) {
        this->reset();
        T* q = nullptr;
        const hipError_t e = hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) { this->p_ = q; this->n_ = n; }
        return e;
    }
};

// The pages of a host range locked while it lives (hipHostRegister), so that copies from them run truly asynchronously -- when
// `want` is true; if the pages cannot be locked the copies still work, staged by the runtime, and the HIP error is cleared.
// Before the pages are unlocked `drain()` is called: copies from them may still be in flight (an early error return).
template <typename Drain>
class PageLock {
public:
    PageLock(const void* src, size_t nbytes, bool want, Drain drain) : drain_(std::move(drain)) {
        if (!want) return;
        if (hipHostRegister(const_cast<void*>(src), nbytes, hipHostRegisterDefault) == hipSuccess) p_ = const_cast<void*>(src);
        else (void)hipGetLastError();
    }
    PageLock(const PageLock&) = delete;
    PageLock& operator=(const PageLock&) = delete;
    ~PageLock() {
        if (!p_) return;
        drain_();
        (void)hipHostUnregister(p_);
    }

private:
    void* p_ = nullptr;
    Drain drain_;
};

}  // namespace havac
