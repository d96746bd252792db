// rtu_devbuf.h — host only: DevBuf<T>, the owner of one grow-only device allocation (PinnedBuf<T>: pinned host memory).
// Every buffer a context or the occluder-list builder keeps is one of these: freed by its destructor, and an empty one (what
// a default-constructed owner holds) makes no HIP call at all. Not for the kernels: device structs keep raw pointers.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <utility>

// device allocations made through DevBuf so far, in the whole process (rtu_debug_device_allocations), and the bytes of those still
// held (rtu_debug_device_bytes)
inline std::atomic<unsigned long long> g_devbuf_allocations{0};
inline std::atomic<unsigned long long> g_devbuf_bytes{0};

struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) {
            g_devbuf_allocations++;
            g_devbuf_bytes += bytes;
        }
        return e;
    }
    static void release(void* p, size_t bytes) {
        (void)hipFree(p);
        g_devbuf_bytes -= bytes;
    }
};

struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void* p, size_t) { (void)hipHostFree(p); }
};

template <class T, class Mem = DeviceMem>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // At least n elements: a smaller buffer is freed (its contents are lost) and exactly n are allocated; on failure the
    // buffer is left empty. A large enough one is left as it is.
    hipError_t grow(size_t n) {
        if (n <= n_) return hipSuccess;
        reset();
        void* p = nullptr;
        const hipError_t e = Mem::alloc(&p, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        n_ = n;
        return hipSuccess;
    }
    void reset() {
        if (p_) Mem::release(p_, n_ * sizeof(T));
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }  // capacity, in elements

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <class T>
using PinnedBuf = DevBuf<T, PinnedMem>;
