// Device allocation of the host layer: dev_malloc, through which every allocation goes, and DevBuf, the scoped owner of a
// short-lived one.  Depends on the HIP runtime API and the standard library only, so a host compiler can build it against stubs
// (tests/c_abi/dev_buf_host.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdlib>

// Every device allocation of the host layer goes through dev_malloc.  Debug aid (RSCM_POISON_ALLOC=1 in the environment): it is filled with 0xFF bytes -- NaN as a
// double, -1 as an integer, 255 as a status byte -- so that a kernel or a copy that reads memory nobody wrote shows up as a wrong
// result in the parity tests instead of passing on whatever a fresh allocation happens to hold (usually zeros).  Off by default: one
// fill per allocation.  The GPU tier is run once per round with it on.
namespace rscm {
template <class T>
inline hipError_t dev_malloc(T** p, size_t n)
{
    static const bool poison = [] { const char* e = getenv("RSCM_POISON_ALLOC"); return e && atoi(e) != 0; }();
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(p), n);
    if (e != hipSuccess || !poison || n == 0) return e;
    const hipError_t f = hipMemset(*p, 0xFF, n);
    return f == hipSuccess ? hipDeviceSynchronize() : f;
}

// A device temporary of the host layer: n elements of T from dev_malloc, freed when the owner goes out of scope -- HIPCHK, a
// validation failure or an exception may return past it.  The destructor takes no stream: hipFree waits for the device's
// outstanding work.  A buffer that outlives the call leaves through release() (to a raw handle member) or install().
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.release()) {}
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            (void)hipFree(p_);
            p_ = o.release();
        }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)hipFree(p_); }

    // n elements in place of what the owner held; goes inside HIPCHK
    hipError_t alloc(size_t n)
    {
        (void)hipFree(p_);
        p_ = nullptr;
        return dev_malloc(&p_, n * sizeof(T));
    }
    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    // the caller owns the pointer from here on
    T* release()
    {
        T* p = p_;
        p_ = nullptr;
        return p;
    }
    // "free old, keep new": the slot (a handle member) takes the buffer over and what it held is freed
    void install(T*& slot)
    {
        (void)hipFree(slot);
        slot = release();
    }

private:
    T* p_ = nullptr;
};
}  // namespace rscm
