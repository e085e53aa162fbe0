// Device allocation of the host layer: dev_malloc, through which every allocation goes, and DevBuf, the one owner of device
// memory -- a call's temporary and a handle's member alike.  Depends on the HIP runtime API and the standard library only, so a
// host compiler can build it against stubs (tests/c_abi/dev_buf_host.cpp).
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

// size() elements of T from dev_malloc, freed when the owner dies: a local goes with its scope -- HIPCHK, a validation failure or
// an exception may return past it -- and a member of a handle, a sampler or a lock-step plan goes with `delete`.  The destructor
// takes no stream: hipFree waits for the device's outstanding work.  Reads as a T* wherever one is expected (a kernel argument, a
// copy, a null test), so only the places that own a buffer name the type.  A buffer moves from a local into a member by
// move-assignment, which frees what the member held: build aside, and move in once nothing can fail any more.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_, n_ = o.n_;
            o.p_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }

    // n fresh elements in place of what the owner held; goes inside HIPCHK.  Empty after a failure
    hipError_t alloc(size_t n)
    {
        reset();
        const hipError_t e = dev_malloc(&p_, n * sizeof(T));
        if (e == hipSuccess) n_ = n;
        else p_ = nullptr;
        return e;
    }
    // room for n elements: what the owner holds if that is enough (contents kept), else alloc(n) (contents gone)
    hipError_t reserve(size_t n) { return n_ >= n ? hipSuccess : alloc(n); }
    void reset()
    {
        (void)hipFree(p_);
        p_ = nullptr, n_ = 0;
    }
    size_t size() const { return n_; }   // in elements
    T* get() const { return p_; }
    operator T*() const { return p_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
}  // namespace rscm
