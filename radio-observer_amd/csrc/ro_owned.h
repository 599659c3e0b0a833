// ro_owned.h -- the one owner of a block of device memory (hipMalloc) or pinned host memory (hipHostMalloc): pointer and
// element count, freed by reset() and by the destructor, move-only.  It converts to T *, so that whoever only uses the
// block (the argument fillers, `if (!h->d_x)`) reads as with a raw pointer; allocation, upload and release go through here.
// Nothing is pooled, counted or deferred: the same hipMalloc / hipHostMalloc / hipFree / hipHostFree at the moment of the call.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

namespace ro {
namespace host {

template <typename T, bool PINNED>
class Owned {
public:
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~Owned() { reset(); }

    operator T *() const { return p_; }
    size_t count() const { return n_; }

    void reset()
    {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    // n elements, uninitialised; whatever was held goes first (the caller has waited for its last user)
    hipError_t alloc(size_t n)
    {
        reset();
        void *q = nullptr;
        const hipError_t e = PINNED ? hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&q, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(q);
        n_ = n;
        return hipSuccess;
    }
    // alloc(n) and a blocking copy of n elements from host memory
    hipError_t upload(const T *src, size_t n)
    {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

template <typename T> using DeviceBlock = Owned<T, false>;
template <typename T> using PinnedBlock = Owned<T, true>;      // (alloc only: nothing uploads into host memory)

}  // namespace host
}  // namespace ro
