// Owning types of the host side (dsg_api.hip): one move-only owner per HIP resource, released by its destructor.  Every owner converts
// implicitly to the raw handle, so launches and pointer arithmetic read it as before.  No pooling, no counting, no sizes: the call
// sites keep the capacities they already kept.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace dsg {

template <class H, hipError_t (*Release)(H)>
class Owner {
  public:
    Owner() = default;
    Owner(Owner&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Owner& operator=(Owner&& o) noexcept {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
        return *this;
    }
    ~Owner() { reset(); }
    void reset() {
        if (h_) (void)Release(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    operator H() const { return h_; }
    H* put() { reset(); return &h_; }     // the out-parameter of the creating call: hipEventCreate(e.put())

  private:
    H h_ = nullptr;
};

using Stream = Owner<hipStream_t, hipStreamDestroy>;
using Event = Owner<hipEvent_t, hipEventDestroy>;
using GraphExec = Owner<hipGraphExec_t, hipGraphExecDestroy>;

template <class T> hipError_t dev_free(T* p) { return hipFree((void*)p); }
template <class T> hipError_t host_free(T* p) { return hipHostFree((void*)p); }

template <class T>
struct DevBuf : Owner<T*, dev_free<T>> {           // hipMalloc; alloc() on a live buffer frees it first
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(this->put()), n * sizeof(T)); }
};
template <class T>
struct PinnedBuf : Owner<T*, host_free<T>> {       // pinned host memory
    hipError_t alloc(size_t n) { return hipHostMalloc(reinterpret_cast<void**>(this->put()), n * sizeof(T), hipHostMallocDefault); }
};

// Per-call temporary of a stateless entry point: hipMallocAsync on a stream, hipFreeAsync on the same stream when the scope ends
// (behind the kernels enqueued in between).  release() is that free for a caller that reports its error.
template <class T>
class StreamScratch {
  public:
    StreamScratch() = default;
    StreamScratch(const StreamScratch&) = delete;
    StreamScratch& operator=(const StreamScratch&) = delete;
    ~StreamScratch() { (void)release(); }
    hipError_t alloc(size_t n, hipStream_t s) {
        (void)release();
        s_ = s;
        return hipMallocAsync(reinterpret_cast<void**>(&p_), n * sizeof(T), s);
    }
    hipError_t release() {
        const hipError_t e = p_ ? hipFreeAsync(p_, s_) : hipSuccess;
        p_ = nullptr;
        return e;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }

  private:
    T* p_ = nullptr;
    hipStream_t s_ = nullptr;
};

}  // namespace dsg
