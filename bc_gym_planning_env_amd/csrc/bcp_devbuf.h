// bcp_devbuf.h -- DevBuf<T>: a device buffer that owns its memory, and Owned<>: an event, a stream or a pinned word that does.
// Host code only; a host compiler builds it alone.
//
// The handle's buffers are scratch and derived data: a re-bind with a larger geometry needs more room, a smaller one
// fits into what is there.  So a buffer only ever grows, and growing frees before it allocates -- the contents are not
// kept (nobody relies on them), and the old and the new block never exist side by side.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)reset(); }

    T* get() const { return p_; }
    size_t capacity() const { return cap_; }   // in elements

    // Room for `count` elements.  A request within the capacity changes nothing.  A failure leaves the buffer empty.
    hipError_t reserve(size_t count)
    {
        if (count <= cap_) return hipSuccess;
        hipError_t e = reset();
        if (e != hipSuccess) return e;
        void* p = nullptr;
        e = hipMalloc(&p, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        cap_ = count;
        return hipSuccess;
    }

    hipError_t reset()
    {
        const hipError_t e = p_ ? hipFree(p_) : hipSuccess;
        p_ = nullptr;
        cap_ = 0;
        return e;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// An owned HIP object that is not device memory: created on demand through put(), given back by the destructor (or by the
// next put()).  Move-only.  The handle's objects and the timing events of a call are all of this kind, so no way out of a
// function, and no bcp_destroy, has a line per resource.
template <typename T, hipError_t (*Destroy)(T)>
class Owned {
public:
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : v_(o.v_) { o.v_ = T(); }
    Owned& operator=(Owned&& o) noexcept
    {
        if (this != &o) {
            (void)reset();
            v_ = o.v_;
            o.v_ = T();
        }
        return *this;
    }
    ~Owned() { (void)reset(); }

    T get() const { return v_; }
    explicit operator bool() const { return v_ != T(); }
    T* put()   // for the call that creates the object
    {
        (void)reset();
        return &v_;
    }
    hipError_t reset()
    {
        const hipError_t e = v_ != T() ? Destroy(v_) : hipSuccess;
        v_ = T();
        return e;
    }

private:
    T v_ = T();
};

inline hipError_t bcp_free_pinned_word(uint64_t* p) { return hipHostFree(p); }
using OwnedEvent = Owned<hipEvent_t, hipEventDestroy>;
using OwnedStream = Owned<hipStream_t, hipStreamDestroy>;
using PinnedWord = Owned<uint64_t*, bcp_free_pinned_word>;   // one uint64 of pinned host memory (hipHostMalloc)
