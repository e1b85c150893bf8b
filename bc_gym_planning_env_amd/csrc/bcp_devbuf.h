// bcp_devbuf.h -- DevBuf<T>: a device buffer that owns its memory.  Host code only; a host compiler builds it alone.
//
// The handle's buffers are scratch and derived data: a re-bind with a larger geometry needs more room, a smaller one
// fits into what is there.  So a buffer only ever grows, and growing frees before it allocates -- the contents are not
// kept (nobody relies on them), and the old and the new block never exist side by side.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>

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
