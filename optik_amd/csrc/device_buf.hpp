// device_buf.hpp -- grow-only owning buffers: device memory (DeviceBuf<T>) and pinned host memory (PinnedBuf<T>).
//
// The workspaces of the kernel layer and of the host API are allocated on first use, grown when a call needs more and
// kept until their owner goes.  reserve(count) is the whole interface: it frees and reallocates (exactly `count`
// elements, contents lost) only when the capacity is too small and never shrinks.  The destructor frees, so an owner
// must be destroyed with the buffers' device current (optik_hip_chain_destroy, optik_robot_free).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace optik {

template <class T, bool Pinned>
class GrowBuf {
public:
    GrowBuf() = default;
    ~GrowBuf() { (void)reset(); }
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;

    T *get() const { return p_; }
    size_t capacity() const { return cap_; }  // elements

    // At least `count` elements.  *grew (if given) tells whether the block was replaced; after a failure the buffer is
    // empty (null, capacity 0).
    hipError_t reserve(size_t count, bool *grew = nullptr) {
        if (grew) *grew = count > cap_;
        if (count <= cap_) return hipSuccess;
        hipError_t e = reset();
        if (e != hipSuccess) return e;
        void *p = nullptr;
        e = Pinned ? hipHostMalloc(&p, sizeof(T) * count) : hipMalloc(&p, sizeof(T) * count);
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(p);
        cap_ = count;
        return hipSuccess;
    }

    // Frees the block (what the destructor does; for a buffer whose size follows another's).
    hipError_t reset() {
        T *p = p_;
        p_ = nullptr;
        cap_ = 0;
        if (!p) return hipSuccess;
        return Pinned ? hipHostFree(p) : hipFree(p);
    }

private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

template <class T> using DeviceBuf = GrowBuf<T, false>;
template <class T> using PinnedBuf = GrowBuf<T, true>;

}  // namespace optik
