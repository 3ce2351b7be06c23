// spt_devbuf.h -- the one owner of a device allocation on the host side of spt_api.cpp.  Move-only; the destructor frees, so a context, an
// InstScene or a local that goes away takes its device memory with it, and assigning a fresh value to a struct of buffers frees them all.
// Every free is a plain hipFree, which waits for the device: no launch still reads what it releases (the callers rely on that).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

template <typename T>
struct DevBuf {
    T* ptr = nullptr;
    size_t cap = 0;                 // elements grow() made room for (0 after upload(): an uploaded table is replaced, never grown)

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { reset(); ptr = o.ptr; cap = o.cap; o.ptr = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    void reset()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr; cap = 0;
    }

    operator T*() const { return ptr; }

    // Room for `need` elements (nothing to do when it has it): frees, allocates `alloc` elements (by default `need`) and sets the capacity
    // only once the allocation stands.  The contents are not kept; after a failure the buffer is empty.
    hipError_t grow(size_t need, size_t alloc = 0)
    {
        if (need <= cap) return hipSuccess;
        reset();
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, (alloc ? alloc : need) * sizeof(T));
        if (e != hipSuccess) return e;
        ptr = static_cast<T*>(p); cap = need;
        return hipSuccess;
    }

    // Replaces the buffer by a copy of `bytes` host bytes (an empty table still gets 16 bytes, so that its address is valid); blocking.
    // After a failure the buffer is empty.
    hipError_t upload(const void* src, size_t bytes)
    {
        reset();
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, bytes > 16 ? bytes : 16);
        if (e != hipSuccess) return e;
        ptr = static_cast<T*>(p);
        if (bytes && (e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice)) != hipSuccess) reset();
        return e;
    }
};
