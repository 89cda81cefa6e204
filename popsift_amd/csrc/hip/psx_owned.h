// psx_owned.h -- the resource owners of a psx_ctx (api.hip).  Every owner is move-only and empty by default; an empty
// owner's destructor makes no HIP call, so a context that never reached a device can be deleted.  They free, they do not
// decide when: the caller waits for the stream before it replaces a buffer a frame in flight may read (Staged::reserve is
// the one place that does so itself).
#pragma once

#include <hip/hip_runtime.h>
#include <cstring>
#include <utility>

// one HIP handle and the call that destroys it
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;

    Handle() = default;
    Handle(Handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { reset(); }
    void reset() { if (h) { (void)Destroy(h); h = nullptr; } }
    operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;
// an event created on first use
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t get(unsigned flags) { return h ? hipSuccess : hipEventCreateWithFlags(&h, flags); }
};

// cap elements of device memory (DevBuf) or of pinned host memory (PinnedBuf)
template <class T, bool Pinned>
struct Buf {
    T*     p = nullptr;
    size_t cap = 0;

    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Buf() { if (p) (void)release(); }

    // nothing when the buffer holds `need` elements already; otherwise free, then allocate (the contents are not kept).
    // slack: elements allocated beyond the recorded capacity
    hipError_t grow(size_t need, size_t slack = 0)
    {
        if (need <= cap && p) return hipSuccess;
        if (p) { const hipError_t e = release(); if (e != hipSuccess) return e; }
        const size_t bytes = (need + slack) * sizeof(T);
        const hipError_t e = Pinned ? hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocDefault)
                                    : hipMalloc(reinterpret_cast<void**>(&p), bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = need;
        return hipSuccess;
    }
    hipError_t release()
    {
        const hipError_t e = Pinned ? hipHostFree(p) : hipFree(p);
        if (e == hipSuccess) { p = nullptr; cap = 0; }
        return e;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

// The device copy of caller data in pageable host memory, made through a pinned staging block: hipMemcpyAsync from
// pageable memory took 4.9 ms for a 2 MB frame (measured), a host memcpy + DMA from pinned memory takes ~0.1 ms.
template <class T>
struct Staged {
    DevBuf<T>    dev;
    PinnedBuf<T> stage;
    Event        done;         // the DMA out of `stage` has finished

    // a device copy that holds n elements; a new one gets dev_room (+ slack) after the stream has drained: a frame in
    // flight may still read the old one
    hipError_t reserve(size_t n, size_t dev_room, size_t slack, hipStream_t s)
    {
        if (n <= dev.cap) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(s);
        return e != hipSuccess ? e : dev.grow(dev_room, slack);
    }
    // n elements of host memory to the device copy, on s.  dev_room / stage_room: sizes of a new device copy / staging
    // block (>= n: the caller's headroom).  dma = false leaves the DMA itself out (a measurement mode of the input image)
    hipError_t push(const T* host, size_t n, size_t dev_room, size_t stage_room, hipStream_t s, size_t dev_slack = 0, bool dma = true)
    {
        hipError_t e = reserve(n, dev_room, dev_slack, s);
        if (e != hipSuccess) return e;
        e = done.h ? hipEventSynchronize(done) : done.get(hipEventDisableTiming);       // previous DMA out of the staging block
        if (e == hipSuccess && n > stage.cap) e = stage.grow(stage_room);
        if (e != hipSuccess) return e;
        memcpy(stage.p, host, n * sizeof(T));
        if (dma) e = hipMemcpyAsync(dev.p, stage.p, n * sizeof(T), hipMemcpyHostToDevice, s);
        return e != hipSuccess ? e : hipEventRecord(done, s);
    }
};

// caller memory the device stores results into (zero-copy export)
struct MappedHost {
    void* host = nullptr;
    void* dev = nullptr;
    bool  registered = false;  // attach() had to register the memory: reset() undoes that
    int   capacity = 0;        // entries

    MappedHost() = default;
    MappedHost(MappedHost&& o) noexcept { *this = std::move(o); }
    MappedHost& operator=(MappedHost&& o) noexcept
    {
        std::swap(host, o.host); std::swap(dev, o.dev); std::swap(registered, o.registered); std::swap(capacity, o.capacity);
        return *this;
    }
    ~MappedHost() { reset(); }

    // ordinary or pinned host memory: registered when the runtime does not know it yet
    hipError_t attach(void* ptr, size_t bytes, int entries)
    {
        reset();
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, ptr) != hipSuccess || attr.type == hipMemoryTypeUnregistered) {
            (void)hipGetLastError();
            const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterMapped);
            if (e != hipSuccess) return e;
            registered = true;
        }
        host = ptr;
        const hipError_t e = hipHostGetDevicePointer(&dev, ptr, 0);
        if (e != hipSuccess) { reset(); return e; }
        capacity = entries;
        return hipSuccess;
    }
    // mapped memory whose device address is its host address (psx_host_alloc); ptr == nullptr detaches.  No HIP call
    // unless the previous attachment was registered
    void adopt(void* ptr, int entries) { reset(); host = dev = ptr; capacity = ptr ? entries : 0; }
    void reset()
    {
        if (registered) (void)hipHostUnregister(host);
        host = dev = nullptr; registered = false; capacity = 0;
    }
};
