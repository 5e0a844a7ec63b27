// dev_owner.hpp -- move-only owners of what the library holds on a device: a block of device memory, an event, an ordering
// mark (an event and whether it is still to be waited for), a stream, a block of page-locked host memory.  Copy is deleted, a
// move leaves the source empty, every destructor releases what the object holds -- so a struct made of these frees itself, in
// the reverse of its members' declaration order.
//
// Nothing is #included here.  The includer brings, in front of this file:
//   - the HIP runtime (<hip/hip_runtime.h>) -- or, a host-only test, stand-ins for the names used below: hipError_t, hipSuccess,
//     hipErrorOutOfMemory, hipGetErrorString, hipEvent_t, hipStream_t, hipEventDisableTiming, hipHostMallocDefault, hipMalloc,
//     hipFree, hipMemset, hipStreamSynchronize, hipEventCreate, hipEventCreateWithFlags, hipEventDestroy, hipEventRecord,
//     hipStreamWaitEvent, hipEventSynchronize, hipStreamCreateWithFlags, hipStreamCreateWithPriority, hipStreamDestroy,
//     hipHostMalloc, hipHostFree;
//   - <string>, <utility>, include/trmc.h (TRMC_ENOMEM, TRMC_EHIP);
//   - int fail(int code, const std::string &msg): stores the message where the caller's last-error lives, returns the code.
#pragma once

struct DevBuf { // device memory
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            bytes = std::exchange(o.bytes, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t need, bool zero_new = false)
    {
        if (need <= bytes) return 0;
        release();
        hipError_t e = hipMalloc(&p, need ? need : 1);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(TRMC_ENOMEM, std::string("hipMalloc(") + std::to_string(need) + "): " + hipGetErrorString(e));
        }
        bytes = need;
        if (zero_new && need) { // (granule planes: recycled memory must not hold a tag that could pass for a live one)
            // (hipMemset of device memory may return before it has run, on the null stream -- which the plans'
            // non-blocking streams do not wait for: without the synchronisation the fill can land AFTER the first
            // kernels of a window have written into the buffer; seen with two processes sharing one GPU)
            e = hipMemset(p, 0, need);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
            if (e != hipSuccess) return fail(TRMC_EHIP, std::string("hipMemset: ") + hipGetErrorString(e));
        }
        return 0;
    }
    void release()
    {
        if (p) (void)hipFree(p); // (waits for the device)
        p = nullptr;
        bytes = 0;
    }
};

struct DevEvent { // an event, made on first use; reads as the hipEvent_t it holds
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    DevEvent(DevEvent &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
    DevEvent &operator=(DevEvent &&o) noexcept
    {
        if (this != &o) {
            release();
            e = std::exchange(o.e, nullptr);
        }
        return *this;
    }
    ~DevEvent() { release(); }
    operator hipEvent_t() const { return e; }
    // one that times (hipEventCreate) or one that only orders streams (hipEventDisableTiming); nothing if it exists
    int ensure(bool timing)
    {
        if (e) return 0;
        const hipError_t rc = timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (rc == hipSuccess) return 0;
        e = nullptr;
        return fail(rc == hipErrorOutOfMemory ? TRMC_ENOMEM : TRMC_EHIP,
                    std::string(timing ? "hipEventCreate: " : "hipEventCreateWithFlags: ") + hipGetErrorString(rc));
    }
    void release()
    {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
};

// An ordering mark: an event that only orders streams, with whether anything recorded on it is still to be waited for.  The
// producer record()s it on its stream; a consumer order()s each stream that has to go behind it and then settle()s it -- apart,
// because one mark may hold several streams back -- or, on the host, sync()s.  Not pending, order() and sync() call nothing.
struct DevMark {
    DevMark() = default;
    DevMark(DevMark &&o) noexcept : ev(std::move(o.ev)), waiting(std::exchange(o.waiting, false)) {}
    DevMark &operator=(DevMark &&o) noexcept
    {
        if (this != &o) {
            ev = std::move(o.ev);
            waiting = std::exchange(o.waiting, false);
        }
        return *this;
    }
    int record(hipStream_t st) // made on first use
    {
        if (int rc = ev.ensure(false)) return rc;
        if (int rc = tried(hipEventRecord(ev, st), "hipEventRecord: ")) return rc;
        waiting = true;
        return 0;
    }
    int order(hipStream_t st) const { return waiting ? tried(hipStreamWaitEvent(st, ev, 0), "hipStreamWaitEvent: ") : 0; }
    void settle() { waiting = false; }
    int sync() // (settled first: a wait that fails is not tried again)
    {
        if (!waiting) return 0;
        waiting = false;
        return tried(hipEventSynchronize(ev), "hipEventSynchronize: ");
    }
    bool pending() const { return waiting; }

private:
    DevEvent ev;
    bool waiting = false;
    static int tried(hipError_t rc, const char *what)
    {
        if (rc == hipSuccess) return 0;
        return fail(rc == hipErrorOutOfMemory ? TRMC_ENOMEM : TRMC_EHIP, std::string(what) + hipGetErrorString(rc));
    }
};

struct DevStream { // a stream, made on first use with flags or with flags and a priority; reads as its hipStream_t
    hipStream_t s = nullptr;
    DevStream() = default;
    DevStream(const DevStream &) = delete;
    DevStream &operator=(const DevStream &) = delete;
    DevStream(DevStream &&o) noexcept : s(std::exchange(o.s, nullptr)) {}
    DevStream &operator=(DevStream &&o) noexcept
    {
        if (this != &o) {
            release();
            s = std::exchange(o.s, nullptr);
        }
        return *this;
    }
    ~DevStream() { release(); }
    operator hipStream_t() const { return s; }
    int ensure(unsigned flags) { return made(s ? hipSuccess : hipStreamCreateWithFlags(&s, flags), "hipStreamCreateWithFlags: "); }
    int ensure(unsigned flags, int priority)
    {
        return made(s ? hipSuccess : hipStreamCreateWithPriority(&s, flags, priority), "hipStreamCreateWithPriority: ");
    }
    void release()
    {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
    }

private:
    int made(hipError_t rc, const char *what)
    {
        if (rc == hipSuccess) return 0;
        s = nullptr;
        return fail(rc == hipErrorOutOfMemory ? TRMC_ENOMEM : TRMC_EHIP, std::string(what) + hipGetErrorString(rc));
    }
};

struct HostBlock { // page-locked host memory
    void *p = nullptr;
    size_t bytes = 0;
    HostBlock() = default;
    HostBlock(const HostBlock &) = delete;
    HostBlock &operator=(const HostBlock &) = delete;
    HostBlock(HostBlock &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    HostBlock &operator=(HostBlock &&o) noexcept
    {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            bytes = std::exchange(o.bytes, 0);
        }
        return *this;
    }
    ~HostBlock() { release(); }
    int ensure(size_t need)
    {
        if (need <= bytes) return 0;
        release();
        const hipError_t e = hipHostMalloc(&p, need ? need : 1, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(e == hipErrorOutOfMemory ? TRMC_ENOMEM : TRMC_EHIP, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        }
        bytes = need;
        return 0;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};
