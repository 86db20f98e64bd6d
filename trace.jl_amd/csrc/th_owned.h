// th_owned.h — the host objects that own something of the HIP runtime: a device allocation, an event, a stream, and a pipe made of them.  Each frees what it holds in its
// destructor and cannot be copied, so whatever holds one (the context, a scene, its geometry, an environment, a function's locals) is torn down by `delete` or by leaving
// the scope, with no list of members to keep.  Nothing of the project is included here: tests/host/owned_main.cpp builds this header alone against stubs of the runtime.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <initializer_list>
#include <type_traits>

// A device allocation.  th_host.h grows and fills it (ensure, upload) and frees it early where that is meant (release).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            (void)reset();
            p = o.p;
            bytes = o.bytes;
            o.p = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { (void)reset(); }
    hipError_t reset() {  // frees the allocation, if any; empty afterwards whatever the runtime answered
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        bytes = 0;
        return e;
    }
};
static_assert(!std::is_copy_constructible_v<DevBuf> && std::is_nothrow_move_constructible_v<DevBuf>, "DevBuf owns its allocation");

// One owned event: without timing, a point in one stream that other streams wait for; with timing, one end of a measured span.
struct OwnedEvent {
    hipEvent_t e = nullptr;
    OwnedEvent() = default;
    OwnedEvent(const OwnedEvent&) = delete;
    OwnedEvent& operator=(const OwnedEvent&) = delete;
    ~OwnedEvent() {
        if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    hipError_t create_timed() { return hipEventCreate(&e); }
    operator hipEvent_t() const { return e; }
};
// One owned stream, at the default priority level or at a given one.
struct OwnedStream {
    hipStream_t s = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream() {
        if (s) (void)hipStreamDestroy(s);
    }
    hipError_t create() { return hipStreamCreate(&s); }
    hipError_t create(int priority) { return hipStreamCreateWithPriority(&s, hipStreamDefault, priority); }
    operator hipStream_t() const { return s; }
};

// One wavefront pipeline: its own queues, counters and stream pair.  Several batches of one frame run concurrently on
// different pipelines so that the long single-ray tail of one batch's traversal launch overlaps the bulk of another's.
// (Members are destroyed last to first: the buffers, then the events, then the streams.)
struct Pipe {
    OwnedStream st, st2;
    OwnedEvent ev_shade, ev_any, ev_any2, ev_done;
    DevBuf q[2][3], sq[3], sq2[3], hits, counters, overflow[2];  // sq / sq2: the shadow queues of odd / even depths (any(d) may still run while shade(d+1) fills the other)
    // Creates each of the six objects that is still null, st2 at *st2_priority when that is given.  After a failure the pipe holds what was made so far and the next call
    // goes on from there: a pipe is used only after a call that returned hipSuccess (th_host.h, ensure_pipe).
    hipError_t complete(const int* st2_priority) {
        if (!st.s)
            if (hipError_t e = st.create()) return e;
        if (!st2.s)
            if (hipError_t e = st2_priority ? st2.create(*st2_priority) : st2.create()) return e;
        for (OwnedEvent* ev : {&ev_shade, &ev_any, &ev_any2, &ev_done})
            if (!ev->e)
                if (hipError_t e = ev->create()) return e;
        return hipSuccess;
    }
};
static_assert(!std::is_copy_constructible_v<Pipe>, "Pipe owns its streams, events and buffers");
