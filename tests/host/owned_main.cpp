// owned_main.cpp — csrc/th_owned.h against stubs of the HIP runtime (tests/test_host_owned.py builds this with -fsanitize=address,undefined and runs it).  The stubs are
// malloc / free with a count of what is live; a second free of a pointer, or a destroy of something never created, aborts.  Links no HIP runtime.
#include "../../trace.jl_amd/csrc/th_owned.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

namespace {
std::set<void*> live_buffers, live_events, live_streams;
int creates = 0, fail_at = 0;  // fail_at: the create call (streams and events counted together, from 1) that fails; 0 = none

void* make(std::set<void*>& live) {
    void* p = std::malloc(16);
    live.insert(p);
    return p;
}
void drop(std::set<void*>& live, void* p, const char* what) {
    if (!live.erase(p)) {
        std::fprintf(stderr, "%s of %p, which is not live\n", what, p);
        std::abort();
    }
    std::free(p);
}
bool create_fails() { return ++creates == fail_at; }
void check(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        std::exit(1);
    }
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t) {
    *p = make(live_buffers);
    return hipSuccess;
}
hipError_t hipFree(void* p) {
    drop(live_buffers, p, "hipFree");
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
    if (create_fails()) return hipErrorOutOfMemory;
    *e = (hipEvent_t)make(live_events);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    drop(live_events, e, "hipEventDestroy");
    return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t* s) {
    if (create_fails()) return hipErrorOutOfMemory;
    *s = (hipStream_t)make(live_streams);
    return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return hipStreamCreate(s); }
hipError_t hipStreamDestroy(hipStream_t s) {
    drop(live_streams, s, "hipStreamDestroy");
    return hipSuccess;
}
}

static DevBuf filled(size_t bytes) {
    DevBuf b;
    check(hipMalloc(&b.p, bytes) == hipSuccess, "hipMalloc");
    b.bytes = bytes;
    return b;
}

int main() {
    {  // move construction leaves the source empty
        DevBuf a = filled(64);
        void* p = a.p;
        DevBuf b(std::move(a));
        check(!a.p && a.bytes == 0 && b.p == p && b.bytes == 64, "move construction");
        check(live_buffers.size() == 1, "one allocation after move construction");
        DevBuf c;  // move assignment into an empty buffer
        c = std::move(b);
        check(!b.p && b.bytes == 0 && c.p == p && c.bytes == 64 && live_buffers.size() == 1, "move assignment into an empty buffer");
        DevBuf d = filled(32);  // ... and into a full one: its allocation is freed
        void* q = d.p;
        d = std::move(c);
        check(!c.p && d.p == p && d.bytes == 64 && live_buffers.size() == 1 && !live_buffers.count(q), "move assignment into a full buffer");
        DevBuf& self = d;  // self-move keeps the allocation
        d = std::move(self);
        check(d.p == p && d.bytes == 64 && live_buffers.size() == 1, "self-move");
        DevBuf e = filled(8);
        void* r = e.p;
        std::swap(d, e);
        check(d.p == r && d.bytes == 8 && e.p == p && e.bytes == 64 && live_buffers.size() == 2, "std::swap");
        check(e.reset() == hipSuccess && !e.p && e.bytes == 0 && live_buffers.size() == 1, "reset");
        check(e.reset() == hipSuccess, "reset of an empty buffer");
    }
    check(live_buffers.empty(), "buffers freed at the end of their scope");
    {  // an array of buffers, some of them empty
        DevBuf arr[2][3];
        arr[0][1] = filled(16);
        arr[1][2] = filled(16);
        check(live_buffers.size() == 2, "two of six filled");
    }
    check(live_buffers.empty(), "an array of buffers destroyed");
    {  // a pipe whose third object (ev_shade, after the two streams) fails to create: held half-made, completed by a second pass
        Pipe pp;
        pp.q[1][2] = filled(16);
        pp.overflow[1] = filled(16);
        creates = 0;
        fail_at = 3;
        check(pp.complete(nullptr) == hipErrorOutOfMemory, "the third create fails");
        check(pp.st.s && pp.st2.s && !pp.ev_shade.e && !pp.ev_any.e && !pp.ev_any2.e && !pp.ev_done.e, "the two streams exist, no event does");
        check(live_streams.size() == 2 && live_events.empty(), "two objects live after the failed pass");
        hipStream_t st = pp.st, st2 = pp.st2;
        fail_at = 0;
        const int prio = -1;
        check(pp.complete(&prio) == hipSuccess, "the second pass completes the pipe");
        check(pp.st.s == st && pp.st2.s == st2, "the second pass keeps the streams of the first");
        check(pp.ev_shade.e && pp.ev_any.e && pp.ev_any2.e && pp.ev_done.e && live_streams.size() == 2 && live_events.size() == 4, "six objects");
        check(pp.complete(nullptr) == hipSuccess && live_streams.size() == 2 && live_events.size() == 4, "a third pass creates nothing");
    }
    check(live_buffers.empty() && live_events.empty() && live_streams.empty(), "the pipe destroyed everything it held");
    {  // an array of pipes, untouched and partly made, as a context holds them
        Pipe pipes[3];
        check(pipes[1].complete(nullptr) == hipSuccess, "one pipe of three made");
        creates = 0;
        fail_at = 1;
        check(pipes[2].complete(nullptr) != hipSuccess && !pipes[2].st.s, "a pipe whose first create fails holds nothing");
        fail_at = 0;
    }
    check(live_buffers.empty() && live_events.empty() && live_streams.empty(), "live counts are 0 at exit");
    std::puts("owned ok");
    return 0;
}
