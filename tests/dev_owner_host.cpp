// dev_owner_host.cpp -- csrc/dev_owner.hpp on the host: the owners compiled against COUNTING STAND-INS for the HIP names they
// call.  Every stand-in keeps what it handed out in a set; releasing something twice, or something it never made, aborts.  Every
// case must leave the set empty, or the program exits non-zero (tests/test_dev_owner_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it).
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../include/trmc.h"

// ---------------------------------------------------------------- the stand-ins
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorUnknown = 999 };
typedef struct ihipEvent_t *hipEvent_t;
typedef struct ihipStream_t *hipStream_t;
constexpr unsigned hipEventDisableTiming = 2, hipStreamNonBlocking = 1, hipHostMallocDefault = 0;

static std::set<void *> g_live;          // everything handed out and not released yet
static int g_made = 0, g_released = 0;   // counts, all kinds
static int g_timing = 0, g_ordering = 0; // events made with hipEventCreate / with hipEventDisableTiming
static int g_memsets = 0, g_syncs = 0;
static bool g_oom = false;               // the next allocation fails

static hipError_t hand_out(void **out)
{
    if (g_oom) {
        g_oom = false;
        return hipErrorOutOfMemory;
    }
    *out = std::malloc(1); // (a distinct address; the sanitizer watches it as well)
    g_live.insert(*out);
    ++g_made;
    return hipSuccess;
}
static hipError_t take_back(void *p, const char *what)
{
    if (!g_live.erase(p)) {
        std::fprintf(stderr, "%s: released twice, or never made\n", what);
        std::abort();
    }
    std::free(p);
    ++g_released;
    return hipSuccess;
}
static const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
static hipError_t hipMalloc(void **p, size_t) { return hand_out(p); }
static hipError_t hipFree(void *p) { return take_back(p, "hipFree"); }
static hipError_t hipMemset(void *p, int, size_t) { ++g_memsets; return g_live.count(p) ? hipSuccess : hipErrorUnknown; }
static hipError_t hipStreamSynchronize(hipStream_t) { ++g_syncs; return hipSuccess; }
static hipError_t hipEventCreate(hipEvent_t *e) { ++g_timing; return hand_out((void **)e); }
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
    if (flags != hipEventDisableTiming) std::abort();
    ++g_ordering;
    return hand_out((void **)e);
}
static hipError_t hipEventDestroy(hipEvent_t e) { return take_back(e, "hipEventDestroy"); }
// the three calls of an ordering mark: counted, each remembering the event (and stream) of its last call; an event that is not
// live aborts
static int g_records = 0, g_waits = 0, g_event_syncs = 0;
static std::vector<std::pair<hipEvent_t, hipStream_t>> g_recorded, g_waited; // (event, stream) of every call, in order
static hipEvent_t g_synced = nullptr;
static bool g_sync_fails = false; // the next hipEventSynchronize fails
static void live_event(hipEvent_t e, const char *what)
{
    if (!g_live.count(e)) {
        std::fprintf(stderr, "%s: on an event that does not exist\n", what);
        std::abort();
    }
}
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    live_event(e, "hipEventRecord");
    ++g_records;
    g_recorded.emplace_back(e, s);
    return hipSuccess;
}
static hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags)
{
    live_event(e, "hipStreamWaitEvent");
    if (flags != 0) std::abort();
    ++g_waits;
    g_waited.emplace_back(e, s);
    return hipSuccess;
}
static hipError_t hipEventSynchronize(hipEvent_t e)
{
    live_event(e, "hipEventSynchronize");
    ++g_event_syncs;
    g_synced = e;
    return std::exchange(g_sync_fails, false) ? hipErrorUnknown : hipSuccess;
}
static hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return hand_out((void **)s); }
static hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned, int) { return hand_out((void **)s); }
static hipError_t hipStreamDestroy(hipStream_t s) { return take_back(s, "hipStreamDestroy"); }
static hipError_t hipHostMalloc(void **p, size_t, unsigned) { return hand_out(p); }
static hipError_t hipHostFree(void *p) { return take_back(p, "hipHostFree"); }

static std::string g_err;
static int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#include "../t-route_amd/csrc/dev_owner.hpp"

// ---------------------------------------------------------------- the cases
static int g_bad = 0;
#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);                    \
            ++g_bad;                                                                           \
        }                                                                                      \
    } while (0)

static void ensure_grows()
{
    DevBuf b;
    CHECK(b.ensure(100) == 0 && b.p && b.bytes == 100);
    void *const first = b.p;
    CHECK(b.ensure(40) == 0 && b.p == first && b.bytes == 100); // a smaller request: nothing changes
    CHECK(g_made == 1 && g_released == 0);
    CHECK(b.ensure(200) == 0 && b.bytes == 200 && !g_live.count(first) && g_released == 1);
    void *const second = b.p;
    CHECK(b.ensure(300, true) == 0 && b.bytes == 300 && !g_live.count(second) && g_released == 2);
    CHECK(g_memsets == 1 && g_syncs == 1); // (zero_new: the fill and the synchronisation behind it)
    CHECK(g_live.size() == 1);
    b.release();
    CHECK(!b.p && b.bytes == 0 && g_live.empty());
    b.release(); // (an empty one: nothing to do)
}

static void ensure_fails()
{
    DevBuf b;
    CHECK(b.ensure(64) == 0);
    g_oom = true;
    CHECK(b.ensure(128) == TRMC_ENOMEM && !b.p && b.bytes == 0 && g_live.empty());
    CHECK(g_err.find("hipMalloc(128)") == 0);
    g_oom = true;
    DevBuf c;
    CHECK(c.ensure(8) == TRMC_ENOMEM && !c.p && c.bytes == 0);
    g_oom = true;
    DevEvent e;
    CHECK(e.ensure(false) == TRMC_ENOMEM && !(hipEvent_t)e);
    g_oom = true;
    DevStream s;
    CHECK(s.ensure(hipStreamNonBlocking) == TRMC_ENOMEM && !(hipStream_t)s);
    g_oom = true;
    HostBlock h;
    CHECK(h.ensure(8) == TRMC_ENOMEM && !h.p && h.bytes == 0);
    CHECK(b.ensure(16) == 0 && b.bytes == 16); // ... and usable again afterwards
}

static void moves()
{
    DevBuf a, b;
    CHECK(a.ensure(10) == 0 && b.ensure(20) == 0);
    void *const pa = a.p, *const pb = b.p;
    DevBuf c(std::move(a)); // move-construct: the source is left empty
    CHECK(c.p == pa && c.bytes == 10 && !a.p && a.bytes == 0 && g_released == 0);
    b = std::move(c); // move-assign onto a non-empty target: the target's block goes, once
    CHECK(b.p == pa && b.bytes == 10 && !c.p && !g_live.count(pb) && g_released == 1);
    DevBuf &self = b;
    b = std::move(self); // self-move: harmless
    CHECK(b.p == pa && b.bytes == 10 && g_released == 1);
    DevEvent e, f;
    CHECK(e.ensure(true) == 0 && f.ensure(false) == 0);
    const hipEvent_t he = e;
    f = std::move(e);
    CHECK((hipEvent_t)f == he && !(hipEvent_t)e && g_released == 2);
    DevEvent &fself = f;
    f = std::move(fself);
    CHECK((hipEvent_t)f == he);
    DevStream s, t;
    CHECK(s.ensure(hipStreamNonBlocking) == 0 && t.ensure(hipStreamNonBlocking, -1) == 0);
    const hipStream_t hs = s;
    CHECK(s.ensure(hipStreamNonBlocking, 0) == 0 && (hipStream_t)s == hs); // (it exists: not made again)
    t = std::move(s);
    DevStream u(std::move(t));
    CHECK((hipStream_t)u == hs && !(hipStream_t)s && !(hipStream_t)t && g_released == 3);
    HostBlock h, k;
    CHECK(h.ensure(10) == 0 && k.ensure(30) == 0 && h.ensure(5) == 0 && h.bytes == 10);
    void *const ph = h.p;
    k = std::move(h);
    HostBlock m(std::move(k));
    CHECK(m.p == ph && m.bytes == 10 && !h.p && !k.p && g_released == 4);
}

static void vectors()
{
    std::vector<DevBuf> bufs;
    std::vector<DevEvent> evs;
    size_t reallocations = 0;
    for (int i = 0; i < 40; ++i) {
        const size_t cap = bufs.capacity();
        DevBuf b;
        CHECK(b.ensure((size_t)i + 1) == 0);
        bufs.push_back(std::move(b));
        reallocations += bufs.capacity() != cap;
        DevEvent e;
        CHECK(e.ensure(i % 2 == 0) == 0);
        evs.push_back(std::move(e));
    }
    CHECK(reallocations >= 3 && g_made == 80 && g_released == 0 && g_live.size() == 80);
    for (int i = 0; i < 40; ++i) CHECK(bufs[(size_t)i].bytes == (size_t)i + 1 && g_live.count(bufs[(size_t)i].p) && g_live.count((hipEvent_t)evs[(size_t)i]));
    bufs.clear();
    CHECK(g_released == 40);
    evs.clear();
    CHECK(g_released == 80);
}

static void swaps()
{
    DevBuf a, b;
    CHECK(a.ensure(10) == 0 && b.ensure(20) == 0);
    void *const pa = a.p, *const pb = b.p;
    std::swap(a, b);
    CHECK(a.p == pb && a.bytes == 20 && b.p == pa && b.bytes == 10 && g_released == 0 && g_live.size() == 2);
    DevBuf empty;
    std::swap(a, empty);
    CHECK(!a.p && a.bytes == 0 && empty.p == pb && g_released == 0);
}

// the shape of trmc_rowset_create: a local is filled, something fails, the function returns before the local is handed over
static int register_rows(std::vector<DevBuf> &sets, bool copy_fails)
{
    DevBuf b;
    if (int rc = b.ensure(64)) return rc;
    if (copy_fails) return fail(TRMC_EHIP, "the copy failed");
    sets.push_back(std::move(b));
    return 0;
}
static void early_return()
{
    std::vector<DevBuf> sets;
    CHECK(register_rows(sets, false) == 0 && sets.size() == 1 && g_live.size() == 1);
    CHECK(register_rows(sets, true) == TRMC_EHIP && sets.size() == 1);
    CHECK(g_live.size() == 1 && g_made == 2 && g_released == 1); // (the local's block went with the local)
}

static void event_made_once()
{
    DevEvent timing, ordering;
    CHECK(timing.ensure(true) == 0 && ordering.ensure(false) == 0);
    const hipEvent_t t = timing, o = ordering;
    CHECK(t && o && timing.ensure(true) == 0 && ordering.ensure(false) == 0);
    CHECK((hipEvent_t)timing == t && (hipEvent_t)ordering == o && g_timing == 1 && g_ordering == 1 && g_made == 2);
}

// a plan's shape: streams and events on top, the hold on a shared block, buffers of its own below
struct Shared {
    DevBuf params, order;
};
struct Holder {
    DevStream stream;
    DevEvent ev;
    std::shared_ptr<Shared> sh;
    DevBuf window;
};
static void shared_block()
{
    int order[3] = {0, 1, 2};
    int orders = 0;
    do {
        g_made = g_released = 0;
        std::unique_ptr<Holder> h[3];
        auto sh = std::make_shared<Shared>();
        CHECK(sh->params.ensure(100) == 0 && sh->order.ensure(50) == 0);
        void *const params = sh->params.p, *const ord = sh->order.p;
        for (auto &x : h) {
            x.reset(new Holder());
            x->sh = sh;
            CHECK(x->stream.ensure(hipStreamNonBlocking, 0) == 0 && x->ev.ensure(false) == 0 && x->window.ensure(1000) == 0);
        }
        sh.reset();
        CHECK(g_live.size() == 2 + 9);
        for (int k = 0; k < 3; ++k) {
            Holder &x = *h[order[k]];
            void *const own[3] = {x.window.p, (void *)(hipStream_t)x.stream, (void *)(hipEvent_t)x.ev};
            h[order[k]].reset();
            for (void *p : own) CHECK(!g_live.count(p)); // its own go at its own destruction
            const bool last = k == 2;
            CHECK(g_live.count(params) == (last ? 0u : 1u) && g_live.count(ord) == (last ? 0u : 1u)); // the block: with the last
            CHECK(g_released == 3 * (k + 1) + (last ? 2 : 0));
        }
        CHECK(g_live.empty());
        ++orders;
    } while (std::next_permutation(order, order + 3));
    CHECK(orders == 6);
}

// ---- DevMark: an event that orders streams and whether it is still to be waited for
static hipStream_t stream_no(int k) // (distinct addresses; never dereferenced)
{
    static char s[4];
    return (hipStream_t)(void *)&s[k];
}
static std::pair<hipEvent_t, hipStream_t> on(hipEvent_t e, hipStream_t s) { return {e, s}; }

static void mark_orders_two_streams()
{
    const hipStream_t a = stream_no(0), b = stream_no(1), c = stream_no(2);
    DevMark m;
    CHECK(!m.pending());
    CHECK(m.record(a) == 0 && m.pending() && g_records == 1 && g_ordering == 1 && g_timing == 0); // (an event that only orders)
    const hipEvent_t e = g_recorded.back().first;
    CHECK(g_recorded.back() == on(e, a));
    CHECK(m.order(b) == 0 && m.order(c) == 0 && m.pending()); // ordering a stream does not settle the mark: the next stream waits too
    CHECK(g_waits == 2 && g_waited[0] == on(e, b) && g_waited[1] == on(e, c));
    m.settle();
    CHECK(!m.pending() && m.order(b) == 0 && g_waits == 2 && g_records == 1);
}

static void mark_idle_calls_nothing()
{
    const hipStream_t a = stream_no(0);
    DevMark m;
    CHECK(m.order(a) == 0 && m.sync() == 0 && !m.pending()); // never recorded: there is not even an event
    CHECK(g_made == 0 && g_waits == 0 && g_event_syncs == 0);
    CHECK(m.record(a) == 0);
    m.settle();
    CHECK(m.order(a) == 0 && m.sync() == 0 && g_waits == 0 && g_event_syncs == 0); // settled: the same
    CHECK(m.record(a) == 0 && m.sync() == 0 && !m.pending() && g_event_syncs == 1 && g_synced == g_recorded.back().first);
    CHECK(m.sync() == 0 && m.order(a) == 0 && g_event_syncs == 1 && g_waits == 0); // a sync settles
}

static void mark_sync_that_fails_settles()
{
    DevMark m;
    CHECK(m.record(stream_no(0)) == 0);
    g_sync_fails = true;
    CHECK(m.sync() == TRMC_EHIP && !m.pending() && g_event_syncs == 1 && g_err.find("hipEventSynchronize") == 0);
    CHECK(m.sync() == 0 && g_event_syncs == 1); // (not tried again)
}

static void mark_without_an_event()
{
    DevMark m;
    g_oom = true;
    CHECK(m.record(stream_no(0)) == TRMC_ENOMEM && !m.pending() && g_records == 0 && g_made == 0 && g_live.empty());
    CHECK(g_err.find("hipEventCreateWithFlags") == 0);
    CHECK(m.order(stream_no(1)) == 0 && m.sync() == 0 && g_waits == 0 && g_event_syncs == 0);
    CHECK(m.record(stream_no(0)) == 0 && m.pending() && g_made == 1); // ... and usable afterwards
}

static void mark_moves()
{
    const hipStream_t a = stream_no(0), b = stream_no(1);
    DevMark m;
    CHECK(m.record(a) == 0);
    const hipEvent_t e = g_recorded.back().first;
    DevMark n(std::move(m)); // move-construct: the source is left with nothing, pending or to free
    CHECK(n.pending() && !m.pending() && m.order(b) == 0 && m.sync() == 0 && g_waits == 0 && g_event_syncs == 0);
    CHECK(n.order(b) == 0 && g_waited.back() == on(e, b));
    DevMark o;
    CHECK(o.record(a) == 0);
    const hipEvent_t eo = g_recorded.back().first;
    o = std::move(n); // move-assign onto a mark with an event: that event goes, once
    CHECK(eo != e && !g_live.count(eo) && g_released == 1 && o.pending() && !n.pending());
    CHECK(o.order(a) == 0 && g_waited.back() == on(e, a));
    DevMark &self = o;
    o = std::move(self); // self-move: harmless
    CHECK(o.pending() && o.order(b) == 0 && g_waited.back() == on(e, b) && g_released == 1);
    o.settle();
    n = std::move(o); // a settled one: the event moves, nothing is pending on either side
    CHECK(!n.pending() && !o.pending() && g_live.count(e) && g_released == 1);
    std::vector<DevMark> marks;
    std::vector<hipEvent_t> evs;
    size_t reallocations = 0;
    for (int i = 0; i < 40; ++i) {
        const size_t cap = marks.capacity();
        DevMark k;
        if (i % 2 == 0) { // every other one pending when it moves in
            CHECK(k.record(a) == 0);
            evs.push_back(g_recorded.back().first);
        }
        marks.push_back(std::move(k));
        reallocations += marks.capacity() != cap;
    }
    CHECK(reallocations >= 3 && g_made == 2 + 20 && g_released == 1);
    for (int i = 0; i < 40; ++i) {
        const int waits = g_waits;
        CHECK(marks[(size_t)i].pending() == (i % 2 == 0) && marks[(size_t)i].order(b) == 0 && g_waits == waits + (i % 2 == 0));
        if (i % 2 == 0) CHECK(g_waited.back() == on(evs[(size_t)i / 2], b)); // each with its own event
    }
    marks.clear();
    CHECK(g_released == 1 + 20);
}

static void mark_event_made_once()
{
    {
        DevMark m;
        hipEvent_t e = nullptr;
        for (int i = 0; i < 5; ++i) {
            CHECK(m.record(stream_no(i % 3)) == 0 && m.pending());
            if (i == 0) e = g_recorded.back().first;
            CHECK(g_recorded.back() == on(e, stream_no(i % 3)));
            if (i % 2) m.settle(); // (recorded again while pending, and after it has been settled)
        }
        CHECK(g_records == 5 && g_ordering == 1 && g_made == 1 && g_released == 0);
    }
    CHECK(g_made == 1 && g_released == 1);
}

int main()
{
    const struct { const char *name; void (*run)(); } cases[] = {
        {"ensure grows", ensure_grows}, {"ensure fails", ensure_fails}, {"moves", moves}, {"vectors", vectors}, {"swap", swaps},
        {"early return", early_return}, {"event made once", event_made_once}, {"shared block", shared_block},
        {"mark orders", mark_orders_two_streams}, {"mark idle", mark_idle_calls_nothing}, {"mark sync fails", mark_sync_that_fails_settles},
        {"mark no event", mark_without_an_event}, {"mark moves", mark_moves}, {"mark made once", mark_event_made_once},
    };
    for (const auto &c : cases) {
        g_made = g_released = g_timing = g_ordering = g_memsets = g_syncs = g_records = g_waits = g_event_syncs = 0;
        g_oom = g_sync_fails = false;
        g_recorded.clear();
        g_waited.clear();
        g_synced = nullptr;
        const int bad = g_bad;
        c.run();
        if (!g_live.empty()) {
            std::fprintf(stderr, "%s: %zu left unreleased\n", c.name, g_live.size());
            ++g_bad;
        }
        std::printf("%-16s %s\n", c.name, g_bad == bad ? "ok" : "FAILED");
    }
    return g_bad ? 1 : 0;
}
