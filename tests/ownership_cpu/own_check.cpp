// csrc/fdc_own.h on a CPU: the HIP names it uses are counting stand-ins defined here (blocks come from malloc, so AddressSanitizer
// sees a leak, a double free or a use after free of what the owning types hold), and the allocating ones can be told to fail.
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all own_check.cpp && ./a.out
// (tests/test_ownership_cpu.py builds and runs it)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <type_traits>

// ---- stand-ins ----------------------------------------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
struct FakeEvent { int tag; };
typedef FakeEvent* hipEvent_t;

static std::set<void*> g_dev, g_pinned;          // what is live, by kind
static std::set<hipEvent_t> g_events;
static void* g_last_freed = nullptr;
static int g_mallocs = 0, g_frees = 0, g_copies = 0, g_bad_frees = 0;
static int g_fail_in = 0;                        // k > 0: the k-th allocating call from now (device, pinned or event) fails

static bool fail_now() { return g_fail_in > 0 && --g_fail_in == 0; }

static hipError_t hipMalloc(void** p, size_t bytes) {
    ++g_mallocs;
    if (fail_now()) { *p = (void*)0x1; return hipErrorOutOfMemory; }      // (garbage on failure: the owner must not keep it)
    *p = malloc(bytes);
    g_dev.insert(*p);
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    ++g_frees;
    if (!g_dev.erase(p)) { ++g_bad_frees; return hipErrorOutOfMemory; }
    g_last_freed = p;
    free(p);
    return hipSuccess;
}
static hipError_t hipHostMalloc(void** p, size_t bytes) {
    if (fail_now()) { *p = (void*)0x1; return hipErrorOutOfMemory; }
    *p = malloc(bytes);
    g_pinned.insert(*p);
    return hipSuccess;
}
static hipError_t hipHostFree(void* p) {
    if (!g_pinned.erase(p)) { ++g_bad_frees; return hipErrorOutOfMemory; }
    free(p);
    return hipSuccess;
}
static hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
    ++g_copies;
    memcpy(dst, src, bytes);
    return hipSuccess;
}
static hipError_t hipEventCreate(hipEvent_t* e) {
    if (fail_now()) { *e = (hipEvent_t)0x1; return hipErrorOutOfMemory; }
    *e = new FakeEvent{0};
    g_events.insert(*e);
    return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) {
    if (!g_events.erase(e)) { ++g_bad_frees; return hipErrorOutOfMemory; }
    delete e;
    return hipSuccess;
}

#include "../../4dcapture-fpv_amd/csrc/fdc_own.h"

using namespace fdc;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "own_check: line %d: %s\n", __LINE__, #c); exit(1); } } while (0)
#define TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)      // the library's HIP_TRY

static_assert(!std::is_copy_constructible_v<DevBuf<float>> && !std::is_copy_assignable_v<DevBuf<float>>, "DevBuf owns its block");
static_assert(!std::is_copy_constructible_v<PinnedBuf<int>> && !std::is_copy_assignable_v<PinnedBuf<int>>, "PinnedBuf owns its block");
static_assert(!std::is_copy_constructible_v<DevEvent> && !std::is_copy_assignable_v<DevEvent>, "DevEvent owns its event");
static_assert(!std::is_copy_constructible_v<DevEvents> && !std::is_copy_assignable_v<DevEvents>, "DevEvents owns its events");
static_assert(std::is_nothrow_move_constructible_v<DevBuf<float>> && std::is_nothrow_move_constructible_v<DevEvent>, "movable");

// the stand-ins' books and the header's counters agree, and both say `blocks` blocks and `events` events
static void expect_live(size_t blocks, size_t events) {
    CHECK(g_dev.size() + g_pinned.size() == blocks);
    CHECK(g_events.size() == events);
    CHECK(g_live_blocks.load() == (long long)blocks);
    CHECK(g_live_events.load() == (long long)events);
    CHECK(g_bad_frees == 0);
    if (blocks == 0) CHECK(g_live_bytes.load() == 0);
}

static void test_ensure_and_grow() {
    DevBuf<float> b;
    CHECK(b.p == nullptr && b.n == 0);
    CHECK(b.ensure(10) == hipSuccess && b.p && b.n == 10);
    expect_live(1, 0);
    CHECK(g_live_bytes.load() == 40);
    float* const first = b.p;
    const int m0 = g_mallocs, f0 = g_frees;
    CHECK(b.ensure(10) == hipSuccess && b.ensure(3) == hipSuccess && b.ensure(0) == hipSuccess);      // count <= n: nothing happens
    CHECK(g_mallocs == m0 && g_frees == f0 && b.p == first && b.n == 10);
    CHECK(b.ensure(11) == hipSuccess && b.n == 11);                                                    // grow: exactly the old block goes
    CHECK(g_mallocs == m0 + 1 && g_frees == f0 + 1 && g_last_freed == (void*)first);
    expect_live(1, 0);
    CHECK(g_live_bytes.load() == 44);
    g_fail_in = 1;                                                                                     // a failed grow leaves it empty
    CHECK(b.ensure(100) == hipErrorOutOfMemory);
    CHECK(b.p == nullptr && b.n == 0);
    expect_live(0, 0);
    CHECK(b.ensure(4) == hipSuccess && b.n == 4);                                                      // ... and usable
    b.release();
    b.release();                                                                                       // twice is harmless
    CHECK(b.p == nullptr && b.n == 0);
    expect_live(0, 0);
    DevBuf<double> z;                                                                                  // nothing asked of an empty buffer: nothing done
    CHECK(z.ensure(0) == hipSuccess && z.p == nullptr && g_mallocs == m0 + 3);
    expect_live(0, 0);
}

static void test_upload() {
    DevBuf<int> b;
    const int c0 = g_copies;
    CHECK(b.upload(nullptr, 0) == hipSuccess);                    // 0 elements: a success, nothing copied, nothing allocated
    CHECK(g_copies == c0 && b.p == nullptr);
    const int h[3] = {7, 8, 9};
    CHECK(b.upload(h, 3) == hipSuccess && b.n == 3 && b.p[0] == 7 && b.p[2] == 9 && g_copies == c0 + 1);
    g_fail_in = 1;
    const int h5[5] = {1, 2, 3, 4, 5};
    CHECK(b.upload(h5, 5) == hipErrorOutOfMemory && b.p == nullptr && b.n == 0 && g_copies == c0 + 1);
    expect_live(0, 0);
}

static void test_moves() {
    DevBuf<float> a;
    CHECK(a.ensure(8) == hipSuccess);
    float* const pa = a.p;
    DevBuf<float> b(std::move(a));                                // construction: the block travels, the source is empty
    CHECK(b.p == pa && b.n == 8 && a.p == nullptr && a.n == 0);
    expect_live(1, 0);
    DevBuf<float> c;
    CHECK(c.ensure(5) == hipSuccess);
    float* const pc = c.p;
    expect_live(2, 0);
    const int f0 = g_frees;
    c = std::move(b);                                             // assignment: the destination's old block is freed
    CHECK(c.p == pa && c.n == 8 && b.p == nullptr && b.n == 0);
    CHECK(g_frees == f0 + 1 && g_last_freed == (void*)pc);
    expect_live(1, 0);
    DevBuf<float>& self = c;
    c = std::move(self);                                          // onto itself: nothing happens
    CHECK(c.p == pa && c.n == 8);
    DevEvent e, f;
    CHECK(e.create() == hipSuccess && f.create() == hipSuccess);
    const hipEvent_t he = e;
    expect_live(1, 2);
    f = std::move(e);
    CHECK((hipEvent_t)f == he && (hipEvent_t)e == nullptr);
    expect_live(1, 1);
    DevEvent g(std::move(f));
    CHECK((hipEvent_t)g == he && (hipEvent_t)f == nullptr);
    PinnedBuf<int> p;                                             // allocated once: a second call keeps the block
    CHECK(p.alloc() == hipSuccess);
    int* const pp = p.p;
    CHECK(p.alloc() == hipSuccess && p.p == pp);
    expect_live(2, 1);
}

struct Several {                                                  // the shape of the library's state structs
    DevBuf<float> a, b;
    DevBuf<int> tab[3];
    struct { DevBuf<unsigned short> ids; int nq = 0; } inner;
    PinnedBuf<int> flag;
    DevEvents ev;
};
static void test_scopes() {
    {
        Several s;
        CHECK(s.a.ensure(3) == hipSuccess && s.b.ensure(1) == hipSuccess && s.inner.ids.ensure(9) == hipSuccess);
        for (auto& t : s.tab) CHECK(t.ensure(2) == hipSuccess);
        CHECK(s.flag.alloc() == hipSuccess);
        CHECK(s.ev.grow_to(4) == hipSuccess && s.ev.size() == 4);
        CHECK(s.ev.grow_to(2) == hipSuccess && s.ev.size() == 4);              // (only grows)
        expect_live(7, 4);
    }
    expect_live(0, 0);
    Several* h = new Several();                                   // ... and through `delete`, as the destroy entry points do
    CHECK(h->a.ensure(3) == hipSuccess && h->tab[2].ensure(2) == hipSuccess && h->ev.grow_to(1) == hipSuccess);
    expect_live(2, 1);
    delete h;
    expect_live(0, 0);
}

static int early_return(int fail_at) {                            // two buffers and an event, then something fails
    DevBuf<float> a, b;
    DevEvent e;
    TRY(a.ensure(16));
    TRY(b.ensure(16));
    TRY(e.create());
    expect_live(2, 1);
    g_fail_in = fail_at;
    DevBuf<int> c;
    TRY(c.ensure(1));
    return 0;
}
static void test_early_return() {
    CHECK(early_return(1) == (int)hipErrorOutOfMemory);
    expect_live(0, 0);
    CHECK(early_return(0) == 0);
    expect_live(0, 0);
}

struct LbfgsLike { DevBuf<double> S; DevBuf<float> W, RO; DevBuf<int> active; PinnedBuf<int> active_h; };   // fdcap_lbfgs_create's sequence
static hipError_t lbfgs_like_create(LbfgsLike** out) {
    LbfgsLike* L = new LbfgsLike();
    hipError_t e = L->S.ensure(4);
    if (e == hipSuccess) e = L->W.ensure(4 * 100);
    if (e == hipSuccess) e = L->RO.ensure(4 * 8);
    if (e == hipSuccess) e = L->active.ensure(2);
    if (e == hipSuccess) e = L->active_h.alloc();
    if (e != hipSuccess) { delete L; return e; }
    *out = L;
    return hipSuccess;
}
static void test_failure_at_every_position() {
    for (int k = 1; k <= 5; ++k) {
        g_fail_in = k;
        LbfgsLike* L = nullptr;
        CHECK(lbfgs_like_create(&L) == hipErrorOutOfMemory && L == nullptr);
        expect_live(0, 0);
    }
    g_fail_in = 6;                                                // (beyond the sequence: it succeeds)
    LbfgsLike* L = nullptr;
    CHECK(lbfgs_like_create(&L) == hipSuccess && L);
    expect_live(5, 0);
    *L->active_h.p = 3;
    delete L;
    expect_live(0, 0);
    g_fail_in = 0;
}

static void test_events_partial() {
    {
        DevEvents ev;
        g_fail_in = 3;
        CHECK(ev.grow_to(5) == hipErrorOutOfMemory);              // the 3rd of 5 fails: two stay
        CHECK(ev.size() == 2 && ev[0] && ev[1] && ev[0] != ev[1]);
        expect_live(0, 2);
        CHECK(ev.grow_to(5) == hipSuccess && ev.size() == 5);     // ... and a later call completes the list
        expect_live(0, 5);
    }
    expect_live(0, 0);
    {
        DevEvents ev;
        g_fail_in = 3;
        CHECK(ev.grow_to(5) == hipErrorOutOfMemory && ev.size() == 2);
    }                                                             // two are destroyed
    expect_live(0, 0);
    DevEvent e;
    g_fail_in = 1;
    CHECK(e.create() == hipErrorOutOfMemory && (hipEvent_t)e == nullptr);
    expect_live(0, 0);
}

int main() {
    test_ensure_and_grow();
    test_upload();
    test_moves();
    expect_live(0, 0);
    test_scopes();
    test_early_return();
    test_failure_at_every_position();
    test_events_partial();
    CHECK(g_live_blocks.load() == 0 && g_live_bytes.load() == 0 && g_live_events.load() == 0);
    CHECK(g_dev.empty() && g_pinned.empty() && g_events.empty() && g_bad_frees == 0);
    printf("own_check: ok\n");
    return 0;
}
