// Who owns device memory, pinned host memory and HIP events: the types of this file, each freeing what it holds in its destructor --
// no release lists, no free at the end of a function.  Part of csrc/fdcap.hip.  Includes no HIP header: hipError_t / hipSuccess,
// hipMalloc / hipFree, hipMemcpy / hipMemcpyHostToDevice, hipHostMalloc / hipHostFree and hipEvent_t / hipEventCreate /
// hipEventDestroy are whatever the includer declares (tests/ownership_cpu/own_check.cpp: counting stand-ins on a CPU).
// A destructor frees and waits for nothing: where a launch reads a temporary, the stream is synchronised before its scope ends.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <atomic>
#include <utility>
#include <vector>

namespace fdc {

// what these types hold right now, process-wide (fdcap_debug_live_allocations); touched only where something is allocated or freed
inline std::atomic<long long> g_live_blocks{0}, g_live_bytes{0}, g_live_events{0};
inline void own_count(size_t bytes, int sign) { g_live_blocks += sign; g_live_bytes += sign * (long long)bytes; }

template <class T>
struct DevBuf {               // a device block of n elements: grown on demand (contents lost), never shrunk; move-only
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = std::exchange(o.p, nullptr); n = std::exchange(o.n, 0); } return *this; }
    ~DevBuf() { release(); }
    size_t bytes() const { return std::max<size_t>(n, 1) * sizeof(T); }
    hipError_t ensure(size_t count) {     // a grow frees the old block first; a failed grow leaves the buffer empty
        if (count <= n) return hipSuccess;
        release();
        const hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
        if (e == hipSuccess) { n = count; own_count(bytes(), +1); } else p = nullptr;
        return e;
    }
    hipError_t upload(const T* h, size_t count) {
        const hipError_t e = ensure(count);
        if (e != hipSuccess) return e;
        return count ? hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    }
    void release() { if (p) { own_count(bytes(), -1); (void)hipFree(p); } p = nullptr; n = 0; }
};

template <class T>
struct PinnedBuf {            // its pinned host counterpart: ONE element, allocated once, neither copied nor moved
    T* p = nullptr;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete; PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (p) { own_count(sizeof(T), -1); (void)hipHostFree(p); } }
    hipError_t alloc() {
        if (p) return hipSuccess;
        const hipError_t e = hipHostMalloc((void**)&p, sizeof(T));
        if (e == hipSuccess) own_count(sizeof(T), +1); else p = nullptr;
        return e;
    }
};

struct DevEvent {             // one event; move-only
    hipEvent_t e{};
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete; DevEvent& operator=(const DevEvent&) = delete;
    DevEvent(DevEvent&& o) noexcept : e(std::exchange(o.e, hipEvent_t{})) {}
    DevEvent& operator=(DevEvent&& o) noexcept { if (this != &o) { destroy(); e = std::exchange(o.e, hipEvent_t{}); } return *this; }
    ~DevEvent() { destroy(); }
    hipError_t create() {
        destroy();
        const hipError_t r = hipEventCreate(&e);
        if (r == hipSuccess) g_live_events += 1; else e = hipEvent_t{};
        return r;
    }
    void destroy() { if (e) { g_live_events -= 1; (void)hipEventDestroy(e); } e = hipEvent_t{}; }
    operator hipEvent_t() const { return e; }
};

class DevEvents {             // a list of events that only grows; stays where it is
    std::vector<DevEvent> v;
public:
    DevEvents() = default;
    DevEvents(const DevEvents&) = delete; DevEvents& operator=(const DevEvents&) = delete;
    hipError_t grow_to(size_t count) {    // on failure the events made so far stay
        while (v.size() < count) {
            DevEvent d;
            const hipError_t r = d.create();
            if (r != hipSuccess) return r;
            v.push_back(std::move(d));
        }
        return hipSuccess;
    }
    hipEvent_t operator[](size_t i) const { return v[i].e; }
    size_t size() const { return v.size(); }
};

}  // namespace fdc
