// c_api_internal.h — what c_api.cpp (the product ABI, include/mi355vits.h) and lab_api.cpp (the test / bench / probe hooks,
// include/mi355vits_lab.h) share: the handle, the exception fence, and the hooks' device scope.
#pragma once
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "engine.h"

using namespace m355;

struct mi355vits_engine {
    std::unique_ptr<Engine> eng;
    std::string err;
};

// message of a failed call that has no handle (create, the device-level hooks): one per thread and library, read by
// mi355vits_last_error(NULL) — external linkage so that both translation units see the same string
inline std::string& create_error() { static thread_local std::string e; return e; }

namespace {

template <typename F>
int guarded(mi355vits_handle h, F&& fn) {
    std::string* err = h ? &h->err : &create_error();
    try {
        fn();
        return MI355VITS_OK;
    } catch (const EngineError& e) {
        *err = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        *err = "out of host memory";
        return MI355VITS_ERR_NOMEM;
    } catch (const std::exception& e) {
        *err = e.what();
        return std::string(e.what()).rfind("HIP error", 0) == 0 ? MI355VITS_ERR_DEVICE : MI355VITS_ERR_INTERNAL;
    } catch (...) {
        *err = "unknown error";
        return MI355VITS_ERR_INTERNAL;
    }
}

}  // namespace

namespace {
// HookScope — the device side of one hook call (lab_api.cpp).  It owns every buffer until it goes out of scope; counts are in elements
// of T.  A NULL host pointer stays NULL on the device (an absent optional input: nothing is allocated); a non-NULL one of zero
// elements gets a valid pointer.  inout() sends the caller's prior contents up, so that a position no kernel writes comes back as it
// was.  finish() synchronises the device, asks for a launch error, and only then copies back what inout() registered, in that order:
// when anything throws before it, nothing is copied and everything is freed.
class HookScope {
  public:
    HookScope() = default;  // the device-level hooks that take no device run on the current one
    explicit HookScope(int device) { HIP_CHECK(hipSetDevice(device)); }
    HookScope(const HookScope&) = delete;
    HookScope& operator=(const HookScope&) = delete;

    template <typename T> T* scratch(size_t n) {
        bufs_.push_back(std::make_unique<DevBuf>(n * sizeof(T)));
        return bufs_.back()->as<T>();
    }
    template <typename T> T* filled(size_t n, int byte) {
        T* d = scratch<T>(n);
        if (n) HIP_CHECK(hipMemset(d, byte, n * sizeof(T)));
        return d;
    }
    template <typename T> T* in(const T* host, size_t n) {
        if (!host) return nullptr;
        T* d = scratch<T>(n);
        if (n) HIP_CHECK(hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <typename T> T* in(const std::vector<T>& host) {  // never NULL: a vector is not optional
        T* d = scratch<T>(host.size());
        if (!host.empty()) HIP_CHECK(hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    // n elements into a range of a buffer this scope already owns (a row at its offset inside a padded or shared buffer)
    template <typename T> void put(T* dev, const T* host, size_t n) {
        if (n) HIP_CHECK(hipMemcpy(dev, host, n * sizeof(T), hipMemcpyHostToDevice));
    }
    template <typename T> T* inout(T* host, size_t n) {
        T* d = in(host, n);
        if (d) owed_.push_back({host, d, n * sizeof(T)});
        return d;
    }
    // once per launch sequence whose results the host needs (the two-phase hooks call it after each phase)
    void finish() {
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipGetLastError());
        for (const Owed& o : owed_)
            if (o.bytes) HIP_CHECK(hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost));
    }
    // after finish(): n elements of H from a device pointer, for the hooks that look at or rearrange a result before they hand it out
    template <typename H, typename D> void fetch(H* host, const D* dev, size_t n) {
        static_assert(sizeof(H) == sizeof(D), "fetch: host and device elements of one size");
        if (n) HIP_CHECK(hipMemcpy(host, dev, n * sizeof(H), hipMemcpyDeviceToHost));
    }

  private:
    struct Owed { void* host; const void* dev; size_t bytes; };
    std::vector<std::unique_ptr<DevBuf>> bufs_;
    std::vector<Owed> owed_;
};
}  // namespace

