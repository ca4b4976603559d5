// Shared by the C ABI's translation units (capi_*.cpp, host_api.cpp): the
// thread's error text and the entry points' exception barrier.  No HIP header.
#pragma once
#include <cstddef>
#include <stdexcept>
#include <string>

#include "riptide_amd.h"

namespace rt {

inline std::string& last_error()   // rt_last_error's text, per thread
{
    thread_local std::string err;
    return err;
}

inline int fail(int code, const std::string& msg)
{
    last_error() = msg;
    return code;
}

struct HipError : std::runtime_error {   // a failed HIP runtime call (capi_device.hpp ck): RT_EHIP
    using std::runtime_error::runtime_error;
};

// Exception barrier for every entry point.
template <class F>
int guarded(F&& f)
{
    try {
        return f();
    } catch (const std::invalid_argument& e) {
        return fail(RT_EINVAL, e.what());
    } catch (const HipError& e) {
        return fail(RT_EHIP, e.what());
    } catch (const std::exception& e) {
        return fail(RT_EINTERNAL, e.what());
    } catch (...) {
        return fail(RT_EINTERNAL, "unknown error");
    }
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

}  // namespace rt
