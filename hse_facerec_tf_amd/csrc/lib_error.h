// The error string of a later library (every row of csrc/build.sh's table but the first), stated once: the thread-local buffer its
// hsefr_<name>_last_error* returns, set_error, and the two macros that fill it and return a status.
//
// This header DEFINES functions: it is included by exactly one translation unit of a library (geom compiles two sources; geom_linkage.hip
// has it) and by no source of libhsefr.so, where engine.hip keeps that library's own error string and the real route probe -- a second
// definition there does not link.  Every library is linked with -fvisibility=hidden, so nothing here is a dynamic symbol.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

namespace hsefr {

namespace {
thread_local char g_error[512] = "";
}

// with external linkage: in a library that compiles common.h this is the function that header declares
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
// what common.h's HSEFR_LAUNCH and launch_status ask before a launch: a later library has no plan and no probe, every launch launches
// (unused in a library that does not compile common.h)
bool route_probe() { return false; }
void route_record(const void*, const char*) {}

}  // namespace hsefr

// common.h's HSEFR_REQUIRE under a name of its own, for the sources that do not include that header
#define HSEFR_LIB_REQUIRE(cond, code, ...)   \
    do {                                     \
        if (!(cond)) {                       \
            ::hsefr::set_error(__VA_ARGS__); \
            return (code);                   \
        }                                    \
    } while (0)

// common.h's HSEFR_HIP_CHECK with the library's own two status names
#define HSEFR_LIB_HIP_CHECK(expr, nomem, hip)                                                                       \
    do {                                                                                                            \
        hipError_t _e = (expr);                                                                                     \
        if (_e != hipSuccess) {                                                                                     \
            ::hsefr::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);          \
            return _e == hipErrorOutOfMemory ? (nomem) : (hip);                                                     \
        }                                                                                                           \
    } while (0)
