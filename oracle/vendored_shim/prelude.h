/* prelude.h -- force-included (-include) ahead of every translation unit of the reference's
 * vendored polar library (out/external/ of the reference tree) when oracle/Makefile builds
 * oracle/_ref/polar_ref. TEST INFRASTRUCTURE ONLY. It names what that library expects
 * from MSVC's runtime, in terms of the C++ and POSIX libraries; it holds no text of the
 * library or of MSVC's headers. */
#pragma once
#include <algorithm>
#include <cassert>
#include <chrono>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <strings.h>

/* MSVC's std::exception can be built from a message; the library relies on that
 * (headers/external/misc.h:59-69). Every later use of the name gets this stand-in. */
namespace std {
struct bchk_msg_exception : exception {
    const char *msg;
    bchk_msg_exception() : msg("") {}
    bchk_msg_exception(const char *s) : msg(s) {}
    const char *what() const noexcept override { return msg; }
};
}  // namespace std
#define exception bchk_msg_exception

#define vsprintf_s vsnprintf
#define sprintf_s snprintf
#define _stricmp strcasecmp
inline char *strcpy_s(char *d, const char *s) { return strcpy(d, s); }
inline char *strcpy_s(char *d, size_t, const char *s) { return strcpy(d, s); }

inline void *_aligned_malloc(size_t n, size_t a) {
    void *p = nullptr;
    if (a < sizeof(void *)) a = sizeof(void *);
    return posix_memalign(&p, a, n ? n : 1) ? nullptr : p;
}
#define _aligned_free free

#define _ASSERT(x) assert(x)
#define _ASSERTE(x) assert(x)
#define _CrtCheckMemory() 1

using std::endl;
