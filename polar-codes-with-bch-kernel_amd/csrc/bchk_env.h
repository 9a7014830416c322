// Environment knobs: every BCHK_* variable the library reads goes through one of these, so
// the names can be listed (DESIGN.md "Environment knobs", tests/test_knob_table.py). An
// unset variable leaves *v as it is -- the default.
#pragma once
#include <stdint.h>
#include <stdlib.h>

namespace bchk {

inline bool env_flag(const char *name) { return getenv(name) != nullptr; }

inline bool env_int(const char *name, int *v, int lo, int hi) {
    const char *e = getenv(name);
    if (!e) return false;
    const int x = atoi(e);
    *v = x < lo ? lo : x > hi ? hi : x;
    return true;
}

// an on / off switch: NAME=0 is off, any other integer on
inline bool env_bool(const char *name, bool *v) {
    const char *e = getenv(name);
    if (!e) return false;
    *v = atoi(e) != 0;
    return true;
}

inline bool env_u64(const char *name, uint64_t *v) {
    const char *e = getenv(name);
    if (!e) return false;
    *v = strtoull(e, nullptr, 10);
    return true;
}

inline bool env_double(const char *name, double *v, double lo, double hi) {
    const char *e = getenv(name);
    if (!e) return false;
    const double x = atof(e);
    *v = x < lo ? lo : x > hi ? hi : x;
    return true;
}

}  // namespace bchk
