// sg_env.h -- the library's environment switches are read through these
// (host only, no HIP).  A caller keeps the value in a static, so that a switch
// is read once per process.
#pragma once

#include <cstdlib>

namespace sg {

// "1" turns a switch on that is off by default, "0" one off that is on
inline bool env_flag(const char* name, bool dflt) {
    const char* e = std::getenv(name);
    if (!e) return dflt;
    return dflt ? e[0] != '0' : e[0] == '1';
}

// an integer clamped to [lo, hi]
inline int env_int(const char* name, int lo, int hi, int dflt) {
    const char* e = std::getenv(name);
    const int v = e ? std::atoi(e) : dflt;
    return v < lo ? lo : (v > hi ? hi : v);
}

}  // namespace sg
