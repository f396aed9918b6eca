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

// A switch that is on by default, with a runtime setter (sg_set_lockstep,
// sg_set_packed).  The environment is read once, by the first on() or set():
// unset means on, set means on only if its first character is '1'.
struct EnvSwitch {
    const char* name;
    int state = -1;  // -1: not read from the environment yet, else 0 / 1
    bool on() {
        if (__atomic_load_n(&state, __ATOMIC_ACQUIRE) < 0) {
            const char* e = std::getenv(name);
            int expect = -1;
            __atomic_compare_exchange_n(&state, &expect, e ? (e[0] == '1' ? 1 : 0) : 1, false,
                                        __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
        }
        return __atomic_load_n(&state, __ATOMIC_ACQUIRE) == 1;
    }
    // enable < 0 only reports; returns the previous value
    int set(int enable) {
        const int prev = on() ? 1 : 0;
        if (enable >= 0) __atomic_store_n(&state, enable ? 1 : 0, __ATOMIC_RELEASE);
        return prev;
    }
};

// an integer clamped to [lo, hi]
inline int env_int(const char* name, int lo, int hi, int dflt) {
    const char* e = std::getenv(name);
    const int v = e ? std::atoi(e) : dflt;
    return v < lo ? lo : (v > hi ? hi : v);
}

}  // namespace sg
