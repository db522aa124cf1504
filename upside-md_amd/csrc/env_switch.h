// The one reader of the environment switches (UPSIDE_HIP_*: INTEGRATION.md section 6 lists them all).
// Switches that select a code path or size a capacity are read once, into PlanSwitches (launch_plan.h); a diagnostic switch is written
// `static const int x = env_int(...);` at its point of use.
#pragma once
#include <cstdlib>

inline const char* env_str(const char* name) { return getenv(name); }            // nullptr when unset
inline bool env_set(const char* name) { return env_str(name) != nullptr; }
inline int env_int(const char* name, int dflt) { const char* e = env_str(name); return e ? atoi(e) : dflt; }
inline float env_float(const char* name, float dflt) { const char* e = env_str(name); return e ? (float)atof(e) : dflt; }
