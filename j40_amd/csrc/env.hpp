// j40_amd/csrc/env.hpp -- the one way the library reads its J40HIP_* environment switches (INTEGRATION.md lists them).
// Nothing is cached here: a call site that reads its switch once per process keeps the value in a `static const` of its own.
// A variable set to the empty string counts as not set.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>

namespace j40hip {

// the variable's text; nullptr when it is not set
inline const char *env_str(const char *name) { const char *e = getenv(name); return e && *e ? e : nullptr; }
// a number between lo and hi; `dflt` (as it is, not clamped) when the variable is not set
inline int env_int(const char *name, int dflt, int lo, int hi) { const char *e = env_str(name); return e ? std::max(lo, std::min(hi, atoi(e))) : dflt; }
// a non-zero number: on; zero or anything that is not a number: off; `dflt` when the variable is not set
inline bool env_on(const char *name, bool dflt) { const char *e = env_str(name); return e ? atoi(e) != 0 : dflt; }

} // namespace j40hip
