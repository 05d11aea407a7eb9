// knobs.hpp -- the environment switches of the engine ("Tuning switches"), parsed in one
// place.  Host only; expects nothing.  A missing or unparsable value gives the default, a value
// outside [min, max] is clamped.  When a switch is read (once per process, at engine creation, or on
// every call) is its call site's business: these functions read the environment each time.
#pragma once

#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdlib>

namespace rs {

// set at all, the empty string included
inline bool env_flag(const char *name) { return getenv(name) != nullptr; }

inline uint64_t env_u64(const char *name, uint64_t def, uint64_t min, uint64_t max) {
  const char *s = getenv(name);
  if (!s) return def;
  while (*s == ' ' || *s == '\t') ++s;
  const bool neg = *s == '-';
  if (neg) ++s;
  if (*s < '0' || *s > '9') return def;  // empty, not a number
  char *end = nullptr;
  errno = 0;
  const unsigned long long v = strtoull(s, &end, 10);
  if (*end != '\0') return def;
  if (neg) return min;  // below every range
  if (errno == ERANGE) return max;
  return v < min ? min : (v > max ? max : (uint64_t)v);
}

inline double env_f64(const char *name, double def, double min, double max) {
  const char *s = getenv(name);
  if (!s) return def;
  char *end = nullptr;
  const double v = strtod(s, &end);
  if (end == s || *end != '\0' || std::isnan(v)) return def;
  return v < min ? min : (v > max ? max : v);
}

}  // namespace rs
