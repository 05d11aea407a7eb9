// knobs_check.cpp -- the environment switches' parser (csrc/knobs.hpp) on its own: defaults, clamping,
// values that do not parse.  Built and run by tests/test_oracle.py::test_knobs_parse.
#include <cstdio>
#include <cstdlib>

#include "knobs.hpp"

static int fails = 0;
#define CHECK(x)                                             \
  do {                                                       \
    if (!(x)) {                                              \
      ++fails;                                               \
      printf("FAIL line %d: %s\n", __LINE__, #x);            \
    }                                                        \
  } while (0)

static uint64_t u64_with(const char *value, uint64_t def, uint64_t min, uint64_t max) {
  if (value) setenv("RS_KNOB_T", value, 1);
  else unsetenv("RS_KNOB_T");
  return rs::env_u64("RS_KNOB_T", def, min, max);
}
static double f64_with(const char *value, double def, double min, double max) {
  if (value) setenv("RS_KNOB_T", value, 1);
  else unsetenv("RS_KNOB_T");
  return rs::env_f64("RS_KNOB_T", def, min, max);
}

int main() {
  const uint64_t big = ~0ull;
  // unset: the default
  CHECK(u64_with(nullptr, 128, 1, big) == 128);
  CHECK(f64_with(nullptr, 0.5, 0.0, 1.0) == 0.5);
  // a knob with min = 1 (RS_SNAP_CHUNK_MB, RS_TAIL_SPLIT): 0 and negatives clamp to 1, what does not
  // parse gives the default
  CHECK(u64_with("0", 128, 1, big) == 1);
  CHECK(u64_with("-3", 128, 1, big) == 1);
  CHECK(u64_with("", 128, 1, big) == 128);
  CHECK(u64_with("abc", 128, 1, big) == 128);
  CHECK(u64_with("12abc", 128, 1, big) == 128);
  CHECK(u64_with("-", 128, 1, big) == 128);
  CHECK(u64_with("64", 128, 1, big) == 64);
  CHECK(u64_with(" 64", 128, 1, big) == 64);
  // above max: max (also past 2^64)
  CHECK(u64_with("9", 2, 1, 8) == 8);
  CHECK(u64_with("8", 2, 1, 8) == 8);
  CHECK(u64_with("99999999999999999999999999", 2, 1, 8) == 8);
  CHECK(u64_with("99999999999999999999999999", 2, 1, big) == big);
  // min = 0 keeps 0 (RS_HALVES_MIN)
  CHECK(u64_with("0", 1 << 20, 0, big) == 0);
  // doubles
  CHECK(f64_with("0.2", 0.5, 0.0, 1.0) == 0.2);
  CHECK(f64_with("7", 0.5, 0.0, 1.0) == 1.0);
  CHECK(f64_with("-1", 0.5, 0.0, 1.0) == 0.0);
  CHECK(f64_with("", 0.5, 0.0, 1.0) == 0.5);
  CHECK(f64_with("x", 0.5, 0.0, 1.0) == 0.5);
  CHECK(f64_with("nan", 0.5, 0.0, 1.0) == 0.5);
  // a flag is set by any value, the empty one included
  unsetenv("RS_KNOB_T");
  CHECK(!rs::env_flag("RS_KNOB_T"));
  setenv("RS_KNOB_T", "", 1);
  CHECK(rs::env_flag("RS_KNOB_T"));
  setenv("RS_KNOB_T", "0", 1);
  CHECK(rs::env_flag("RS_KNOB_T"));
  if (!fails) printf("ok\n");
  return fails ? 1 : 0;
}
