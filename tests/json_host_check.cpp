// The host side of csrc/json_write.hpp's conversion helpers (json_dec, json_dig32: the code the kernels
// run, compiled for the host): every line of stdin is four hexadecimal limbs, least significant first;
// the answer is the value in decimal as the writers' kernels put it together.  A stand-alone program
// (tests/test_json_abi.py builds it with the address and undefined-behaviour sanitizers).
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>
#define __host__
#define __device__
#define __forceinline__ inline
#include "json_write.hpp"

int main() {
  uint64_t v[4];
  while (scanf("%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &v[0], &v[1], &v[2], &v[3]) == 4) {
    uint32_t d[9];
    const int top = json_dec(v, d);
    std::string s;
    for (int k = top; k >= 0; --k) {
      const int w = k == top ? json_dig32(d[k]) : 9;
      std::string part(w, '0');
      uint32_t x = d[k];
      for (int i = w - 1; i >= 0; --i) {
        part[i] = (char)('0' + x % 10);
        x /= 10;
      }
      if (x) return 1;  // d[k] has more digits than its field
      s += part;
    }
    printf("%s %d\n", s.c_str(), 9 * top + json_dig32(d[top]));
  }
  return 0;
}
