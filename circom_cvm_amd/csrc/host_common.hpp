// host_common.hpp -- shared host-side helpers of librs_simplify (error state, prime table,
// owned rs_lc blocks).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/rs_simplify.h"

namespace rs {

void set_error(const std::string &msg);

// program_structure/src/utils/constants.rs:3-13, little-endian limbs.
extern const uint64_t kPrimes[8][4];

inline bool prime_of(const rs_input *in, uint64_t p[4]) {
  if (in->prime_id == RS_PRIME_CUSTOM) {
    memcpy(p, in->prime, 32);
    return (p[0] & 1) && (p[0] | p[1] | p[2] | p[3]) > 1;
  }
  if (in->prime_id >= 8) return false;
  memcpy(p, kPrimes[in->prime_id], 32);
  return true;
}

inline int bit_length(const uint64_t p[4]) {
  for (int i = 3; i >= 0; --i)
    if (p[i]) return 64 * i + 64 - __builtin_clzll(p[i]);
  return 0;
}

// r1cs_porting.rs:6-10
inline int field_size_bytes(const uint64_t p[4]) {
  int bits = bit_length(p);
  return bits % 64 == 0 ? bits / 8 : (bits / 64 + 1) * 8;
}

// Host-owned CSR block builder.
struct Block {
  std::vector<uint64_t> ptr{0};
  std::vector<uint32_t> col;
  std::vector<uint64_t> val;  // 4 limbs per entry
  void push(uint32_t k, const uint64_t v[4]) {
    col.push_back(k);
    val.insert(val.end(), v, v + 4);
  }
  void end_row() { ptr.push_back(col.size()); }
  uint64_t rows() const { return ptr.size() - 1; }
};

// Moves a Block into malloc'ed rs_lc arrays (freed by free_lc).
inline void to_lc(Block &b, rs_lc &lc) {
  lc.n_rows = b.rows();
  lc.nnz = b.col.size();
  lc.ptr = (uint64_t *)malloc(sizeof(uint64_t) * b.ptr.size());
  memcpy(lc.ptr, b.ptr.data(), sizeof(uint64_t) * b.ptr.size());
  lc.col = (uint32_t *)malloc(sizeof(uint32_t) * (b.col.size() ? b.col.size() : 1));
  if (!b.col.empty()) memcpy(lc.col, b.col.data(), sizeof(uint32_t) * b.col.size());
  lc.val = (uint64_t *)malloc(sizeof(uint64_t) * (b.val.size() ? b.val.size() : 4));
  if (!b.val.empty()) memcpy(lc.val, b.val.data(), sizeof(uint64_t) * b.val.size());
  b = Block();
}

// r1cs_io.cpp: the output's custom-gate sections (4 and 5) from an --O0 file, label_to_wire applied
bool r1cs_gate_sections(const char *o0_r1cs, const int32_t *l2w, uint64_t n_labels, std::vector<uint8_t> &out,
                        bool &present);

// Section table of an .r1cs file (r1cs_writer.rs:147-204): the first section of each type 1-5.
struct R1csSections {
  bool have[6] = {};
  uint64_t off[6] = {}, size[6] = {};
};
// What an --O0 file's small sections say (header, custom gates): everything of the rs_input but the
// six blocks.
struct R1csO0Head {
  uint32_t fs = 0;  // bytes of a field element in the file: 8, 16, 24 or 32
  uint64_t prime[4] = {0, 0, 0, 0};
  uint32_t prime_id = RS_PRIME_CUSTOM;
  uint32_t n_out = 0, n_pub = 0, n_prv = 0, n_cons = 0;
  uint64_t n_labels = 0;
  std::vector<uint32_t> forbidden;  // sorted, distinct
};
// r1cs_io.cpp: the small sections parsed (each given alone; s4 / s5 nullptr when absent), and an --O0
// file opened through preads of the section table and those sections only (the caller closes *fd)
bool r1cs_o0_small(const uint8_t *s1, uint64_t size1, const uint8_t *s4, uint64_t size4, const uint8_t *s5, uint64_t size5,
                   R1csO0Head &H);
bool r1cs_o0_open(const char *path, int *fd, R1csSections &S, R1csO0Head &H);

// An open file, closed on every way out of its scope (release(): the caller closes it and sees the verdict)
struct Fd {
  int fd = -1;
  ~Fd() {
    if (fd >= 0) close(fd);
  }
  int release() {
    const int f = fd;
    fd = -1;
    return f;
  }
};
// All n bytes at `off`, over short reads / writes; false: an error, or the file ends first
inline bool pread_all(int fd, void *dst, uint64_t n, uint64_t off) {
  uint8_t *d = (uint8_t *)dst;
  while (n) {
    const ssize_t g = pread(fd, d, n, (off_t)off);
    if (g <= 0) return false;
    d += g;
    n -= (uint64_t)g;
    off += (uint64_t)g;
  }
  return true;
}
inline bool pwrite_all(int fd, const void *src, uint64_t n, uint64_t off) {
  const uint8_t *p = (const uint8_t *)src;
  while (n) {
    const ssize_t w = pwrite(fd, p, n, (off_t)off);
    if (w <= 0) return false;
    p += w;
    n -= (uint64_t)w;
    off += (uint64_t)w;
  }
  return true;
}

inline void free_lc(rs_lc &lc) {
  free(lc.ptr);
  free(lc.col);
  free(lc.val);
  lc.ptr = nullptr;
  lc.col = nullptr;
  lc.val = nullptr;
}

}  // namespace rs
