// wtns_io.hpp -- the .wtns witness file and the host evaluation of a witness (rs_read_wtns,
// rs_write_wtns, rs_check_witness of include/rs_simplify.h; the extern "C" wrappers are in r1cs_io.cpp).
// Header-only and HIP-free: the library's host side includes it, the device path (witness.hpp) takes its
// header parser, and tests/wtns_host_check.cpp builds it alone under the sanitizers.
//
// The format is what the reference's generated witness programs write (writeBinWitness,
// code_producers/src/c_elements/common/main.cpp:286-333; the wasm witness_calculator.js writes the same
// bytes), all integers little endian:
//   `wtns`, u32 version = 2, u32 nSections,
//   section 1: u32 1, u64 8 + n8;    body u32 n8, the prime in n8 bytes, u32 nVars
//   section 2: u32 2, u64 n8 * nVars; body nVars values of n8 bytes, each canonical
// n8 is the .r1cs header's field size (r1cs_porting.rs:6-10).
//
// The evaluation uses its own arithmetic (a 4 x 64-bit Montgomery product, R = 2^256), not field.hpp's
// radix-2^29 one the kernels use: the host twin is an oracle for the device path, not a copy of it.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "host_common.hpp"

namespace rs {
namespace wtns {

typedef unsigned __int128 u128;

// ------------------------------------------------------------------ 256-bit host arithmetic
inline bool lt4(const uint64_t *a, const uint64_t *b) {
  for (int i = 3; i >= 0; --i)
    if (a[i] != b[i]) return a[i] < b[i];
  return false;
}
inline bool eq4(const uint64_t *a, const uint64_t *b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }
inline bool zero4(const uint64_t *a) { return (a[0] | a[1] | a[2] | a[3]) == 0; }
inline bool prime_ok(const uint64_t p[4]) { return (p[0] & 1) && ((p[1] | p[2] | p[3]) || p[0] > 1); }

struct HostField {
  uint64_t p[4];
  uint64_t n0;     // -p^-1 mod 2^64
  uint64_t r2[4];  // 2^512 mod p
};
// r = a + b mod p for a, b < p
inline void hadd(const HostField &F, const uint64_t *a, const uint64_t *b, uint64_t *r) {
  uint64_t t[4], c = 0;
  for (int i = 0; i < 4; ++i) {
    const u128 s = (u128)a[i] + b[i] + c;
    t[i] = (uint64_t)s;
    c = (uint64_t)(s >> 64);
  }
  if (c || !lt4(t, F.p)) {
    uint64_t br = 0;
    for (int i = 0; i < 4; ++i) {
      const u128 d = (u128)t[i] - F.p[i] - br;
      t[i] = (uint64_t)d;
      br = (uint64_t)(d >> 64) & 1;
    }
  }
  memcpy(r, t, 32);
}
inline HostField host_field(const uint64_t p[4]) {
  HostField F;
  memcpy(F.p, p, 32);
  uint64_t inv = 1;  // p^-1 mod 2^64 (Newton: each step doubles the correct bits)
  for (int i = 0; i < 6; ++i) inv *= 2 - p[0] * inv;
  F.n0 = 0 - inv;
  uint64_t x[4] = {1, 0, 0, 0};
  for (int i = 0; i < 512; ++i) hadd(F, x, x, x);
  memcpy(F.r2, x, 32);
  return F;
}
// a * b * 2^-256 mod p (CIOS; the sixth word takes the carry a prime just under 2^256 produces)
inline void hmul(const HostField &F, const uint64_t *a, const uint64_t *b, uint64_t *r) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) {
    uint64_t c = 0;
    for (int j = 0; j < 4; ++j) {
      const u128 s = (u128)a[j] * b[i] + t[j] + c;
      t[j] = (uint64_t)s;
      c = (uint64_t)(s >> 64);
    }
    u128 s = (u128)t[4] + c;
    t[4] = (uint64_t)s;
    t[5] = (uint64_t)(s >> 64);
    const uint64_t m = t[0] * F.n0;
    s = (u128)m * F.p[0] + t[0];
    c = (uint64_t)(s >> 64);
    for (int j = 1; j < 4; ++j) {
      s = (u128)m * F.p[j] + t[j] + c;
      t[j - 1] = (uint64_t)s;
      c = (uint64_t)(s >> 64);
    }
    s = (u128)t[4] + c;
    t[3] = (uint64_t)s;
    t[4] = t[5] + (uint64_t)(s >> 64);
  }
  if (t[4] || !lt4(t, F.p)) {
    uint64_t br = 0;
    for (int i = 0; i < 4; ++i) {
      const u128 d = (u128)t[i] - F.p[i] - br;
      t[i] = (uint64_t)d;
      br = (uint64_t)(d >> 64) & 1;
    }
  }
  memcpy(r, t, 32);
}

// ------------------------------------------------------------------ the file's header
struct Head {
  uint32_t n8 = 0;
  uint64_t prime[4] = {0, 0, 0, 0};
  uint32_t prime_id = RS_PRIME_CUSTOM;
  uint64_t n = 0;     // nVars
  uint64_t off2 = 0;  // where section 2's body starts in the file (n8 * n bytes)
};

inline uint32_t prime_id_of(const uint64_t p[4]) {
  for (uint32_t i = 0; i < 8; ++i)
    if (eq4(p, kPrimes[i])) return i;
  return RS_PRIME_CUSTOM;
}

// The section table and section 1 of the open file `fd` of `size` bytes; false with the error set.
inline bool read_head(int fd, uint64_t size, Head &H) {
  uint8_t h[12];
  if (size < 12 || !pread_all(fd, h, 12, 0)) { set_error("wtns: the file is shorter than its 12-byte header"); return false; }
  if (memcmp(h, "wtns", 4) != 0) { set_error("wtns: bad magic (the file does not start with `wtns`)"); return false; }
  uint32_t version, nsec;
  memcpy(&version, h + 4, 4);
  memcpy(&nsec, h + 8, 4);
  if (version != 2) { set_error("wtns: version " + std::to_string(version) + " is not 2"); return false; }
  bool have[3] = {false, false, false};
  uint64_t soff[3] = {0, 0, 0}, ssize[3] = {0, 0, 0};
  uint64_t off = 12;
  for (uint32_t s = 0; s < nsec; ++s) {
    uint8_t e[12];
    if (size - off < 12 || !pread_all(fd, e, 12, off)) { set_error("wtns: the section table runs past the end of the file"); return false; }
    uint32_t id;
    uint64_t len;
    memcpy(&id, e, 4);
    memcpy(&len, e + 4, 8);
    off += 12;
    if (len > size - off) { set_error("wtns: section " + std::to_string(id) + " runs past the end of the file"); return false; }
    if (id == 1 || id == 2) {
      if (have[id]) { set_error("wtns: section " + std::to_string(id) + " appears twice"); return false; }
      have[id] = true;
      soff[id] = off;
      ssize[id] = len;
    }
    off += len;
  }
  for (int id = 1; id <= 2; ++id)
    if (!have[id]) { set_error("wtns: section " + std::to_string(id) + " is missing"); return false; }
  if (ssize[1] < 4) { set_error("wtns: section 1 is shorter than its field-size word"); return false; }
  uint8_t s1[4 + 32 + 4];
  if (!pread_all(fd, s1, 4, soff[1])) { set_error("wtns: cannot read section 1"); return false; }
  memcpy(&H.n8, s1, 4);
  if (H.n8 < 8 || H.n8 > 32 || H.n8 % 8) {
    set_error("wtns: the field size n8 = " + std::to_string(H.n8) + " is not a multiple of 8 in 8..32");
    return false;
  }
  if (ssize[1] != 8ull + H.n8) { set_error("wtns: section 1's length is not 8 + n8"); return false; }
  if (!pread_all(fd, s1, 8 + H.n8, soff[1])) { set_error("wtns: cannot read section 1"); return false; }
  memcpy(H.prime, s1 + 4, H.n8);
  uint32_t nvars;
  memcpy(&nvars, s1 + 4 + H.n8, 4);
  if (!prime_ok(H.prime)) { set_error("wtns: the prime is not an odd number above 1"); return false; }
  H.prime_id = prime_id_of(H.prime);
  H.n = nvars;
  if (ssize[2] != (uint64_t)H.n8 * H.n) { set_error("wtns: section 2's length is not n8 * nVars"); return false; }
  H.off2 = soff[2];
  return true;
}

// Opens `path` and parses its header; the caller owns f.fd (Fd, pread_all: host_common.hpp).
inline bool open_head(const char *path, Fd &f, Head &H) {
  f.fd = open(path, O_RDONLY);
  struct stat sb;
  if (f.fd < 0 || fstat(f.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
    set_error(std::string("cannot read wtns file ") + path);
    return false;
  }
  return read_head(f.fd, (uint64_t)sb.st_size, H);
}

inline void witness_free(rs_witness *w) {
  if (!w) return;
  free(w->val);
  free(w);
}

inline int read_wtns(const char *path, rs_witness **out) {
  if (!path || !out) { set_error("rs_read_wtns: null argument"); return RS_E_INVALID; }
  *out = nullptr;
  Fd f;
  Head H;
  if (!open_head(path, f, H)) return RS_E_INVALID;
  // (section 2 lies inside the file, so 32 n <= 4 * the file's size: checked before this allocation)
  rs_witness *w = (rs_witness *)calloc(1, sizeof(rs_witness));
  if (!w) { set_error("out of memory"); return RS_E_INTERNAL; }
  w->prime_id = H.prime_id;
  memcpy(w->prime, H.prime, 32);
  w->n8 = H.n8;
  w->n = H.n;
  w->val = (uint64_t *)calloc(H.n ? H.n : 1, 32);
  if (!w->val) { witness_free(w); set_error("out of memory"); return RS_E_INTERNAL; }
  const uint64_t per = (1u << 20) / H.n8;  // values a block
  std::vector<uint8_t> buf((size_t)std::min<uint64_t>(per, H.n ? H.n : 1) * H.n8);
  for (uint64_t i0 = 0; i0 < H.n; i0 += per) {
    const uint64_t cnt = std::min(per, H.n - i0);
    if (!pread_all(f.fd, buf.data(), cnt * H.n8, H.off2 + i0 * H.n8)) {
      witness_free(w);
      set_error(std::string("cannot read wtns file ") + path);
      return RS_E_INVALID;
    }
    for (uint64_t i = 0; i < cnt; ++i) {
      uint64_t *v = w->val + 4 * (i0 + i);
      memcpy(v, buf.data() + i * H.n8, H.n8);
      if (!lt4(v, H.prime)) {
        witness_free(w);
        set_error("wtns: value " + std::to_string(i0 + i) + " is not below the prime");
        return RS_E_INVALID;
      }
    }
  }
  *out = w;
  return RS_OK;
}

// The prime of a witness (prime[] when it is custom, the table's otherwise); n8 fits it
inline bool witness_prime(const rs_witness *w, uint64_t p[4]) {
  if (w->prime_id == RS_PRIME_CUSTOM) memcpy(p, w->prime, 32);
  else if (w->prime_id < 8) memcpy(p, kPrimes[w->prime_id], 32);
  else return false;
  if (!prime_ok(p)) return false;
  if (w->n8 < 8 || w->n8 > 32 || w->n8 % 8) return false;
  for (uint32_t i = w->n8 / 8; i < 4; ++i)
    if (p[i]) return false;
  return true;
}

// The 12 + 12 + (8 + n8) + 12 bytes before section 2's body
inline std::vector<uint8_t> head_bytes(uint32_t n8, const uint64_t p[4], uint64_t nvars) {
  std::vector<uint8_t> h(12 + 12 + 8 + n8 + 12);
  uint8_t *d = h.data();
  auto u32 = [&](uint32_t v) { memcpy(d, &v, 4); d += 4; };
  auto u64 = [&](uint64_t v) { memcpy(d, &v, 8); d += 8; };
  memcpy(d, "wtns", 4);
  d += 4;
  u32(2);
  u32(2);
  u32(1);
  u64(8ull + n8);
  u32(n8);
  memcpy(d, p, n8);
  d += n8;
  u32((uint32_t)nvars);
  u32(2);
  u64((uint64_t)n8 * nvars);
  return h;
}

inline int write_wtns(const char *path, const rs_witness *w, const rs_output *out) {
  if (!path || !w || (w->n && !w->val)) { set_error("rs_write_wtns: null argument"); return RS_E_INVALID; }
  uint64_t p[4];
  if (!witness_prime(w, p)) { set_error("rs_write_wtns: bad prime or field size"); return RS_E_INVALID; }
  if (w->n >> 32) { set_error("rs_write_wtns: more than 2^32 - 1 values"); return RS_E_INVALID; }
  for (uint64_t i = 0; i < w->n; ++i)
    if (!lt4(w->val + 4 * i, p)) { set_error("rs_write_wtns: value " + std::to_string(i) + " is not below the prime"); return RS_E_INVALID; }
  const uint32_t n8 = w->n8;
  uint64_t nv = w->n;
  if (out) {
    if (out->n_labels && !out->label_to_wire) { set_error("rs_write_wtns: null argument"); return RS_E_INVALID; }
    if (w->n != out->n_labels) { set_error("rs_write_wtns: the witness has " + std::to_string(w->n) + " values, the result " + std::to_string(out->n_labels) + " labels"); return RS_E_INVALID; }
    if (out->n_wires > out->n_labels) { set_error("rs_write_wtns: more wires than labels"); return RS_E_INVALID; }
    nv = out->n_wires;
  }
  std::vector<uint8_t> body((size_t)(nv * n8));
  if (out) {
    for (uint64_t s = 0; s < out->n_labels; ++s) {
      const int32_t wire = out->label_to_wire[s];
      if (wire < 0) continue;
      if ((uint64_t)wire >= nv) { set_error("rs_write_wtns: a wire is not below n_wires"); return RS_E_INVALID; }
      memcpy(body.data() + (uint64_t)wire * n8, w->val + 4 * s, n8);
    }
  } else {
    for (uint64_t i = 0; i < nv; ++i) memcpy(body.data() + i * n8, w->val + 4 * i, n8);
  }
  const std::vector<uint8_t> head = head_bytes(n8, p, nv);
  FILE *f = fopen(path, "wb");
  if (!f) { set_error(std::string("cannot write ") + path); return RS_E_INVALID; }
  bool ok = fwrite(head.data(), 1, head.size(), f) == head.size();
  ok = ok && (body.empty() || fwrite(body.data(), 1, body.size(), f) == body.size());
  ok = (fclose(f) == 0) && ok;
  if (!ok) { set_error("write error"); return RS_E_INVALID; }
  return RS_OK;
}

// ------------------------------------------------------------------ the host evaluation
struct Eval {
  HostField F;
  uint64_t n = 0;             // labels
  std::vector<uint64_t> wm;   // the witness in Montgomery form (w * 2^256)
  const uint64_t *w = nullptr;  // canonical
  // sum of val[e] * w[col[e]] over e in [b, b + len): canonical.  false: a key >= n
  bool dot(const rs_lc &L, uint64_t b, uint64_t len, uint64_t *r) const {
    uint64_t acc[4] = {0, 0, 0, 0}, t[4];
    for (uint64_t e = b; e < b + len; ++e) {
      const uint32_t k = L.col[e];
      if (k >= n) return false;
      hmul(F, L.val + 4 * e, wm.data() + 4 * (uint64_t)k, t);
      hadd(F, acc, t, acc);
    }
    memcpy(r, acc, 32);
    return true;
  }
  // a * b canonical for canonical a, b
  void mul(const uint64_t *a, const uint64_t *b, uint64_t *r) const {
    uint64_t am[4];
    hmul(F, a, F.r2, am);
    hmul(F, am, b, r);
  }
};

inline bool csr_ok(const rs_lc &L, const char *name) {
  if (!L.n_rows) return true;
  bool ok = L.ptr && L.ptr[0] == 0 && L.ptr[L.n_rows] == L.nnz && (!L.nnz || (L.col && L.val));
  for (uint64_t r = 0; ok && r < L.n_rows; ++r) ok = L.ptr[r] <= L.ptr[r + 1];
  if (!ok) set_error(std::string(name) + " block: bad row pointers (ptr[0] != 0, decreasing, or ptr[n_rows] != nnz)");
  return ok;
}

struct Tally {
  rs_witness_report *rep;
  int c;
  void row(uint64_t i, bool holds) {
    ++rep->checked[c];
    if (!holds) {
      ++rep->failed[c];
      if (rep->first_failed[c] == UINT64_MAX) rep->first_failed[c] = i;
    }
  }
};

inline int check_witness(const rs_input *in, const rs_output *out, const rs_witness *w, uint32_t what, rs_witness_report *rep) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!w || !rep || (w->n && !w->val)) { set_error("rs_check_witness: null argument"); return RS_E_INVALID; }
  if (what & ~(RS_WIT_INPUT | RS_WIT_OUTPUT | RS_WIT_LOG)) { set_error("rs_check_witness: unknown bits in `what`"); return RS_E_INVALID; }
  if ((what & RS_WIT_INPUT) && !in) { set_error("rs_check_witness: RS_WIT_INPUT without an input"); return RS_E_INVALID; }
  if ((what & (RS_WIT_OUTPUT | RS_WIT_LOG)) && !out) { set_error("rs_check_witness: RS_WIT_OUTPUT / RS_WIT_LOG without an output"); return RS_E_INVALID; }
  memset(rep, 0, sizeof(*rep));
  for (uint64_t &x : rep->first_failed) x = UINT64_MAX;
  uint64_t p[4];
  if (!witness_prime(w, p)) { set_error("rs_check_witness: bad prime or field size"); return RS_E_INVALID; }
  if (in) {
    uint64_t pi[4];
    if (!prime_of(in, pi)) { set_error("unknown prime"); return RS_E_INVALID; }
    if (!eq4(p, pi)) { set_error("rs_check_witness: the witness's prime is not the input's"); return RS_E_INVALID; }
  }
  if ((what & RS_WIT_INPUT) && w->n != in->max_signal) {
    set_error("rs_check_witness: the witness has " + std::to_string(w->n) + " values, the input " + std::to_string(in->max_signal) + " labels");
    return RS_E_INVALID;
  }
  if ((what & (RS_WIT_OUTPUT | RS_WIT_LOG)) && w->n != out->n_labels) {
    set_error("rs_check_witness: the witness has " + std::to_string(w->n) + " values, the result " + std::to_string(out->n_labels) + " labels");
    return RS_E_INVALID;
  }
  if (w->n == 0 || w->val[0] != 1 || w->val[1] || w->val[2] || w->val[3]) { set_error("rs_check_witness: w[0] is not 1 (key 0 is the constant)"); return RS_E_INVALID; }
  Eval ev;
  ev.F = host_field(p);
  ev.n = w->n;
  ev.w = w->val;
  ev.wm.resize(4 * w->n);
  for (uint64_t i = 0; i < w->n; ++i) {
    if (!lt4(w->val + 4 * i, p)) { set_error("rs_check_witness: value " + std::to_string(i) + " is not below the prime"); return RS_E_INVALID; }
    hmul(ev.F, w->val + 4 * i, ev.F.r2, ev.wm.data() + 4 * i);
  }
  const char *bad_key = "rs_check_witness: a key is not below the number of labels";
  uint64_t a[4], b[4], c[4], ab[4];
  if (what & RS_WIT_INPUT) {
    const rs_lc *lin[3] = {&in->cons_eq, &in->eq, &in->linear};
    const char *nm[3] = {"cons_eq", "eq", "linear"};
    for (int q = 0; q < 3; ++q) {
      const rs_lc &L = *lin[q];
      if (!csr_ok(L, nm[q])) return RS_E_INVALID;
      Tally t{rep, q};
      for (uint64_t r = 0; r < L.n_rows; ++r) {
        if (!ev.dot(L, L.ptr[r], L.ptr[r + 1] - L.ptr[r], c)) { set_error(bad_key); return RS_E_INVALID; }
        t.row(r, zero4(c));
      }
    }
    if (in->nl_a.n_rows != in->nl_b.n_rows || in->nl_a.n_rows != in->nl_c.n_rows) { set_error("non-linear blocks differ in row count"); return RS_E_INVALID; }
    if (!csr_ok(in->nl_a, "nl_a") || !csr_ok(in->nl_b, "nl_b") || !csr_ok(in->nl_c, "nl_c")) return RS_E_INVALID;
    Tally t{rep, RS_WITC_NONLINEAR};
    for (uint64_t r = 0; r < in->nl_a.n_rows; ++r) {
      if (!ev.dot(in->nl_a, in->nl_a.ptr[r], in->nl_a.ptr[r + 1] - in->nl_a.ptr[r], a) ||
          !ev.dot(in->nl_b, in->nl_b.ptr[r], in->nl_b.ptr[r + 1] - in->nl_b.ptr[r], b) ||
          !ev.dot(in->nl_c, in->nl_c.ptr[r], in->nl_c.ptr[r + 1] - in->nl_c.ptr[r], c)) {
        set_error(bad_key);
        return RS_E_INVALID;
      }
      ev.mul(a, b, ab);
      t.row(r, eq4(ab, c));
    }
  }
  if (what & RS_WIT_OUTPUT) {
    const rs_lc *L[3] = {&out->a, &out->b, &out->c};
    const uint32_t *len[3] = {out->a_len, out->b_len, out->c_len};
    const uint64_t njump[3] = {out->a_njump, out->b_njump, out->c_njump};
    rs_rows it[3];
    for (int q = 0; q < 3; ++q) {
      if (out->n_constraints && !len[q] && !L[q]->ptr) { set_error("rows without a ptr array"); return RS_E_INVALID; }
      if (L[q]->nnz && (!L[q]->col || !L[q]->val)) { set_error("entries without col/val"); return RS_E_INVALID; }
      rs_rows_begin(out, q, &it[q]);
    }
    Tally t{rep, RS_WITC_OUTPUT};
    uint64_t *d[3] = {a, b, c};
    for (uint64_t r = 0; r < out->n_constraints; ++r) {
      for (int q = 0; q < 3; ++q) {
        if (len[q] && (len[q][r] & RS_ROW_JUMP) && (it[q].j >= njump[q] || !it[q].jump)) { set_error("row layout: more jumping rows than jump offsets"); return RS_E_INVALID; }
        uint64_t rb, rl;
        rs_rows_next(&it[q], r, &rb, &rl);
        if (rb > L[q]->nnz || rl > L[q]->nnz - rb) { set_error("row layout reaches past the block's entries"); return RS_E_INVALID; }
        if (!ev.dot(*L[q], rb, rl, d[q])) { set_error(bad_key); return RS_E_INVALID; }
      }
      ev.mul(a, b, ab);
      t.row(r, eq4(ab, c));
    }
  }
  if ((what & RS_WIT_LOG) && out->n_log) {
    const rs_lc &L = out->log_to;
    if (!out->log_from || !L.ptr) { set_error("rs_check_witness: a log without log_from / log_to"); return RS_E_INVALID; }
    if (L.nnz && (!L.col || !L.val)) { set_error("entries without col/val"); return RS_E_INVALID; }
    Tally t{rep, RS_WITC_LOG};
    for (uint64_t r = 0; r < out->n_log; ++r) {
      if (L.ptr[r] > L.ptr[r + 1] || L.ptr[r + 1] > L.nnz) { set_error("log_to block: bad row pointers"); return RS_E_INVALID; }
      if (out->log_from[r] >= ev.n || !ev.dot(L, L.ptr[r], L.ptr[r + 1] - L.ptr[r], c)) { set_error(bad_key); return RS_E_INVALID; }
      t.row(r, eq4(ev.w + 4 * (uint64_t)out->log_from[r], c));
    }
  }
  rep->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  rep->kernel_ms = rep->total_ms;
  return RS_OK;
}

// ------------------------------------------------------------------ the lift (ABI 14)
// A wire witness v (one value per wire of `out`) back to one value per --O0 label through the
// substitution log: entry i says w[log_from[i]] = log_to[i] . w.  The owner of a label is its last entry
// (constant_eq_simplification logs every row, the map keeps the last); an entry that is not its label's
// owner is shadowed and defines nothing.  A label with a wire takes the wire's value, a label with an
// owner the owner's dot product, every other label 0 (free).  The log is in elimination order: an owner
// entry's owned keys belong to later entries, so one pass from the last entry to the first evaluates
// every entry after everything it reads; the levels (0: no owned key, else 1 + the deepest owned key's)
// come out of the same pass.  The device path (lift.hpp) must agree to the bit.
inline int lift_witness(const rs_output *out, const rs_witness *v, rs_witness **wout, rs_lift_report *rep) {
  const auto t0 = std::chrono::steady_clock::now();
  if (wout) *wout = nullptr;
  if (!out || !v || !wout || !rep || (v->n && !v->val) || (out->n_labels && !out->label_to_wire) ||
      (out->n_log && (!out->log_from || !out->log_to.ptr)) || (out->log_to.nnz && (!out->log_to.col || !out->log_to.val))) {
    set_error("rs_lift_witness: null argument");
    return RS_E_INVALID;
  }
  memset(rep, 0, sizeof(*rep));
  const uint64_t L = out->n_labels, Wn = out->n_wires, n = out->n_log;
  const rs_lc &T = out->log_to;
  uint64_t p[4];
  if (!witness_prime(v, p)) { set_error("rs_lift_witness: bad prime or field size"); return RS_E_INVALID; }
  if (v->n != Wn) {
    set_error("rs_lift_witness: the witness has " + std::to_string(v->n) + " values, the result " + std::to_string(Wn) + " wires");
    return RS_E_INVALID;
  }
  if (L == 0 || L > 0x7fffffffull) { set_error("rs_lift_witness: the result needs 1 .. 2^31 - 1 labels"); return RS_E_INVALID; }
  if (v->n == 0 || v->val[0] != 1 || v->val[1] || v->val[2] || v->val[3]) { set_error("rs_lift_witness: w[0] is not 1 (key 0 is the constant)"); return RS_E_INVALID; }
  for (uint64_t i = 0; i < Wn; ++i)
    if (!lt4(v->val + 4 * i, p)) { set_error("rs_lift_witness: value " + std::to_string(i) + " is not below the prime"); return RS_E_INVALID; }
  if (n) {
    bool ok = T.ptr[0] == 0 && T.ptr[n] == T.nnz;
    for (uint64_t r = 0; ok && r < n; ++r) ok = T.ptr[r] <= T.ptr[r + 1];
    if (!ok) { set_error("rs_lift_witness: log_to block: bad row pointers (ptr[0] != 0, decreasing, or ptr[n_log] != nnz)"); return RS_E_INVALID; }
  }
  // the owners, one forward pass: owner[s] = 1 + the last entry whose `from` is s
  std::vector<uint64_t> owner(L, 0);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t f = out->log_from[i];
    if (f >= L) { set_error("rs_lift_witness: log entry " + std::to_string(i) + ": `from` is not below the number of labels"); return RS_E_INVALID; }
    if (f == 0) { set_error("rs_lift_witness: log entry " + std::to_string(i) + ": `from` is the constant (label 0)"); return RS_E_INVALID; }
    if (out->label_to_wire[f] >= 0) { set_error("rs_lift_witness: log entry " + std::to_string(i) + ": `from` still has a wire"); return RS_E_INVALID; }
    owner[f] = i + 1;
  }
  for (uint64_t e = 0; e < T.nnz; ++e)
    if (T.col[e] >= L) { set_error("rs_lift_witness: a key is not below the number of labels"); return RS_E_INVALID; }
  Eval ev;
  ev.F = host_field(p);
  ev.n = L;
  ev.wm.assign(4 * L, 0);
  for (uint64_t s = 0; s < L; ++s) {
    const int32_t wire = out->label_to_wire[s];
    if (wire >= 0) {
      if ((uint64_t)wire >= Wn) { set_error("rs_lift_witness: a wire is not below n_wires"); return RS_E_INVALID; }
      hmul(ev.F, v->val + 4 * (uint64_t)wire, ev.F.r2, ev.wm.data() + 4 * s);
    } else if (owner[s]) {
      ++rep->lifted;
    } else {
      ++rep->free_labels;
    }
  }
  rep->n_labels = L;
  rep->n_wires = Wn;
  rep->shadowed = n - rep->lifted;
  // the entries, last to first
  std::vector<uint64_t> level(n, 0);
  uint64_t c[4];
  for (uint64_t i = n; i-- > 0;) {
    const uint64_t f = out->log_from[i];
    if (owner[f] != i + 1) continue;
    uint64_t lv = 0;
    for (uint64_t e = T.ptr[i]; e < T.ptr[i + 1]; ++e) {
      const uint64_t o = owner[T.col[e]];
      if (!o) continue;
      if (o - 1 <= i) {
        set_error("rs_lift_witness: the log is not in elimination order: entry " + std::to_string(i) + " reads the label entry " +
                  std::to_string(o - 1) + " defines");
        return RS_E_INVALID;
      }
      lv = std::max(lv, level[o - 1] + 1);
    }
    level[i] = lv;
    rep->levels = std::max(rep->levels, lv + 1);
    rep->entries += T.ptr[i + 1] - T.ptr[i];
    ev.dot(T, T.ptr[i], T.ptr[i + 1] - T.ptr[i], c);  // (every key is below L: checked above)
    hmul(ev.F, c, ev.F.r2, ev.wm.data() + 4 * f);
  }
  rs_witness *w = (rs_witness *)calloc(1, sizeof(rs_witness));
  if (!w) { set_error("out of memory"); return RS_E_INTERNAL; }
  w->prime_id = prime_id_of(p);
  memcpy(w->prime, p, 32);
  w->n8 = v->n8;
  w->n = L;
  w->val = (uint64_t *)calloc(L, 32);
  if (!w->val) { witness_free(w); set_error("out of memory"); return RS_E_INTERNAL; }
  const uint64_t one[4] = {1, 0, 0, 0};
  for (uint64_t s = 0; s < L; ++s) hmul(ev.F, ev.wm.data() + 4 * s, one, w->val + 4 * s);  // out of Montgomery form
  *wout = w;
  rep->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return RS_OK;
}

}  // namespace wtns
}  // namespace rs
