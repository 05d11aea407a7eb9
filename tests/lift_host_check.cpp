// Stand-alone host build of the lift of circom_cvm_amd/csrc/wtns_io.hpp (rs_lift_witness's body), driven by
// tests/test_lift_abi.py under the address and undefined-behaviour sanitizers (built together with
// csrc/host_common.cpp: the error text and the prime table).
//   lift_host_check
// Hand-built logs over F_257 and over bn128: a three-level chain with a shadowed entry and a free label
// against values worked out here with plain integers; a 5,000-key row (every key's value p - 1, every
// coefficient p - 1) whose value is 5,000 mod p, read by an entry one level up; the empty log; and every
// refusal the host can see, each of which must return RS_E_INVALID with a message and leave *w NULL, with
// a good call right after it.  Prints `ok` and exits 0, or says what went wrong and exits 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wtns_io.hpp"

using namespace rs;

static int fail(const std::string &what) {
  fprintf(stderr, "lift_host_check: %s\n", what.c_str());
  return 1;
}

// A log and a result header over caller-owned vectors
struct Case {
  std::vector<int32_t> l2w;
  std::vector<uint32_t> from, col;
  std::vector<uint64_t> ptr{0}, val;
  std::vector<uint64_t> v;  // the wire witness, 4 limbs a value
  uint64_t prime[4] = {257, 0, 0, 0};
  uint32_t n8 = 8;
  void entry(uint32_t f, const std::vector<std::pair<uint32_t, uint64_t>> &to) {
    from.push_back(f);
    for (const auto &kv : to) {
      col.push_back(kv.first);
      val.insert(val.end(), {kv.second, 0, 0, 0});
    }
    ptr.push_back(col.size());
  }
  void value(uint64_t x) { v.insert(v.end(), {x, 0, 0, 0}); }
  rs_output out() {
    rs_output o{};
    o.n_labels = l2w.size();
    o.label_to_wire = l2w.data();
    for (int32_t x : l2w) o.n_wires += x >= 0;
    o.n_log = from.size();
    o.log_from = from.data();
    o.log_to = rs_lc{(uint64_t)from.size(), (uint64_t)col.size(), ptr.data(), col.data(), val.data()};
    return o;
  }
  rs_witness wit() {
    rs_witness w{};
    w.prime_id = RS_PRIME_CUSTOM;
    memcpy(w.prime, prime, 32);
    w.n8 = n8;
    w.n = v.size() / 4;
    w.val = v.data();
    return w;
  }
};

// labels 0..6: wires 0, 1, 2; label 3 := 2 w1 + 5; label 4 := 3 w3 + w2; label 5 := w4 + w6 (6 is free);
// and a shadowed first entry for label 3
static Case small_case() {
  Case c;
  c.l2w = {0, 1, 2, -1, -1, -1, -1};
  c.entry(3, {{0, 9}});                  // shadowed: a later entry owns label 3
  c.entry(5, {{4, 1}, {6, 1}});          // level 2
  c.entry(4, {{2, 1}, {3, 3}});          // level 1
  c.entry(3, {{0, 5}, {1, 2}});          // level 0
  c.value(1);
  c.value(10);
  c.value(20);
  return c;
}

static int expect_refusal(Case c, const char *word, const char *what) {
  rs_output o = c.out();
  rs_witness v = c.wit();
  rs_witness *w = (rs_witness *)&v;  // (must be reset to NULL)
  rs_lift_report rep;
  const int rc = wtns::lift_witness(&o, &v, &w, &rep);
  if (rc != RS_E_INVALID || w) return fail(std::string(what) + " was not refused");
  if (!strstr(rs_last_error(), word)) return fail(std::string(what) + ": the message `" + rs_last_error() + "` lacks `" + word + "`");
  // a good call right after it
  Case g = small_case();
  o = g.out();
  v = g.wit();
  if (wtns::lift_witness(&o, &v, &w, &rep) != RS_OK || !w) return fail(std::string("a good call after ") + what + " failed");
  wtns::witness_free(w);
  return 0;
}

static int small() {
  Case c = small_case();
  rs_output o = c.out();
  rs_witness v = c.wit();
  rs_witness *w = nullptr;
  rs_lift_report rep;
  if (wtns::lift_witness(&o, &v, &w, &rep) != RS_OK) return fail(std::string("small: ") + rs_last_error());
  const uint64_t want[7] = {1, 10, 20, 25, 95, 95, 0};
  for (int s = 0; s < 7; ++s)
    if (w->val[4 * s] != want[s] || w->val[4 * s + 1] || w->val[4 * s + 2] || w->val[4 * s + 3]) return fail("small: wrong value at label " + std::to_string(s));
  if (w->n != 7 || w->n8 != 8 || w->prime[0] != 257) return fail("small: wrong header");
  if (rep.n_labels != 7 || rep.n_wires != 3 || rep.lifted != 3 || rep.free_labels != 1 || rep.shadowed != 1 || rep.levels != 3 || rep.entries != 6 ||
      rep.in_ms != 0 || rep.kernel_ms != 0)
    return fail("small: wrong report");
  wtns::witness_free(w);
  return 0;
}

// 5,000 wires of value p - 1, one level-0 row over all of them with coefficient p - 1 (value 5,000 mod p)
// and one level-1 row that doubles it; over bn128 too (4 limbs)
static int long_row(bool bn128) {
  Case c;
  const uint64_t bn[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
  if (bn128) {
    memcpy(c.prime, bn, 32);
    c.n8 = 32;
  }
  const uint32_t n = 5000;
  uint64_t m1[4];
  memcpy(m1, c.prime, 32);
  m1[0] -= 1;  // p - 1 (p is odd)
  c.l2w.push_back(0);
  c.value(1);
  for (uint32_t i = 1; i <= n; ++i) {
    c.l2w.push_back((int32_t)i);
    c.v.insert(c.v.end(), m1, m1 + 4);
  }
  c.l2w.push_back(-1);
  c.l2w.push_back(-1);
  c.from.push_back(n + 2);  // level 1: 2 w[n + 1]
  c.col.push_back(n + 1);
  c.val.insert(c.val.end(), {2, 0, 0, 0});
  c.ptr.push_back(c.col.size());
  c.from.push_back(n + 1);  // level 0
  for (uint32_t i = 1; i <= n; ++i) {
    c.col.push_back(i);
    c.val.insert(c.val.end(), m1, m1 + 4);
  }
  c.ptr.push_back(c.col.size());
  rs_output o = c.out();
  rs_witness v = c.wit();
  rs_witness *w = nullptr;
  rs_lift_report rep;
  if (wtns::lift_witness(&o, &v, &w, &rep) != RS_OK) return fail(std::string("long row: ") + rs_last_error());
  const uint64_t a = bn128 ? 5000 : 5000 % 257, b = bn128 ? 10000 : 10000 % 257;
  if (w->val[4 * (n + 1)] != a || w->val[4 * (n + 2)] != b || w->val[4 * (n + 1) + 3] || w->val[4 * (n + 2) + 1])
    return fail("long row: wrong value");
  if (rep.levels != 2 || rep.entries != n + 1 || rep.lifted != 2 || rep.free_labels != 0 || rep.shadowed != 0) return fail("long row: wrong report");
  wtns::witness_free(w);
  return 0;
}

static int empty_log() {
  Case c;
  c.l2w = {0, -1, 1};
  c.value(1);
  c.value(7);
  rs_output o = c.out();
  o.log_from = nullptr;
  o.log_to = rs_lc{};
  rs_witness v = c.wit();
  rs_witness *w = nullptr;
  rs_lift_report rep;
  if (wtns::lift_witness(&o, &v, &w, &rep) != RS_OK) return fail(std::string("empty log: ") + rs_last_error());
  if (w->val[0] != 1 || w->val[4] != 0 || w->val[8] != 7 || rep.free_labels != 1 || rep.levels != 0 || rep.lifted != 0) return fail("empty log: wrong result");
  wtns::witness_free(w);
  return 0;
}

static int refusals() {
  Case c;
  {  // null arguments
    c = small_case();
    rs_output o = c.out();
    rs_witness v = c.wit();
    rs_witness *w = nullptr;
    rs_lift_report rep;
    if (wtns::lift_witness(nullptr, &v, &w, &rep) != RS_E_INVALID || wtns::lift_witness(&o, nullptr, &w, &rep) != RS_E_INVALID ||
        wtns::lift_witness(&o, &v, nullptr, &rep) != RS_E_INVALID || wtns::lift_witness(&o, &v, &w, nullptr) != RS_E_INVALID)
      return fail("a null argument was accepted");
    if (!strstr(rs_last_error(), "null argument")) return fail("null argument: wrong message");
    o.log_from = nullptr;
    if (wtns::lift_witness(&o, &v, &w, &rep) != RS_E_INVALID) return fail("a null log_from was accepted");
    o = c.out();
    o.label_to_wire = nullptr;
    if (wtns::lift_witness(&o, &v, &w, &rep) != RS_E_INVALID) return fail("a null label_to_wire was accepted");
  }
  c = small_case();
  c.value(3);
  if (expect_refusal(c, "wires", "a witness one value long")) return 1;
  c = small_case();
  c.v.resize(8);
  if (expect_refusal(c, "wires", "a witness one value short")) return 1;
  c = small_case();
  c.v[0] = 2;
  if (expect_refusal(c, "w[0]", "w[0] = 2")) return 1;
  c = small_case();
  c.v[4] = 257;
  if (expect_refusal(c, "not below the prime", "a value = p")) return 1;
  c = small_case();
  c.v[5] = 1;  // a high limb beyond n8 = 8
  if (expect_refusal(c, "not below the prime", "a value above 2^64")) return 1;
  c = small_case();
  c.from[1] = 7;
  if (expect_refusal(c, "`from` is not below", "from = L")) return 1;
  c = small_case();
  c.from[1] = 0xffffffffu;
  if (expect_refusal(c, "`from` is not below", "from = 2^32 - 1")) return 1;
  c = small_case();
  c.from[0] = 0;
  if (expect_refusal(c, "`from` is the constant", "from = 0")) return 1;
  c = small_case();
  c.from[0] = 2;
  if (expect_refusal(c, "still has a wire", "a from with a wire")) return 1;
  c = small_case();
  c.col[2] = 7;
  if (expect_refusal(c, "a key is not below", "a key = L")) return 1;
  c = small_case();
  c.col[0] = 0xffffffffu;  // (of the shadowed entry: every entry's keys are checked)
  if (expect_refusal(c, "a key is not below", "a key = 2^32 - 1")) return 1;
  c = small_case();
  c.ptr[0] = 1;
  if (expect_refusal(c, "row pointers", "ptr[0] = 1")) return 1;
  c = small_case();
  c.ptr[2] = 1;
  c.ptr[1] = 2;  // [0, 2, 1, ...]
  if (expect_refusal(c, "row pointers", "decreasing pointers")) return 1;
  c = small_case();
  c.ptr[4] = 5;
  if (expect_refusal(c, "row pointers", "ptr[n] != nnz")) return 1;
  c = small_case();
  c.ptr[4] = 1ull << 40;
  if (expect_refusal(c, "row pointers", "ptr[n] far past nnz")) return 1;
  c = small_case();
  std::swap(c.from[2], c.from[3]);  // entry 2 now defines label 3 and reads it (key 3): its `to` holds its own `from`
  if (expect_refusal(c, "elimination order", "an entry that reads its own label")) return 1;
  c = Case();
  c.l2w = {0, 1, -1, -1};
  c.entry(2, {{0, 1}});
  c.entry(3, {{2, 1}});  // reads label 2, which the earlier entry 0 defines
  c.value(1);
  c.value(4);
  if (expect_refusal(c, "elimination order", "an entry that reads an earlier entry's label")) return 1;
  c = Case();
  c.l2w = {0, 1, -1, -1};
  c.entry(2, {{3, 1}});
  c.entry(3, {{2, 1}});  // a cycle
  c.value(1);
  c.value(4);
  if (expect_refusal(c, "elimination order", "a cycle")) return 1;
  c = small_case();
  c.l2w[1] = 3;  // a wire >= n_wires
  if (expect_refusal(c, "n_wires", "a wire past n_wires")) return 1;
  c = small_case();
  c.n8 = 12;
  if (expect_refusal(c, "field size", "n8 = 12")) return 1;
  return 0;
}

int main() {
  if (small() || long_row(false) || long_row(true) || empty_log() || refusals()) return 1;
  printf("ok\n");
  return 0;
}
