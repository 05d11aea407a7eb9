// Stand-alone host build of circom_cvm_amd/csrc/wtns_io.hpp (the .wtns reader / writer and the host
// evaluation of a witness), driven by tests/test_wtns_abi.py under the address and undefined-behaviour
// sanitizers (built together with csrc/host_common.cpp: the error text and the prime table).
//   wtns_host_check <scratch file> <good.wtns> [<malformed.wtns> ...]
// First the file helpers it reads through (Fd, pread_all, pwrite_all of csrc/host_common.hpp) on the scratch
// file, a short read and a short write among them.  Then
// the good file is read, written back (the same bytes) and then cut at every byte length: each cut must
// be refused with RS_E_INVALID, and so must every malformed file.  Last, a three-row system over F_257 is
// evaluated on a witness that satisfies it and on one that does not.  Prints `ok` and exits 0, or says
// what went wrong and exits 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <csignal>
#include <sys/resource.h>

#include "wtns_io.hpp"

using namespace rs;

static bool slurp(const char *path, std::vector<uint8_t> &b) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t g;
  while ((g = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + g);
  fclose(f);
  return true;
}
static bool spill(const char *path, const uint8_t *p, size_t n) {
  FILE *f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = n == 0 || fwrite(p, 1, n, f) == n;
  return fclose(f) == 0 && ok;
}
static int fail(const std::string &what) {
  fprintf(stderr, "wtns_host_check: %s\n", what.c_str());
  return 1;
}

static int small_evaluation() {
  // F_257, labels 0..3, w = (1, 3, 5, 15): 3 * 5 = 15;  w3 - 15 = 0;  2 w1 + w2 - 11 = 0
  const uint64_t P = 257;
  uint64_t wv[16] = {1, 0, 0, 0, 3, 0, 0, 0, 5, 0, 0, 0, 15, 0, 0, 0};
  rs_witness w{};
  w.prime_id = RS_PRIME_CUSTOM;
  w.prime[0] = P;
  w.n8 = 8;
  w.n = 4;
  w.val = wv;
  uint64_t p1[2] = {0, 1};
  uint32_t ca[1] = {1}, cb[1] = {2}, cc[1] = {3};
  uint64_t one[4] = {1, 0, 0, 0};
  uint64_t pce[2] = {0, 2};
  uint32_t kce[2] = {0, 3};
  uint64_t vce[8] = {P - 15, 0, 0, 0, 1, 0, 0, 0};
  uint64_t pl[2] = {0, 3};
  uint32_t kl[3] = {0, 1, 2};
  uint64_t vl[12] = {P - 11, 0, 0, 0, 2, 0, 0, 0, 1, 0, 0, 0};
  rs_input in{};
  in.prime_id = RS_PRIME_CUSTOM;
  in.prime[0] = P;
  in.max_signal = 4;
  in.cons_eq = rs_lc{1, 2, pce, kce, vce};
  in.linear = rs_lc{1, 3, pl, kl, vl};
  in.nl_a = rs_lc{1, 1, p1, ca, one};
  in.nl_b = rs_lc{1, 1, p1, cb, one};
  in.nl_c = rs_lc{1, 1, p1, cc, one};
  rs_witness_report rep;
  if (wtns::check_witness(&in, nullptr, &w, RS_WIT_INPUT, &rep) != RS_OK) return fail(std::string("small system: ") + rs_last_error());
  for (int c = 0; c < RS_WITC_COUNT; ++c)
    if (rep.failed[c] || rep.first_failed[c] != UINT64_MAX) return fail("small system: a row fails on its own witness");
  if (rep.checked[RS_WITC_CONS_EQ] != 1 || rep.checked[RS_WITC_EQ] != 0 || rep.checked[RS_WITC_LINEAR] != 1 || rep.checked[RS_WITC_NONLINEAR] != 1)
    return fail("small system: wrong row counts");
  wv[12] = 16;  // w3: the product row and the constant equality fail, the linear row holds
  if (wtns::check_witness(&in, nullptr, &w, RS_WIT_INPUT, &rep) != RS_OK) return fail(std::string("small system: ") + rs_last_error());
  if (rep.failed[RS_WITC_CONS_EQ] != 1 || rep.failed[RS_WITC_NONLINEAR] != 1 || rep.failed[RS_WITC_LINEAR] != 0 ||
      rep.first_failed[RS_WITC_NONLINEAR] != 0)
    return fail("small system: wrong failing set");
  wv[0] = 2;
  if (wtns::check_witness(&in, nullptr, &w, RS_WIT_INPUT, &rep) != RS_E_INVALID) return fail("small system: w[0] = 2 was accepted");
  return 0;
}

// Fd, pread_all and pwrite_all (host_common.hpp; the device path's staging code uses them too): a read that
// the file ends before is refused whole, and a write that the file-size limit cuts short -- pwrite returns
// fewer bytes than asked, then fails -- is reported, with the bytes that fit on disk.
static int short_read_and_write(const char *scratch) {
  const uint8_t src[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  uint8_t buf[16] = {};
  {
    Fd f;
    f.fd = open(scratch, O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (f.fd < 0) return fail("cannot open the scratch file");
    if (!pwrite_all(f.fd, src, 10, 0) || !pwrite_all(f.fd, src, 0, 99)) return fail("pwrite_all: a plain write failed");
    if (!pread_all(f.fd, buf, 10, 0) || memcmp(buf, src, 10) != 0) return fail("pread_all: the bytes written do not come back");
    if (!pread_all(f.fd, buf, 4, 6) || memcmp(buf, src + 6, 4) != 0) return fail("pread_all: wrong bytes at an offset");
    if (pread_all(f.fd, buf, 11, 0) || pread_all(f.fd, buf, 1, 10)) return fail("pread_all: a read past the end of the file succeeded");
    if (!pread_all(f.fd, buf, 0, 10)) return fail("pread_all: an empty read failed");
    struct rlimit old, cut;
    if (getrlimit(RLIMIT_FSIZE, &old) != 0) return fail("getrlimit");
    cut = old;
    cut.rlim_cur = 12;
    signal(SIGXFSZ, SIG_IGN);
    if (setrlimit(RLIMIT_FSIZE, &cut) != 0) return fail("setrlimit");
    const bool wrote = pwrite_all(f.fd, src, 16, 4);  // 8 bytes fit below the limit
    setrlimit(RLIMIT_FSIZE, &old);
    signal(SIGXFSZ, SIG_DFL);
    if (wrote) return fail("pwrite_all: a write cut short by the file-size limit was reported whole");
    if (!pread_all(f.fd, buf, 12, 0) || memcmp(buf, src, 4) != 0 || memcmp(buf + 4, src, 8) != 0 || pread_all(f.fd, buf, 1, 12))
      return fail("pwrite_all: the short write did not leave the bytes that fit");
    const int fd = f.release();
    if (f.fd != -1 || close(fd) != 0) return fail("Fd::release");
  }
  Fd none;  // (closes nothing)
  if (pread_all(none.fd, buf, 1, 0) || pwrite_all(none.fd, src, 1, 0)) return fail("a closed descriptor was read or written");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) return fail("usage: wtns_host_check scratch good.wtns [malformed.wtns ...]");
  const char *scratch = argv[1];
  if (short_read_and_write(scratch)) return 1;
  std::vector<uint8_t> good;
  if (!slurp(argv[2], good)) return fail("cannot read the good file");
  rs_witness *w = nullptr;
  if (wtns::read_wtns(argv[2], &w) != RS_OK) return fail(std::string("the good file was refused: ") + rs_last_error());
  if (wtns::write_wtns(scratch, w, nullptr) != RS_OK) return fail(std::string("write: ") + rs_last_error());
  std::vector<uint8_t> back;
  if (!slurp(scratch, back) || back != good) return fail("the good file does not round-trip");
  wtns::witness_free(w);
  for (size_t n = 0; n < good.size(); ++n) {
    if (!spill(scratch, good.data(), n)) return fail("cannot write the scratch file");
    w = nullptr;
    const int rc = wtns::read_wtns(scratch, &w);
    if (rc != RS_E_INVALID || w) return fail("a file cut at " + std::to_string(n) + " bytes was not refused");
    if (!*rs_last_error()) return fail("a refusal without a message");
  }
  for (int i = 3; i < argc; ++i) {
    w = nullptr;
    const int rc = wtns::read_wtns(argv[i], &w);
    if (rc != RS_E_INVALID || w) return fail(std::string(argv[i]) + " was not refused");
  }
  if (small_evaluation()) return 1;
  printf("ok %zu cuts %d malformed\n", good.size(), argc - 3);
  return 0;
}
