// lift.hpp -- a wire witness lifted back to the --O0 labels on the device (rs_engine_lift_witness,
// rs_lift_witness_device, rs_engine_fetch_witness, rs_engine_write_wtns_resident; include/rs_simplify.h has
// the definition).  The host twin (wtns_io.hpp lift_witness) is the oracle: values and report agree to the
// bit.
//
// The resident wire witness is n_wires values in Montgomery form (SA "wit.w", witness.hpp); the lifted one
// is n_labels values in the same form, built beside it (SA "lift.w") and swapped in once the last error
// word reads clean.  The log goes up once, as the check stages it.  On one stream:
//   k_lift_owner   a lane per entry: validates `from`, atomicMax of i + 1 on owner[from] (64-bit integers;
//                  no atomics on field values anywhere, so the result is deterministic)
//   k_lift_seed    a lane per label: w[s] from the wire witness or zero; lifted and free labels counted per
//                  wave, one atomic each; the owner entries marked (an unmarked entry is shadowed)
//   k_lift_level   a lane per (key, value) pair of the log: consecutive lanes load consecutive keys; the
//                  pair's row by binary search in the row pointers; a candidate level[owner(key)] + 1 for an
//                  owned key of an owner row; a segmented max over the wave's runs of equal rows, and one
//                  integer atomicMax per run that raises its row's level -- a row may span any number of
//                  waves, workgroups or passes of the grid, so nothing depends on the grid.  Repeated until
//                  a pass raises nothing (one changed word read back per pass through pinned memory): at
//                  most levels + 1 passes.  The first pass also raises the error bits for a key >= the
//                  labels and for an owned key whose owner is not a later entry; the host reads that
//                  verdict before it goes on, which is what bounds the loop (the dependencies then point
//                  strictly forward).
//   one stable radix sort of the rows by level (shadowed rows keyed past every level, so the owner rows
//   come first, index order kept inside a level), k_lift_len (the sorted rows' lengths, the level
//   boundaries), one exclusive scan of the lengths: the virtual row pointers of all levels at once.  The
//   boundaries and their virtual pointers are read back once.
//   per level, ascending:
//   k_lift_dot     k_wit_dot's scheme (witness.hpp wit_dot_chunks) over the level's virtual rows: a
//                  workgroup per RS_WIT_CHUNK consecutive virtual entries, the lane's row by binary search in
//                  the chunk's slice of the virtual pointers (LDS, beside the rows' source positions); the
//                  lane reads source entry ptr[row] + (e - vptr[row]).  Nothing is copied or permuted: each
//                  pair is multiplied once.
//   k_lift_rows    a lane per row of the level: the partials in chunk order, into Montgomery form, w[from].
// A log of d levels costs 2 d launches here (kernel boundaries order the levels): a 100 k-level log is
// slow, not wrong.
#pragma once
// (included by engine.hip inside namespace rs, after witness.hpp)

constexpr int kLiftErrFromRange = 16, kLiftErrFromZero = 32, kLiftErrFromWire = 64, kLiftErrOrder = 128;  // beside kWitErr* in res[12]
// res words of a lift: [0] labels with an owner, [1] free labels, [2] the pass raised a level, [3] the deepest level

#ifdef __HIPCC__
__global__ void k_lift_owner(const uint32_t *from, uint64_t n, const int32_t *l2w, uint64_t n_labels, unsigned long long *owner,
                             unsigned long long *res) {
  int bad = 0;
  for (uint64_t i = gtid(); i < n; i += gstride()) {
    const uint32_t f = from[i];
    if (f >= n_labels) bad |= kLiftErrFromRange;
    else if (f == 0) bad |= kLiftErrFromZero;
    else if (l2w[f] >= 0) bad |= kLiftErrFromWire;
    else atomicMax(owner + f, (unsigned long long)(i + 1));
  }
  if (bad) atomicOr(res + 12, (unsigned long long)bad);
}

__global__ void k_lift_seed(const Fe *vm, uint64_t n_wires, const int32_t *l2w, const unsigned long long *owner, uint64_t n_labels, Fe *w,
                            uint8_t *own, unsigned long long *res) {
  unsigned long long n_own = 0, n_free = 0;
  int bad = 0;
  for (uint64_t s = gtid(); s < n_labels; s += gstride()) {
    const int32_t wire = l2w[s];
    Fe x = fe_zero();
    if (wire >= 0) {
      if ((uint64_t)wire < n_wires) x = vm[wire];
      else bad |= kWitErrWire;
    } else {
      const unsigned long long o = owner[s];
      if (o) {
        ++n_own;
        own[o - 1] = 1;
      } else {
        ++n_free;
      }
    }
    w[s] = x;
  }
  // all lanes arrive here: one pair of atomics per wave
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    n_own += __shfl_xor(n_own, d);
    n_free += __shfl_xor(n_free, d);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_own) atomicAdd(res + 0, n_own);
    if (n_free) atomicAdd(res + 1, n_free);
  }
  if (bad) atomicOr(res + 12, (unsigned long long)bad);
}

__global__ void __launch_bounds__(256) k_lift_level(const uint64_t *ptr, const uint32_t *key, uint64_t n, uint64_t nnz, uint64_t n_labels,
                                                    const unsigned long long *owner, const uint8_t *own, uint32_t *level, int first,
                                                    unsigned long long *res) {
  const uint32_t lane = threadIdx.x & 63;
  int bad = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * 256; base < nnz; base += (uint64_t)gridDim.x * 256) {  // (uniform over the workgroup)
    const uint64_t e = base + threadIdx.x;
    const bool active = e < nnz;
    unsigned long long row = ~0ull;
    uint32_t cand = 0;
    if (active) {
      uint64_t a = 0, b = n - 1;  // the last row whose pointer is not above e
      while (a < b) {
        const uint64_t m = a + (b - a + 1) / 2;
        if (ptr[m] <= e) a = m;
        else b = m - 1;
      }
      row = a;
      const uint32_t k = key[e];
      if (k >= n_labels) bad |= kWitErrKey;
      else if (own[row]) {
        const unsigned long long o = owner[k];
        if (o) {
          if (o - 1 <= row) bad |= kLiftErrOrder;  // (no candidate: a cycle raises nothing)
          else cand = level[o - 1] + 1;
        }
      }
    }
    // the max over each run of equal rows in the wave, at the run's last lane
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long orow = __shfl_up(row, d);
      const uint32_t oc = __shfl_up(cand, d);
      if (lane >= (uint32_t)d && orow == row && oc > cand) cand = oc;
    }
    const unsigned long long nrow = __shfl_down(row, 1);
    if (active && (lane == 63 || nrow != row) && cand > level[row]) {
      if (atomicMax(level + row, cand) < cand) {
        res[2] = 1;
        atomicMax(res + 3, (unsigned long long)cand);
      }
    }
  }
  if (bad && first) atomicOr(res + 12, (unsigned long long)bad);
}

// The sort's input: an owner row's level, a shadowed row past every level
__global__ void k_lift_keys(const uint8_t *own, const uint32_t *level, uint64_t n, uint32_t *skey, uint32_t *sval) {
  for (uint64_t i = gtid(); i < n; i += gstride()) {
    skey[i] = own[i] ? level[i] : 0xffffffffu;
    sval[i] = (uint32_t)i;
  }
}

// j in [0, n_own]: the sorted row's length (0 for the pad at n_own, whose scan is the total), and where
// each level begins: bound[l] for l in [0, levels], bound[levels] = n_own (every level holds a row)
__global__ void k_lift_len(const uint64_t *ptr, const uint32_t *skey, const uint32_t *idx, uint64_t n_own, uint64_t levels, uint64_t *len,
                           uint64_t *bound) {
  for (uint64_t j = gtid(); j <= n_own; j += gstride()) {
    if (j == n_own) {
      len[j] = 0;
      bound[levels] = n_own;
      continue;
    }
    const uint32_t r = idx[j], lv = skey[j];
    len[j] = ptr[r + 1] - ptr[r];
    if (lv < levels && (j == 0 || skey[j - 1] != lv)) bound[lv] = j;
  }
}

// hb[2 l] = bound[l], hb[2 l + 1] = vptr[bound[l]]: what the host reads back
__global__ void k_lift_bounds(const uint64_t *bound, const uint64_t *vptr, uint64_t levels, uint64_t n_own, uint64_t *hb) {
  for (uint64_t l = gtid(); l <= levels; l += gstride()) {
    const uint64_t b = bound[l];
    hb[2 * l] = b;
    hb[2 * l + 1] = b <= n_own ? vptr[b] : 0;
  }
}

// P.ptr / P.dot / V.idx: the level's rows (already offset to its first row); [V.e0, V.e1) its virtual entries
__global__ void __launch_bounds__(256) k_lift_dot(FieldP F, WitPart P, WitVirt V, uint64_t n_rows, const Fe *wm, uint64_t n_labels, uint32_t C,
                                                  uint64_t n_chunks, unsigned long long *res) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lift_lds[];
  wit_dot_chunks<true>(lift_lds, F, P, V, n_rows, wm, n_labels, C, n_chunks, res);
}

// (every `from` is below the labels: k_lift_owner's verdict was read before the first level)
__global__ void k_lift_rows(FieldP F, WitPart P, const uint32_t *idx, const uint32_t *from, uint64_t n_rows, uint64_t e0, uint32_t shift, Fe *w) {
  for (uint64_t j = gtid(); j < n_rows; j += gstride()) w[from[idx[j]]] = fto_mont(F, wit_row_dot(F, P, j, shift, e0));
}

// ---------------------------------------------------------------- the lift
struct LiftIn {
  uint64_t n_labels = 0, n_wires = 0;
  const int32_t *l2w = nullptr;  // device
  uint64_t n = 0, nnz = 0;       // the log: host arrays
  const uint32_t *from = nullptr, *key = nullptr;
  const uint64_t *ptr = nullptr, *val = nullptr;
};

static void lift_throw(const char *who, unsigned long long bits, bool pbad) {
  const std::string f = std::string(who) + ": ";
  if (pbad) throw RsError(RS_E_INVALID, f + "log_to block: bad row pointers (ptr[0] != 0, decreasing, or ptr[n_log] != nnz)");
  if (bits & kLiftErrFromRange) throw RsError(RS_E_INVALID, f + "a log entry's `from` is not below the number of labels");
  if (bits & kLiftErrFromZero) throw RsError(RS_E_INVALID, f + "a log entry's `from` is the constant (label 0)");
  if (bits & kLiftErrFromWire) throw RsError(RS_E_INVALID, f + "a log entry's `from` still has a wire");
  if (bits & kWitErrWire) throw RsError(RS_E_INVALID, f + "a wire is not below n_wires");
  if (bits & kWitErrKey) throw RsError(RS_E_INVALID, f + "a key is not below the number of labels");
  if (bits & kLiftErrOrder) throw RsError(RS_E_INVALID, f + "the log is not in elimination order: an entry reads a label that no later entry defines");
}

// who: the entry point the caller used, for the messages
static void lift_device(rs_engine *E, const LiftIn &in, rs_lift_report *rep, const char *who) {
  const std::string f = std::string(who) + ": ";
  const double t0 = now_ms();
  hipStream_t st = E->st;
  Arena &A = E->SA;
  if (!E->wit_on) throw RsError(RS_E_INVALID, f + "no witness is loaded");
  if (in.n_labels == 0 || in.n_labels > 0x7fffffffull) throw RsError(RS_E_INVALID, f + "the result needs 1 .. 2^31 - 1 labels");
  if (E->wit_n != in.n_wires)
    throw RsError(RS_E_INVALID, f + "the witness has " + std::to_string(E->wit_n) + " values, the result " +
                                    std::to_string(in.n_wires) + " wires");
  if (in.n > 0xfffffffeull) throw RsError(RS_E_INVALID, f + "more than 2^32 - 2 log entries");
  const uint64_t L = in.n_labels, n = in.n, nnz = n ? in.nnz : 0;
  uint64_t C = env_u64("RS_WIT_CHUNK", kWitChunk, kWitChunkMin, kWitChunkMax);  // (read on every call)
  while (C & (C - 1)) C &= C - 1;
  uint32_t shift = 0;
  while ((1ull << shift) < C) ++shift;
  memset(rep, 0, sizeof(*rep));
  // ---- the log goes up once
  WitSrc log;
  if (n) {
    StageIn up(E, (log_stage_bytes(n, nnz) + 4095) & ~4095ull);
    wit_stage_log(E, up, in.from, in.ptr, in.key, in.val, n, nnz, log);
    HC(hipStreamSynchronize(E->stc));
  }
  const double t_in = now_ms();
  const FieldP F = E->WF;
  const Fe *vm = A.get<Fe>("wit.w", 1);
  Fe *w = A.get<Fe>("lift.w", L);
  unsigned long long *owner = A.get<unsigned long long>("lift.owner", L);
  uint8_t *own = A.get<uint8_t>("lift.own", n);
  uint32_t *level = A.get<uint32_t>("lift.level", n);
  unsigned long long *res = A.get<unsigned long long>("wit.res", kWitRes);
  int *d_pbad = A.get<int>("wit.pbad", 1);
  unsigned long long *h = (unsigned long long *)pin_get(E, kPinRead, kPinRb);  // pinned read-back words [0..15]
  HC(hipMemsetAsync(res, 0, 8 * kWitRes, st));
  HC(hipMemsetAsync(d_pbad, 0, 4, st));
  HC(hipMemsetAsync(owner, 0, 8 * L, st));
  if (n) {
    HC(hipMemsetAsync(own, 0, n, st));
    HC(hipMemsetAsync(level, 0, 4 * n, st));
    launch(st, k_check_ptr, n + 1, log.ptr[0], n, nnz, d_pbad);
    launch(st, k_lift_owner, n, log.from, n, in.l2w, L, owner, res);
  }
  launch_capped(st, k_lift_seed, L, 4096, vm, in.n_wires, in.l2w, (const unsigned long long *)owner, L, w, own, res);
  // ---- the first verdict: the row pointers and `from`, before any kernel reads a row
  h[15] = 0;
  HC(hipMemcpyAsync(h, res, 8 * 15, hipMemcpyDeviceToHost, st));
  HC(hipMemcpyAsync(h + 15, d_pbad, 4, hipMemcpyDeviceToHost, st));
  HC(hipStreamSynchronize(st));
  lift_throw(who, h[12], h[15] != 0);
  const uint64_t n_own = h[0], n_free = h[1];
  // ---- the levels
  uint64_t levels = n_own ? 1 : 0;
  if (n_own && nnz) {
    const unsigned blocks = (unsigned)std::min<uint64_t>((nnz + 255) / 256, 16384);
    for (uint64_t pass = 0;; ++pass) {
      if (pass > n_own + 1) throw RsError(RS_E_INTERNAL, f + "the level passes do not end");
      HC(hipMemsetAsync(res + 2, 0, 8, st));
      hipLaunchKernelGGL(k_lift_level, dim3(blocks), dim3(256), 0, st, log.ptr[0], log.col[0], n, nnz, L, (const unsigned long long *)owner,
                         (const uint8_t *)own, level, pass == 0 ? 1 : 0, res);
      HC(hipGetLastError());
      HC(hipMemcpyAsync(h + 2, res + 2, 16, hipMemcpyDeviceToHost, st));
      if (pass == 0) HC(hipMemcpyAsync(h + 12, res + 12, 8, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
      if (pass == 0) lift_throw(who, h[12], false);
      if (!h[2]) break;
    }
    levels = h[3] + 1;
  }
  uint64_t entries = 0;
  if (n_own) {
    // ---- the owner rows by level, their virtual row pointers
    uint32_t *skey = A.get<uint32_t>("lift.skey", n), *sval = A.get<uint32_t>("lift.sval", n);
    uint32_t *skey2 = A.get<uint32_t>("lift.skey2", n), *idx = A.get<uint32_t>("lift.idx", n);
    uint64_t *len = A.get<uint64_t>("lift.len", n_own + 1), *vptr = A.get<uint64_t>("lift.vptr", n_own + 1);
    uint64_t *bound = A.get<uint64_t>("lift.bound", levels + 1), *hb = A.get<uint64_t>("lift.hb", 2 * (levels + 1));
    launch(st, k_lift_keys, n, (const uint8_t *)own, (const uint32_t *)level, n, skey, sval);
    {
      size_t tb = 0;
      HC(rocprim::radix_sort_pairs(nullptr, tb, skey, skey2, sval, idx, (size_t)n, 0, 32, st));
      void *tmp = A.get<uint8_t>("lift.sort.tmp", tb);
      HC(rocprim::radix_sort_pairs(tmp, tb, skey, skey2, sval, idx, (size_t)n, 0, 32, st));
    }
    HC(hipMemsetAsync(bound, 0xff, 8 * (levels + 1), st));
    launch(st, k_lift_len, n_own + 1, log.ptr[0], (const uint32_t *)skey2, (const uint32_t *)idx, n_own, levels, len, bound);
    excl_scan(A, "lift.scan.tmp", st, (const uint64_t *)len, vptr, (uint64_t)0, n_own + 1, rocprim::plus<uint64_t>());
    launch(st, k_lift_bounds, levels + 1, (const uint64_t *)bound, (const uint64_t *)vptr, levels, n_own, hb);
    std::vector<uint64_t> b(2 * (levels + 1));
    HC(hipStreamSynchronize(st));
    rd(E, b.data(), hb, 8 * b.size());
    uint64_t max_chunks = 0;
    for (uint64_t l = 0; l <= levels; ++l) {
      const bool ok = b[2 * l] <= n_own && (l == 0 ? b[0] == 0 && b[1] == 0 : b[2 * l] > b[2 * l - 2] && b[2 * l + 1] >= b[2 * l - 1]);
      if (!ok || (l == levels && b[2 * l] != n_own)) throw RsError(RS_E_INTERNAL, f + "the level boundaries disagree");
      if (l) max_chunks = std::max(max_chunks, (b[2 * l + 1] - b[2 * l - 1] + C - 1) / C);
    }
    entries = b[2 * levels + 1];
    if (entries > nnz) throw RsError(RS_E_INTERNAL, f + "more virtual entries than the log holds");
    // ---- per level: the dot products, then w[from]
    Fe *dot = A.get<Fe>("lift.dot", n_own), *head = A.get<Fe>("lift.head", max_chunks), *tail = A.get<Fe>("lift.tail", max_chunks);
    int lds_max = 0;
    HC(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, E->device));
    const int src_lds = kWitLdsFixed + 16 * ((size_t)C + 2) <= (size_t)lds_max ? 1 : 0;  // (else the source positions stay in global memory)
    const size_t lds = kWitLdsFixed + (src_lds ? 16 : 8) * ((size_t)C + 2);
    if (lds > 48 * 1024) HC(hipFuncSetAttribute((const void *)k_lift_dot, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (uint64_t l = 0; l < levels; ++l) {
      const uint64_t b0 = b[2 * l], b1 = b[2 * l + 2], e0 = b[2 * l + 1], e1 = b[2 * l + 3];
      const uint64_t n_chunks = (e1 - e0 + C - 1) / C;
      WitPart P{};
      P.ptr = vptr + b0;
      P.col = log.col[0];
      P.val = reinterpret_cast<const Fe *>(log.val[0]);
      P.nnz = nnz;
      P.dot = dot + b0;
      P.head = head;
      P.tail = tail;
      if (n_chunks) {
        const WitVirt V{idx + b0, log.ptr[0], e0, e1, src_lds};
        hipLaunchKernelGGL(k_lift_dot, dim3((unsigned)std::min<uint64_t>(n_chunks, 65536)), dim3(256), lds, st, F, P, V, b1 - b0, (const Fe *)w, L,
                           (uint32_t)C, n_chunks, res);
        HC(hipGetLastError());
      }
      launch(st, k_lift_rows, b1 - b0, F, P, (const uint32_t *)(idx + b0), log.from, b1 - b0, e0, shift, w);
    }
  }
  // ---- the resident witness is replaced only after the last error word reads clean
  HC(hipMemcpyAsync(h + 12, res + 12, 8, hipMemcpyDeviceToHost, st));
  HC(hipStreamSynchronize(st));
  lift_throw(who, h[12], false);
  std::swap(A.bufs["wit.w"], A.bufs["lift.w"]);
  E->wit_n = L;
  const double t_end = now_ms();
  rep->n_labels = L;
  rep->n_wires = in.n_wires;
  rep->lifted = n_own;
  rep->free_labels = n_free;
  rep->shadowed = n - n_own;
  rep->levels = levels;
  rep->entries = entries;
  rep->in_ms = t_in - t0;
  rep->kernel_ms = t_end - t_in;
  rep->total_ms = t_end - t0;
  if (g_prof_env)
    fprintf(stderr, "[rs-prof] lift_witness (chunk %llu): %llu levels, in %.2f ms, kernels + read-backs %.2f ms\n", (unsigned long long)C,
            (unsigned long long)levels, rep->in_ms, rep->kernel_ms);
}

// The engine's own result and log
static void lift_engine(rs_engine *E, rs_lift_report *rep) {
  if (!E->have_result) throw RsError(RS_E_INVALID, "rs_engine_lift_witness: no result");
  if (!E->wit_on) throw RsError(RS_E_INVALID, "rs_engine_lift_witness: no witness is loaded");
  if (!E->log_on) throw RsError(RS_E_INVALID, "rs_engine_lift_witness: the last run kept no substitution log");
  if (!wit_same_prime(E->prime, E->wit_prime)) throw RsError(RS_E_INVALID, "rs_engine_lift_witness: the witness's prime is not the run's");
  LiftIn in;
  in.n_labels = E->S;
  in.n_wires = E->n_wires;
  in.l2w = E->A.get<int32_t>("fin.l2w", 1);
  in.n = E->log_from.size();
  if (in.n) {
    log_arrays_agree(E);
    in.nnz = E->log_key.size();
    in.from = E->log_from.data();
    in.ptr = E->log_ptr.data();
    in.key = E->log_key.data();
    in.val = E->log_val.data();
  }
  lift_device(E, in, rep, "rs_engine_lift_witness");
}

// ---------------------------------------------------------------- the resident witness, out
static void fetch_witness_device(rs_engine *E, rs_witness **out) {
  if (!E->wit_on) throw RsError(RS_E_INVALID, "rs_engine_fetch_witness: no witness is loaded");
  const uint64_t n = E->wit_n;
  uint64_t *canon = E->SA.get<uint64_t>("wit.canon", 4 * n);
  unsigned long long *res = E->SA.get<unsigned long long>("wit.res", kWitRes);
  // (the image of a 32-byte witness without a map: value i, canonical, as four limbs; without a map the
  // place is s < n, so the kernel can raise no bit in res and none is read)
  launch(E->st, k_wit_project, n, E->WF, (const Fe *)E->SA.get<Fe>("wit.w", 1), (const int32_t *)nullptr, n, n, 32u, (uint8_t *)canon, res);
  HC(hipStreamSynchronize(E->st));
  rs_witness *w = (rs_witness *)calloc(1, sizeof(rs_witness));
  if (!w) throw std::bad_alloc();
  w->prime_id = E->wit_prime_id;
  memcpy(w->prime, E->wit_prime, 32);
  w->n8 = E->wit_n8;
  w->n = n;
  w->val = (uint64_t *)calloc(n ? n : 1, 32);
  if (!w->val) {
    free(w);
    throw std::bad_alloc();
  }
  try {
    rd(E, w->val, canon, 32 * n);
  } catch (...) {
    wtns::witness_free(w);
    throw;
  }
  *out = w;
}

static void write_wtns_resident_device(rs_engine *E, const char *path) {
  hipStream_t st = E->st;
  Arena &A = E->SA;
  if (!E->wit_on) throw RsError(RS_E_INVALID, "rs_engine_write_wtns_resident: no witness is loaded");
  const uint32_t n8 = E->wit_n8;
  const uint64_t n = E->wit_n, total = n * n8;
  if (n >> 32) throw RsError(RS_E_INVALID, "rs_engine_write_wtns_resident: more than 2^32 - 1 values");
  const Fe *wm = A.get<Fe>("wit.w", 1);
  unsigned long long *res = A.get<unsigned long long>("wit.res", kWitRes);
  uint8_t *img = A.get<uint8_t>("wit.img", total);
  launch(st, k_wit_project, n, E->WF, wm, (const int32_t *)nullptr, n, n, n8, img, res);  // (every byte of the image is written; no bit of res can be raised without a map)
  const std::vector<uint8_t> head = wtns::head_bytes(n8, E->wit_prime, n);
  write_image_file(E, path, {head.data(), head.size()}, {}, img, total, st);
}
#endif  // __HIPCC__
