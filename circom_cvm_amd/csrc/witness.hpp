// witness.hpp -- a witness on the device (rs_engine_load_witness / rs_engine_load_wtns,
// rs_engine_check_witness, rs_engine_write_wtns; include/rs_simplify.h): the evaluation of
// A.w o B.w - C.w over the input rows, the result's rows and the substitution log, and the projection of
// the witness onto the result's wires.  The host twins (wtns_io.hpp) are the oracles.
//
// The resident witness is n values in Montgomery form (SA "wit.w"); a coefficient is canonical, so one
// fmul(coefficient, witness value) is the canonical product, and every sum below is canonical.
//
// One evaluator serves every source.  Its input is n rows of 3 parts (A, B, C of a constraint) or of 1
// part (the C part of a linear class; the `to` map of a substitution, with its `from` column), every part
// a CSR block (ptr, col, val) with ptr[0] = 0 and ptr[n] = nnz.
//   k_wit_dot    entry-parallel: a workgroup per chunk of C consecutive entries of one part (RS_WIT_CHUNK).
//                256 entries a pass: consecutive lanes load consecutive col / val, gather w[col], multiply,
//                and find their row by binary search in the chunk's slice of ptr (in LDS when it fits:
//                a slice may hold any number of empty rows).  The products are summed per row by a
//                segmented scan over the pass (rows are runs of equal row numbers, so `same row d lanes
//                back` is the segment test; the scan stops at the first distance at which no lane adds);
//                a row that runs on into the next pass hands its sum on as the pass's carry, as the
//                run-sum scan of frames_wave.hpp does between blocks.  A row wholly inside the chunk
//                stores its dot product (dot[row]); a row that crosses a border leaves one partial per
//                chunk: head[chunk] when it began before the chunk, tail[chunk] when it began inside and
//                runs past the end.  Every partial has one writer; no atomics on field values.
//   k_wit_rows   a lane per row: each part's dot product -- 0 for an empty row, dot[row] for a row inside
//                one chunk, else tail[first chunk] + head[chunks between, in order] + head[last chunk]
//                (a 100 k-entry row is ~100 additions at the default chunk) -- then the verdict:
//                fmul(a, b) against c, c against 0, or w[from] against the dot.  Failures are counted and
//                the smallest failing row found per lane, reduced over the wave, one atomicAdd and one
//                atomicMin per wave that saw a failure.
// k_wit_dot's body is the template wit_dot_chunks: the lift (lift.hpp, k_lift_dot) runs it over a level's
// virtual rows, whose entries lie elsewhere in the log (WitVirt); the check's instance reads entry e at e.
// A key >= n_labels sets an error bit instead of being gathered.  Positions are 64-bit.  Empty parts launch
// nothing.  The result does not depend on the grid or on the chunk.
#pragma once
// (included by engine.hip inside namespace rs, after stage_io.hpp: StageIn, write_image_file)

constexpr uint64_t kWitChunk = 1024, kWitChunkMin = 64, kWitChunkMax = 8192;  // a power of two (LDS: 8 B an entry)
constexpr int kWitErrRange = 1, kWitErrOne = 2, kWitErrKey = 4, kWitErrWire = 8;
constexpr int kWitRes = 16;  // result words: [2 c] failures of class c, [2 c + 1] its smallest failing row, [12] error bits

#ifdef __HIPCC__
// A lane per value i in [i0, i0 + cnt): n8 bytes at raw + n8 * i widened to four limbs, refused when
// >= p (and value 0 when != 1), stored in Montgomery form.
__global__ void k_wit_prepare(const uint8_t *raw, uint32_t n8, uint64_t i0, uint64_t cnt, FieldP F, Fe *wm, unsigned long long *res) {
  int bad = 0;
  for (uint64_t j = gtid(); j < cnt; j += gstride()) {
    const uint64_t i = i0 + j;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(raw + (uint64_t)n8 * i);
    Fe v = fe_zero();
    for (uint32_t k = 0; k < n8 / 8; ++k) v.l[k] = src[k];
    if (geq4(v.l, F.p)) {
      bad |= kWitErrRange;
      v = fe_zero();
    }
    if (i == 0 && (v.l[0] != 1 || v.l[1] || v.l[2] || v.l[3])) bad |= kWitErrOne;
    wm[i] = fto_mont(F, v);
  }
  if (bad) atomicOr(res + 12, (unsigned long long)bad);
}

struct WitPart {
  const uint64_t *ptr;  // n + 1
  const uint32_t *col;
  const Fe *val;        // canonical
  uint64_t nnz;
  Fe *dot;              // n: rows inside one chunk
  Fe *head, *tail;      // a chunk each: the partial of the row that began before the chunk / runs past it
};

// LDS (dynamic, 16 B aligned): 2 x 256 Fe (the scan's two rows), 256 u64 (the lanes' rows), the carry
// (Fe + its row), then C + 2 row pointers
constexpr size_t kWitLdsFixed = 2 * 256 * sizeof(Fe) + 256 * 8 + sizeof(Fe) + 16;
// The rows the lift evaluates (lift.hpp) are a virtual CSR: P.ptr holds the virtual pointers of a level's
// rows, the entries [e0, e1) are theirs, and row r's entries lie at sptr[idx[r]] + (e - P.ptr[r]) of
// col / val.  The check's rows are their own source: entry e of [0, nnz) is entry e.
struct WitVirt {
  const uint32_t *idx;   // virtual row -> source row
  const uint64_t *sptr;  // the source's row pointers
  uint64_t e0, e1;
  int src_lds;           // the rows' source positions fit in LDS beside the pointer slice
};
// The body of k_wit_dot and k_lift_dot (kVirt).  lds: kWitLdsFixed + 8 (C + 2) bytes, with kVirt 8 (C + 2)
// more (the rows' source positions beside their virtual pointers).
template <bool kVirt>
__device__ __forceinline__ void wit_dot_chunks(uint8_t *wit_lds, const FieldP &F, const WitPart &P, const WitVirt &V, uint64_t n_rows,
                                               const Fe *wm, uint64_t n_labels, uint32_t C, uint64_t n_chunks, unsigned long long *res) {
  Fe *s_v = reinterpret_cast<Fe *>(wit_lds);
  uint64_t *s_row = reinterpret_cast<uint64_t *>(s_v + 512);
  Fe *s_carry = reinterpret_cast<Fe *>(s_row + 256);
  uint64_t *s_carry_row = reinterpret_cast<uint64_t *>(s_carry + 1);
  uint64_t *s_ptr = s_carry_row + 2;
  uint64_t *s_src = s_ptr + C + 2;  // (kVirt)
  const uint32_t t = threadIdx.x;
  const uint64_t e0 = kVirt ? V.e0 : 0, e1 = kVirt ? V.e1 : P.nnz;
  int bad = 0;
  for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t lo = e0 + c * C, hi = lo + C < e1 ? lo + C : e1;
    // r0 / r1: the rows that hold entries lo / hi - 1 (the last row whose pointer is not above the entry)
    uint64_t a = 0, b = n_rows - 1;
    while (a < b) {
      const uint64_t m = a + (b - a + 1) / 2;
      if (P.ptr[m] <= lo) a = m;
      else b = m - 1;
    }
    const uint64_t r0 = a;
    b = n_rows - 1;
    while (a < b) {
      const uint64_t m = a + (b - a + 1) / 2;
      if (P.ptr[m] <= hi - 1) a = m;
      else b = m - 1;
    }
    const uint64_t nr = a - r0 + 1;  // rows of the slice; S[0 .. nr] their pointers
    const uint64_t *S = P.ptr + r0;
    const bool in_lds = nr + 1 <= (uint64_t)C + 2;
    if (in_lds) {
      for (uint64_t i = t; i <= nr; i += 256) s_ptr[i] = P.ptr[r0 + i];
      if (kVirt && V.src_lds)
        for (uint64_t i = t; i < nr; i += 256) s_src[i] = V.sptr[V.idx[r0 + i]];
      S = s_ptr;
    }
    if (t == 0) *s_carry_row = UINT64_MAX;
    __syncthreads();
    for (uint64_t base = lo; base < hi; base += 256) {
      const uint64_t e = base + t;
      const bool active = e < hi;
      uint64_t row = UINT64_MAX, i = 0;
      Fe x = fe_zero();
      if (active) {
        uint64_t u = 0, v = nr - 1;  // the last i with S[i] <= e
        while (u < v) {
          const uint64_t m = u + (v - u + 1) / 2;
          if (S[m] <= e) u = m;
          else v = m - 1;
        }
        i = u;
        row = r0 + i;
        // (kVirt: lanes on one row still read consecutive col / val)
        const uint64_t se = kVirt ? (in_lds && V.src_lds ? s_src[i] : V.sptr[V.idx[row]]) + (e - S[i]) : e;
        const uint32_t k = P.col[se];
        if (k < n_labels) x = fmul(F, P.val[se], wm[k]);
        else bad |= kWitErrKey;
      }
      s_row[t] = row;
      int cur = 0;
      for (uint32_t d = 1; d < 256; d <<= 1) {  // the segmented inclusive scan
        s_v[cur * 256 + t] = x;
        __syncthreads();
        const bool add = active && t >= d && s_row[t - d] == row;
        if (add) x = fadd(F, x, s_v[cur * 256 + t - d]);
        cur ^= 1;
        if (!__syncthreads_or(add)) break;
      }
      const bool seg_end = active && (t == 255 || s_row[t + 1] != row);
      const uint64_t crow = *s_carry_row;
      Fe cval = fe_zero();
      if (seg_end && crow == row) cval = *s_carry;
      __syncthreads();  // the carry is read before the pass replaces it
      if (seg_end) {
        if (crow == row) x = fadd(F, x, cval);
        const bool before = S[i] < lo, ends = e + 1 == S[i + 1];
        if (ends || e + 1 == hi) {
          if (before) P.head[c] = x;
          else if (ends) P.dot[row] = x;
          else P.tail[c] = x;
        } else {  // the row runs on into the next pass
          *s_carry = x;
          *s_carry_row = row;
        }
      }
      __syncthreads();
    }
  }
  if (bad) atomicOr(res + 12, (unsigned long long)bad);
}

__global__ void __launch_bounds__(256) k_wit_dot(FieldP F, WitPart P, uint64_t n_rows, const Fe *wm, uint64_t n_labels, uint32_t C,
                                                 uint64_t n_chunks, unsigned long long *res) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wit_lds[];
  wit_dot_chunks<false>(wit_lds, F, P, WitVirt{}, n_rows, wm, n_labels, C, n_chunks, res);
}

struct WitRows {
  uint64_t n;
  int nparts;            // 3: (A.w)(B.w) = C.w; 1: C.w = 0, or with `from`: w[from] = C.w
  WitPart p[3];
  const uint32_t *from;  // the log
  int cls;               // the report's class
  uint32_t shift;        // log2 of the chunk
};

// (e0: where the part's chunks begin: 0 for the check, the level's first virtual entry for the lift)
__device__ __forceinline__ Fe wit_row_dot(const FieldP &F, const WitPart &P, uint64_t r, uint32_t shift, uint64_t e0 = 0) {
  const uint64_t b = P.ptr[r], e = P.ptr[r + 1];
  if (b == e) return fe_zero();
  const uint64_t c0 = (b - e0) >> shift, c1 = (e - 1 - e0) >> shift;
  if (c0 == c1) return P.dot[r];
  Fe s = P.tail[c0];
  for (uint64_t c = c0 + 1; c < c1; ++c) s = fadd(F, s, P.head[c]);
  return fadd(F, s, P.head[c1]);
}

__global__ void k_wit_rows(FieldP F, WitRows R, const Fe *wm, uint64_t n_labels, unsigned long long *res) {
  unsigned long long nfail = 0, first = ~0ull;
  int bad = 0;
  for (uint64_t r = gtid(); r < R.n; r += gstride()) {
    bool ok;
    if (R.nparts == 3) {
      const Fe a = wit_row_dot(F, R.p[0], r, R.shift), b = wit_row_dot(F, R.p[1], r, R.shift), c = wit_row_dot(F, R.p[2], r, R.shift);
      ok = fe_eq(fmul(F, fto_mont(F, a), b), c);
    } else {
      const Fe c = wit_row_dot(F, R.p[0], r, R.shift);
      if (!R.from) ok = fe_is_zero(c);
      else {
        const uint32_t k = R.from[r];
        if (k < n_labels) ok = fe_eq(ffrom_mont(F, wm[k]), c);
        else {
          bad |= kWitErrKey;
          ok = true;
        }
      }
    }
    if (!ok) {
      ++nfail;
      if (r < first) first = r;
    }
  }
  // all lanes arrive here: one pair of atomics per wave that saw a failure
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    nfail += __shfl_xor(nfail, d);
    const unsigned long long o = __shfl_xor(first, d);
    first = o < first ? o : first;
  }
  if ((threadIdx.x & 63) == 0 && nfail) {
    atomicAdd(res + 2 * R.cls, nfail);
    atomicMin(res + 2 * R.cls + 1, first);
  }
  if (bad) atomicOr(res + 12, (unsigned long long)bad);
}

// A lane per label with a wire: its value, canonical and narrowed to n8 bytes, at image byte n8 * l2w[s].
// l2w is the order-preserving rank of the kept labels: every byte has one writer.  l2w == nullptr: the
// witness as it is (value s at n8 * s).
__global__ void k_wit_project(FieldP F, const Fe *wm, const int32_t *l2w, uint64_t n_labels, uint64_t n_wires, uint32_t n8, uint8_t *img,
                              unsigned long long *res) {
  int bad = 0;
  for (uint64_t s = gtid(); s < n_labels; s += gstride()) {
    const int64_t wire = l2w ? (int64_t)l2w[s] : (int64_t)s;
    if (wire < 0) continue;
    if ((uint64_t)wire >= n_wires) {
      bad |= kWitErrWire;
      continue;
    }
    const Fe v = ffrom_mont(F, wm[s]);
    uint64_t *dst = reinterpret_cast<uint64_t *>(img + (uint64_t)n8 * (uint64_t)wire);
    for (uint32_t k = 0; k < n8 / 8; ++k) dst[k] = v.l[k];
  }
  if (bad) atomicOr(res + 12, (unsigned long long)bad);
}

// ---------------------------------------------------------------- the resident witness
// n values of n8 bytes to the device through the pinned staging pool on the copy stream, k_wit_prepare
// behind each buffer's copy; fill(dst, i0, cnt) puts values [i0, i0 + cnt) into a pinned buffer (false: a
// read error).  n8: the width of what `fill` delivers; n8_file: the width the witness's file has (what
// rs_engine_write_wtns writes).  The verdict is read back once, before anything else runs.
template <class Fill>
static void wit_upload(rs_engine *E, uint64_t n, uint32_t n8, uint32_t n8_file, const uint64_t prime[4], uint32_t prime_id, Fill &&fill) {
  E->wit_on = false;
  Arena &A = E->SA;
  hipStream_t stc = E->stc;
  const FieldP F = make_field(prime);
  Fe *wm = A.get<Fe>("wit.w", n);
  uint8_t *raw = A.get<uint8_t>("wit.raw", n * n8);
  unsigned long long *res = A.get<unsigned long long>("wit.res", kWitRes);
  unsigned long long *h = (unsigned long long *)pin_get(E, kPinRead, kPinRb);
  StageIn up(E, n * n8, n8);  // (a buffer: whole values)
  HC(hipMemsetAsync(res, 0, 8 * kWitRes, stc));
  up.send(raw, n * n8, "cannot read the witness's values",
          [&](uint8_t *buf, uint64_t off, uint64_t len) { return fill(buf, off / n8, len / n8); },
          [&](const uint8_t *, uint64_t off, uint64_t len) {
            launch(stc, k_wit_prepare, len / n8, (const uint8_t *)raw, n8, off / n8, len / n8, F, wm, res);
          });
  HC(hipMemcpyAsync(h, res + 12, 8, hipMemcpyDeviceToHost, stc));
  HC(hipStreamSynchronize(stc));
  if (h[0] & kWitErrRange) throw RsError(RS_E_INVALID, "witness: a value is not below the prime");
  if (h[0] & kWitErrOne) throw RsError(RS_E_INVALID, "witness: w[0] is not 1 (key 0 is the constant)");
  E->WF = F;
  memcpy(E->wit_prime, prime, 32);
  E->wit_prime_id = prime_id;
  E->wit_n = n;
  E->wit_n8 = n8_file;
  E->wit_on = true;
}

// ---------------------------------------------------------------- the evaluation
// What the evaluator reads, on the device
struct WitSrc {
  uint64_t n = 0;
  int nparts = 1;
  const uint64_t *ptr[3] = {};
  const uint32_t *col[3] = {};
  const uint64_t *val[3] = {};
  uint64_t nnz[3] = {0, 0, 0};
  const uint32_t *from = nullptr;
  int cls = 0;
};

// One rs_lc of the caller (host arrays) into the writers' arena under `nm`, through the staging pool
static void wit_stage_block(rs_engine *E, const rs_lc &L, const char *what, const std::string &nm, StageIn &up, WitSrc &s, int q) {
  const uint64_t n = L.n_rows, nnz = L.nnz;
  if (!L.ptr || (nnz && (!L.col || !L.val))) throw RsError(RS_E_INVALID, std::string(what) + " block: rows without ptr / col / val");
  uint64_t *ptr = E->SA.get<uint64_t>(nm + ".ptr", n + 1);
  uint32_t *col = E->SA.get<uint32_t>(nm + ".col", nnz);
  uint64_t *val = E->SA.get<uint64_t>(nm + ".val", 4 * nnz);
  up.send(ptr, L.ptr, 8 * (n + 1));
  up.send(col, L.col, 4 * nnz);
  up.send(val, L.val, 32 * nnz);
  s.ptr[q] = ptr;
  s.col[q] = col;
  s.val[q] = val;
  s.nnz[q] = nnz;
}

// The substitution log (host arrays) into the writers' arena, through the staging pool: the check's and
// the lift's source.  log_stage_bytes: what it sends, for the pool's size.
static uint64_t log_stage_bytes(uint64_t n_log, uint64_t log_nnz) { return n_log ? 4 * n_log + 8 * (n_log + 1) + 36 * log_nnz : 0; }
static void wit_stage_log(rs_engine *E, StageIn &up, const uint32_t *h_from, const uint64_t *h_ptr, const uint32_t *h_key,
                          const uint64_t *h_val, uint64_t n_log, uint64_t log_nnz, WitSrc &s) {
  Arena &A = E->SA;
  uint32_t *from = A.get<uint32_t>("wit.log.from", n_log), *key = A.get<uint32_t>("wit.log.key", log_nnz);
  uint64_t *ptr = A.get<uint64_t>("wit.log.ptr", n_log + 1), *val = A.get<uint64_t>("wit.log.val", 4 * log_nnz);
  up.send(from, h_from, 4 * n_log);
  up.send(ptr, h_ptr, 8 * (n_log + 1));
  up.send(key, h_key, 4 * log_nnz);
  up.send(val, h_val, 32 * log_nnz);
  s.n = n_log;
  s.nparts = 1;
  s.cls = RS_WITC_LOG;
  s.from = from;
  s.ptr[0] = ptr;
  s.col[0] = key;
  s.val[0] = val;
  s.nnz[0] = log_nnz;
}
// The engine's own log: its vectors agree
static void log_arrays_agree(rs_engine *E) {
  const uint64_t n_log = E->log_from.size(), log_nnz = E->log_key.size();
  if (E->log_ptr.size() != n_log + 1 || E->log_ptr[n_log] != log_nnz || E->log_val.size() != 4 * log_nnz)
    throw RsError(RS_E_INTERNAL, "the substitution log's arrays disagree");
}

// The rows of `s` against the resident witness: their failures into res[2 cls], res[2 cls + 1]
static void wit_eval(rs_engine *E, const WitSrc &s, uint32_t C, unsigned long long *res) {
  if (!s.n) return;
  hipStream_t st = E->st;
  Arena &A = E->SA;
  const Fe *wm = A.get<Fe>("wit.w", 1);
  const char *nm[3] = {"wit.p0", "wit.p1", "wit.p2"};
  uint32_t shift = 0;
  while ((1u << shift) < C) ++shift;
  WitRows R{};
  R.n = s.n;
  R.nparts = s.nparts;
  R.from = s.from;
  R.cls = s.cls;
  R.shift = shift;
  const size_t lds = kWitLdsFixed + 8 * ((size_t)C + 2);
  if (lds > 48 * 1024) HC(hipFuncSetAttribute((const void *)k_wit_dot, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int q = 0; q < s.nparts; ++q) {
    const uint64_t n_chunks = (s.nnz[q] + C - 1) / C;
    WitPart P{};
    P.ptr = s.ptr[q];
    P.col = s.col[q];
    P.val = reinterpret_cast<const Fe *>(s.val[q]);
    P.nnz = s.nnz[q];
    P.dot = A.get<Fe>(std::string(nm[q]) + ".dot", s.n);
    P.head = A.get<Fe>(std::string(nm[q]) + ".head", n_chunks);
    P.tail = A.get<Fe>(std::string(nm[q]) + ".tail", n_chunks);
    R.p[q] = P;
    if (n_chunks) {
      hipLaunchKernelGGL(k_wit_dot, dim3((unsigned)std::min<uint64_t>(n_chunks, 65536)), dim3(256), lds, st, E->WF, P, s.n, wm, E->wit_n, C,
                         n_chunks, res);
      HC(hipGetLastError());
    }
  }
  launch_capped(st, k_wit_rows, s.n, 4096, E->WF, R, wm, E->wit_n, res);
}

static bool wit_same_prime(const uint64_t a[4], const uint64_t b[4]) { return memcmp(a, b, 32) == 0; }

static void check_witness_device(rs_engine *E, const rs_input *in, uint32_t what, rs_witness_report *rep) {
  const double t0 = now_ms();
  hipStream_t st = E->st;
  Arena &A = E->SA;
  if (what & ~(RS_WIT_INPUT | RS_WIT_OUTPUT | RS_WIT_LOG)) throw RsError(RS_E_INVALID, "rs_engine_check_witness: unknown bits in `what`");
  if (!E->wit_on) throw RsError(RS_E_INVALID, "rs_engine_check_witness: no witness is loaded");
  if ((what & RS_WIT_INPUT) && !in) throw RsError(RS_E_INVALID, "rs_engine_check_witness: RS_WIT_INPUT without an input");
  if ((what & (RS_WIT_OUTPUT | RS_WIT_LOG)) && !E->have_result) throw RsError(RS_E_INVALID, "rs_engine_check_witness: no result");
  if ((what & RS_WIT_LOG) && !E->log_on) throw RsError(RS_E_INVALID, "rs_engine_check_witness: the last run kept no substitution log");
  if (what & RS_WIT_INPUT) {
    uint64_t p[4];
    if (!prime_of(in, p)) throw RsError(RS_E_INVALID, "unknown prime");
    if (!wit_same_prime(p, E->wit_prime)) throw RsError(RS_E_INVALID, "rs_engine_check_witness: the witness's prime is not the input's");
    if (E->wit_n != in->max_signal)
      throw RsError(RS_E_INVALID, "rs_engine_check_witness: the witness has " + std::to_string(E->wit_n) + " values, the input " +
                                      std::to_string(in->max_signal) + " labels");
    if (in->nl_a.n_rows != in->nl_b.n_rows || in->nl_a.n_rows != in->nl_c.n_rows) throw RsError(RS_E_INVALID, "non-linear blocks differ in row count");
  }
  if (what & (RS_WIT_OUTPUT | RS_WIT_LOG)) {
    if (!wit_same_prime(E->prime, E->wit_prime)) throw RsError(RS_E_INVALID, "rs_engine_check_witness: the witness's prime is not the run's");
    if (E->wit_n != E->S)
      throw RsError(RS_E_INVALID, "rs_engine_check_witness: the witness has " + std::to_string(E->wit_n) + " values, the result " +
                                      std::to_string(E->S) + " labels");
  }
  uint64_t C = env_u64("RS_WIT_CHUNK", kWitChunk, kWitChunkMin, kWitChunkMax);  // (read on every call)
  while (C & (C - 1)) C &= C - 1;  // a power of two (rounded down)
  if (what & RS_WIT_OUTPUT) ensure_csr(E);  // (before the evaluator's own buffers: they live in another arena and move nothing of the result)
  memset(rep, 0, sizeof(*rep));
  for (uint64_t &x : rep->first_failed) x = UINT64_MAX;
  unsigned long long *res = A.get<unsigned long long>("wit.res", kWitRes);
  unsigned long long *h = (unsigned long long *)pin_get(E, kPinRead, kPinRb);  // pinned read-back words [0..15]
  int *d_pbad = A.get<int>("wit.pbad", 1);
  for (int c = 0; c < RS_WITC_COUNT; ++c) {
    h[2 * c] = 0;
    h[2 * c + 1] = ~0ull;
  }
  for (int i = 12; i < kWitRes; ++i) h[i] = 0;
  HC(hipMemcpyAsync(res, h, 8 * kWitRes, hipMemcpyHostToDevice, st));
  HC(hipMemsetAsync(d_pbad, 0, 4, st));
  HC(hipStreamSynchronize(st));  // (h is read back into below)
  // ---- the uploads: the caller's input, the log
  WitSrc src[6];
  int n_src = 0;
  {
    const rs_lc *lin[3] = {nullptr, nullptr, nullptr};
    uint64_t all = 0;
    if (what & RS_WIT_INPUT) {
      lin[0] = &in->cons_eq;
      lin[1] = &in->eq;
      lin[2] = &in->linear;
      for (const rs_lc *L : {&in->cons_eq, &in->eq, &in->linear, &in->nl_a, &in->nl_b, &in->nl_c}) all += 8 * (L->n_rows + 1) + 36 * L->nnz;
    }
    const uint64_t n_log = (what & RS_WIT_LOG) ? E->log_from.size() : 0, log_nnz = n_log ? E->log_key.size() : 0;
    if (n_log) {
      log_arrays_agree(E);
      all += log_stage_bytes(n_log, log_nnz);
    }
    if (all) {
      StageIn up(E, (all + 4095) & ~4095ull);
      if (what & RS_WIT_INPUT) {
        const char *nm[3] = {"cons_eq", "eq", "linear"};
        for (int q = 0; q < 3; ++q) {
          if (!lin[q]->n_rows) continue;
          WitSrc &s = src[n_src++];
          s.n = lin[q]->n_rows;
          s.nparts = 1;
          s.cls = q;
          wit_stage_block(E, *lin[q], nm[q], std::string("wit.in.") + nm[q], up, s, 0);
        }
        if (in->nl_a.n_rows) {
          WitSrc &s = src[n_src++];
          s.n = in->nl_a.n_rows;
          s.nparts = 3;
          s.cls = RS_WITC_NONLINEAR;
          wit_stage_block(E, in->nl_a, "nl_a", "wit.in.nl_a", up, s, 0);
          wit_stage_block(E, in->nl_b, "nl_b", "wit.in.nl_b", up, s, 1);
          wit_stage_block(E, in->nl_c, "nl_c", "wit.in.nl_c", up, s, 2);
        }
        rep->checked[RS_WITC_CONS_EQ] = in->cons_eq.n_rows;
        rep->checked[RS_WITC_EQ] = in->eq.n_rows;
        rep->checked[RS_WITC_LINEAR] = in->linear.n_rows;
        rep->checked[RS_WITC_NONLINEAR] = in->nl_a.n_rows;
      }
      if (n_log)  // (src[5]: evaluated last, after the output)
        wit_stage_log(E, up, E->log_from.data(), E->log_ptr.data(), E->log_key.data(), E->log_val.data(), n_log, log_nnz, src[5]);
      HC(hipStreamSynchronize(E->stc));
    }
    rep->checked[RS_WITC_LOG] = n_log;
  }
  const double t_in = now_ms();
  // ---- the caller's row pointers are not trusted: their verdict precedes every kernel that reads a row
  if (n_src) {
    for (int i = 0; i < n_src; ++i)
      for (int q = 0; q < src[i].nparts; ++q) launch(st, k_check_ptr, src[i].n + 1, src[i].ptr[q], src[i].n, src[i].nnz[q], d_pbad);
    HC(hipMemcpyAsync(h + 13, d_pbad, 4, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    if (h[13]) throw RsError(RS_E_INVALID, "rs_engine_check_witness: bad row pointers in the input (ptr[0] != 0, decreasing, or ptr[n_rows] != nnz)");
  }
  for (int i = 0; i < n_src; ++i) wit_eval(E, src[i], (uint32_t)C, res);
  if (what & RS_WIT_OUTPUT) {
    const char *nm[3] = {"out.a", "out.b", "out.c"};
    WitSrc s;
    s.n = E->out_n_dev;
    s.nparts = 3;
    s.cls = RS_WITC_OUTPUT;
    for (int q = 0; q < 3; ++q) {
      s.ptr[q] = E->A.get<uint64_t>(std::string(nm[q]) + ".ptr", 1);
      s.col[q] = E->A.get<uint32_t>(std::string(nm[q]) + ".col", 1);
      s.val[q] = E->A.get<uint64_t>(std::string(nm[q]) + ".val", 1);
      s.nnz[q] = E->out_nnz[q];
    }
    rep->checked[RS_WITC_OUTPUT] = s.n;
    wit_eval(E, s, (uint32_t)C, res);
  }
  if (rep->checked[RS_WITC_LOG]) wit_eval(E, src[5], (uint32_t)C, res);
  HC(hipMemcpyAsync(h, res, 8 * kWitRes, hipMemcpyDeviceToHost, st));
  HC(hipStreamSynchronize(st));
  if (h[12] & kWitErrKey) throw RsError(RS_E_INVALID, "rs_engine_check_witness: a key is not below the number of labels");
  for (int c = 0; c < RS_WITC_COUNT; ++c) {
    rep->failed[c] = h[2 * c];
    rep->first_failed[c] = h[2 * c + 1];
  }
  const double t_end = now_ms();
  rep->in_ms = t_in - t0;
  rep->kernel_ms = t_end - t_in;
  rep->total_ms = t_end - t0;
  if (g_prof_env)
    fprintf(stderr, "[rs-prof] check_witness (what %u, chunk %llu): in %.2f ms, kernels + read-back %.2f ms\n", what, (unsigned long long)C,
            rep->in_ms, rep->kernel_ms);
}

// ---------------------------------------------------------------- the projection
static void write_wtns_device(rs_engine *E, const char *path) {
  hipStream_t st = E->st;
  Arena &A = E->SA;
  if (!E->have_result) throw RsError(RS_E_INVALID, "no result");
  if (!E->wit_on) throw RsError(RS_E_INVALID, "rs_engine_write_wtns: no witness is loaded");
  if (!wit_same_prime(E->prime, E->wit_prime)) throw RsError(RS_E_INVALID, "rs_engine_write_wtns: the witness's prime is not the run's");
  if (E->wit_n != E->S)
    throw RsError(RS_E_INVALID, "rs_engine_write_wtns: the witness has " + std::to_string(E->wit_n) + " values, the result " + std::to_string(E->S) +
                                    " labels");
  const uint32_t n8 = E->wit_n8;
  const uint64_t nw = E->n_wires, total = nw * n8;
  const int32_t *l2w = E->A.get<int32_t>("fin.l2w", 1);
  const Fe *wm = A.get<Fe>("wit.w", 1);
  unsigned long long *res = A.get<unsigned long long>("wit.res", kWitRes);
  unsigned long long *h = (unsigned long long *)pin_get(E, kPinRead, kPinRb);
  uint8_t *img = A.get<uint8_t>("wit.img", total);
  HC(hipMemsetAsync(res, 0, 8 * kWitRes, st));
  if (total) HC(hipMemsetAsync(img, 0, total, st));
  launch(st, k_wit_project, E->S, E->WF, wm, l2w, E->S, nw, n8, img, res);
  HC(hipMemcpyAsync(h, res + 12, 8, hipMemcpyDeviceToHost, st));
  HC(hipStreamSynchronize(st));
  if (h[0] & kWitErrWire) throw RsError(RS_E_INTERNAL, "rs_engine_write_wtns: a wire is not below n_wires");
  const std::vector<uint8_t> head = wtns::head_bytes(n8, E->wit_prime, nw);
  write_image_file(E, path, {head.data(), head.size()}, {}, img, total, st);
}
#endif  // __HIPCC__
