// json_write.hpp -- the --json and --simplification_substitution files on the device
// (rs_engine_write_constraints_json / rs_engine_write_substitution_json and their one-shots,
// include/rs_simplify.h): the bytes rs_write_constraints_json / rs_write_substitution_json (r1cs_io.cpp)
// write (constraint_list/src/json_porting.rs:16-48, constraint_writers/src/json_writer.rs:4-45, 94-131).
//
// One formatter serves both files.  Its input is n rows of 3 parts (A, B, C of a constraint) or of 1 part
// (the `to` map of a substitution), every part a CSR block (ptr, col, val) with ptr[0] = 0; its output is
// the image of the rows, the file without its opening and closing strings (the host writes those):
//   constraints  row r = `\n[` (r = 0) | `,\n[`, obj(A) `,` obj(B) `,` obj(C) `]`              12 fixed bytes
//   log          row r = `\n"` (r = 0) | `,\n"`, from[r] in decimal, `" : `, obj(to[r])          9 fixed bytes
//   obj          `{` entries joined by `,` `}`;  entry = `"key":"value"`, key = label_to_wire[col] (the
//                constraints) or col (the log), value = the four limbs in decimal
// An entry's text is 5 + digits(key) + digits(value) bytes, 1 more for the comma before it unless it is
// the first of its part.  With escan_q the exclusive scan of those lengths over part q's entries and xscan
// the exclusive scan of digits(from[r]) (the log only), row r starts at image byte
//   P(r) = fixed * r - (r > 0) + xscan[r] + sum over q of escan_q[ptr_q[r]]
// (row 0's opening is a byte shorter), part q of it at P(r) + its opening + the parts before (their
// entries + 3 bytes each), and entry e of it at that + 1 + escan_q[e] - escan_q[ptr_q[r]]: every byte's
// place is a closed form, there is no per-row table, and positions are 64-bit.
//   k_json_first  a lane per row: marks the first entry of every non-empty part (elen[ptr[r]] = 1)
//   k_json_len    a lane per entry: the mapped key and the entry's text length (the value is converted to
//                 count its digits exactly); a removed or out-of-range signal sets error bit 0, a key not
//                 above the one before it in the same part sets bit 1
//   k_json_from   a lane per log row: digits(from[r])
//   (rocprim exclusive scans; the totals and the error word read back: the verdict precedes the file)
//   k_json_emit   a workgroup per chunk of C image bytes (RS_JSON_CHUNK): the first and last row that
//                 overlap the chunk by binary search over P, then 256 (row, part) pairs at a time: a lane
//                 per pair writes the pair's punctuation and finds its entries that overlap the chunk
//                 (binary search over escan), the entries of the 256 pairs are dealt to the lanes
//                 (a workgroup scan of their counts), each converted (eight 32-bit limbs divided by 10^9
//                 nine times) and written, clipped to the chunk, into the chunk's LDS image, which goes to
//                 the image in aligned 16-byte pieces (the image's last partial piece byte by byte).
// An entry that straddles a chunk border is converted by both neighbours; every image byte has exactly
// one writer and nothing is atomic.  A row of 100 k entries is simply many chunks.
#pragma once
// (included by engine.hip inside namespace rs, after its scan helpers and stage_io.hpp)

constexpr uint64_t kJsonChunk = 16384, kJsonChunkMin = 64, kJsonChunkMax = 65536;  // a power of two
constexpr int kJsonErrRemoved = 1, kJsonErrOrder = 2;

// decimal digits of m (1 for 0)
__host__ __device__ __forceinline__ int json_dig32(uint32_t m) {
  int n = 1;
  if (m >= 100000000u) { n += 8; m /= 100000000u; }
  if (m >= 10000u) { n += 4; m /= 10000u; }
  if (m >= 100u) { n += 2; m /= 100u; }
  if (m >= 10u) ++n;
  return n;
}

// v (four limbs) = sum of d[k] * 10^(9 k), d[k] < 10^9; returns the index of the top non-zero d (0 for
// v = 0).  Pass k divides what is left, < 2^(256 - 29 k), by 10^9: only the limbs that can be non-zero.
__host__ __device__ __forceinline__ int json_dec(const uint64_t *v, uint32_t d[9]) {
  uint32_t x[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[2 * i] = (uint32_t)v[i];
    x[2 * i + 1] = (uint32_t)(v[i] >> 32);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    uint64_t rem = 0;
#pragma unroll
    for (int i = (256 - 29 * k + 31) / 32 - 1; i >= 0; --i) {
      const uint64_t cur = (rem << 32) | x[i];
      const uint32_t q = (uint32_t)(cur / 1000000000u);  // rem < 10^9: the quotient fits
      x[i] = q;
      rem = cur - (uint64_t)q * 1000000000u;
    }
    d[k] = (uint32_t)rem;
  }
  int top = 0;
#pragma unroll
  for (int k = 1; k < 9; ++k)
    if (d[k]) top = k;
  return top;
}

#ifdef __HIPCC__
struct JsonPart {
  const uint64_t *ptr;    // n + 1 row offsets, ptr[0] = 0
  const uint32_t *col;
  const uint64_t *val;    // 4 limbs an entry
  const uint64_t *escan;  // nnz + 1: the exclusive scan of the entries' text lengths
};
struct JsonGeom {
  uint64_t n;            // rows
  uint32_t nparts;       // 3: the constraints file, 1: the log
  uint32_t fixed;        // bytes a row besides its entries and from[r]: 12 / 9
  JsonPart p[3];
  const uint32_t *from;  // the log: log_from (else nullptr)
  const uint64_t *xscan; // the log: n + 1, the exclusive scan of digits(from[r])
  const int32_t *l2w;    // the constraints file: label_to_wire (else nullptr: the key is col)
  uint64_t n_labels;
  uint64_t total;        // image bytes
  uint32_t C;            // bytes a chunk: a power of two, 64 .. 65536
};

__global__ void k_json_first(const uint64_t *ptr, uint64_t n, uint64_t *elen) {
  for (uint64_t r = gtid(); r < n; r += gstride())
    if (ptr[r + 1] > ptr[r]) elen[ptr[r]] = 1;
}

__device__ __forceinline__ int64_t json_key(const uint32_t *col, uint64_t e, const int32_t *l2w, uint64_t n_labels) {
  const uint32_t k = col[e];
  if (!l2w) return (int64_t)k;
  return k < n_labels ? (int64_t)l2w[k] : -1;
}

// elen[e]: 1 on entry for the first entry of a part (k_json_first), 0 otherwise
__global__ void k_json_len(const uint32_t *col, const uint64_t *val, uint64_t nnz, const int32_t *l2w, uint64_t n_labels, uint64_t *elen,
                           int *err) {
  int bad = 0;
  for (uint64_t e = gtid(); e < nnz; e += gstride()) {
    const uint64_t first = elen[e];
    const int64_t m = json_key(col, e, l2w, n_labels);
    if (m < 0) bad |= kJsonErrRemoved;
    else if (!first && e && json_key(col, e - 1, l2w, n_labels) >= m) bad |= kJsonErrOrder;
    uint32_t d[9];
    const int top = json_dec(val + 4 * e, d);
    elen[e] = (uint64_t)(6 + json_dig32(m < 0 ? 0u : (uint32_t)m) + 9 * top + json_dig32(d[top])) - first;
  }
  if (bad) atomicOr(err, bad);
}

__global__ void k_json_from(const uint32_t *from, uint64_t n, uint64_t *xlen) {
  for (uint64_t r = gtid(); r < n; r += gstride()) xlen[r] = (uint64_t)json_dig32(from[r]);
}

// image byte where row r starts, r in [0, n]
__device__ __forceinline__ uint64_t json_row_pos(const JsonGeom &g, uint64_t r) {
  uint64_t p = (uint64_t)g.fixed * r - (r ? 1 : 0);
  if (g.xscan) p += g.xscan[r];
  for (uint32_t q = 0; q < g.nparts; ++q) p += g.p[q].escan[g.p[q].ptr[r]];
  return p;
}

// the chunk's LDS image: bytes [lo, hi) of the image
struct JsonBuf {
  uint8_t *b;
  uint64_t lo, hi;
  __device__ __forceinline__ void put(uint64_t p, uint8_t c) const {
    if (p >= lo && p < hi) b[p - lo] = c;
  }
  // the `w` low decimal digits of x at [p, p + w)
  __device__ __forceinline__ void digits(uint64_t p, int w, uint32_t x) const {
    for (int i = w - 1; i >= 0; --i) {
      put(p + (uint64_t)i, (uint8_t)('0' + x % 10));
      x /= 10;
    }
  }
};

// entry e of part P at image byte s: [`,`] `"key":"value"`
__device__ __forceinline__ void json_emit_entry(const JsonGeom &g, const JsonPart &P, uint64_t e, bool first, uint64_t s, const JsonBuf &B) {
  if (!first) B.put(s++, ',');
  const int64_t m = json_key(P.col, e, g.l2w, g.n_labels);
  const uint32_t key = m < 0 ? 0u : (uint32_t)m;  // (a refused image is never emitted)
  const int dk = json_dig32(key);
  B.put(s++, '"');
  B.digits(s, dk, key);
  s += (uint64_t)dk;
  B.put(s++, '"');
  B.put(s++, ':');
  B.put(s++, '"');
  uint32_t d[9];
  const int top = json_dec(P.val + 4 * e, d);
#pragma unroll
  for (int k = 8; k >= 0; --k)
    if (k <= top) {
      const int w = k == top ? json_dig32(d[k]) : 9;
      B.digits(s, w, d[k]);
      s += (uint64_t)w;
    }
  B.put(s, '"');
}

// LDS (dynamic, 16 B aligned): C bytes, then 256 x (u64 first entry of the pair, u64 first entry in the
// chunk, i64 image byte of the pair's entry 0 less escan there), then 3 x 256 ints (counts, the scan's two rows)
__global__ void __launch_bounds__(256) k_json_emit(JsonGeom g, uint64_t n_chunks, uint8_t *out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t json_lds[];
  uint8_t *buf = json_lds;
  uint64_t *s_pb = reinterpret_cast<uint64_t *>(json_lds + g.C);
  uint64_t *s_ea = s_pb + 256;
  int64_t *s_base = reinterpret_cast<int64_t *>(s_ea + 256);
  int *s_cnt = reinterpret_cast<int *>(s_base + 256);
  int *scan = s_cnt + 256;  // [2][256]
  const uint32_t l = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t lo = c * g.C, hi = lo + g.C < g.total ? lo + g.C : g.total;
    const JsonBuf B{buf, lo, hi};
    // r0: the last row that starts at or before lo; r1: the last row that starts before hi (a row is 9
    // bytes at least)
    uint64_t a = 0, b = g.n - 1;
    while (a < b) {
      const uint64_t m = a + (b - a + 1) / 2;
      if (json_row_pos(g, m) <= lo) a = m;
      else b = m - 1;
    }
    const uint64_t r0 = a;
    b = r0 + g.C / 9 + 1;
    if (b > g.n - 1) b = g.n - 1;
    while (a < b) {
      const uint64_t m = a + (b - a + 1) / 2;
      if (json_row_pos(g, m) < hi) a = m;
      else b = m - 1;
    }
    const uint32_t n_pairs = (uint32_t)(a - r0 + 1) * g.nparts;
    for (uint32_t t0 = 0; t0 < n_pairs; t0 += 256) {
      const uint32_t t = t0 + l;
      int cnt = 0;
      if (t < n_pairs) {
        const uint64_t r = r0 + t / g.nparts;
        const uint32_t q = t % g.nparts;
        uint64_t ps = json_row_pos(g, r);
        if (q == 0) {  // the row's opening
          uint64_t s = ps;
          if (r) B.put(s++, ',');
          B.put(s++, '\n');
          B.put(s++, g.from ? '"' : '[');
          if (g.from) {
            const uint32_t f = g.from[r];
            const int df = json_dig32(f);
            B.digits(s, df, f);
            s += (uint64_t)df;
            B.put(s++, '"');
            B.put(s++, ' ');
            B.put(s++, ':');
            B.put(s, ' ');
          }
        }
        ps += (r ? 3 : 2) + (g.from ? (uint64_t)json_dig32(g.from[r]) + 4 : 0);
        for (uint32_t x = 0; x < q; ++x) ps += 3 + g.p[x].escan[g.p[x].ptr[r + 1]] - g.p[x].escan[g.p[x].ptr[r]];
        const JsonPart &P = g.p[q];
        const uint64_t pb = P.ptr[r], pe = P.ptr[r + 1];
        const uint64_t end = ps + 1 + (P.escan[pe] - P.escan[pb]);  // the closing brace
        B.put(ps, '{');
        B.put(end, '}');
        if (q + 1 < g.nparts) B.put(end + 1, ',');
        else if (!g.from) B.put(end + 1, ']');
        // entry e lies at [base + escan[e], base + escan[e + 1])
        const int64_t base = (int64_t)(ps + 1) - (int64_t)P.escan[pb];
        uint64_t ea = pb, eb = pe;  // ea: the first entry that ends after lo
        for (uint64_t y = pe; ea < y;) {
          const uint64_t m = ea + (y - ea) / 2;
          if (base + (int64_t)P.escan[m + 1] > (int64_t)lo) y = m;
          else ea = m + 1;
        }
        for (uint64_t x = ea; x < eb;) {  // eb: the first entry at or after ea that starts at or after hi
          const uint64_t m = x + (eb - x) / 2;
          if (base + (int64_t)P.escan[m] >= (int64_t)hi) eb = m;
          else x = m + 1;
        }
        cnt = (int)(eb - ea);
        s_pb[l] = pb;
        s_ea[l] = ea;
        s_base[l] = base;
      }
      s_cnt[l] = cnt;
      // inclusive scan of the pairs' counts (Hillis-Steele, 8 rounds)
      int cur = 0;
      scan[l] = cnt;
      __syncthreads();
      for (uint32_t d = 1; d < 256; d <<= 1) {
        scan[(cur ^ 1) * 256 + l] = scan[cur * 256 + l] + (l >= d ? scan[cur * 256 + l - d] : 0);
        cur ^= 1;
        __syncthreads();
      }
      const int *inc = scan + cur * 256;
      const int total = inc[255];
      for (int j = (int)l; j < total; j += 256) {
        int x = 0, y = 255;  // the first pair whose inclusive count passes j
        while (x < y) {
          const int m = (x + y) / 2;
          if (inc[m] > j) y = m;
          else x = m + 1;
        }
        const uint64_t e = s_ea[x] + (uint64_t)(j - (inc[x] - s_cnt[x]));
        const JsonPart &P = g.p[(t0 + (uint32_t)x) % g.nparts];
        json_emit_entry(g, P, e, e == s_pb[x], (uint64_t)(s_base[x] + (int64_t)P.escan[e]), B);
      }
      __syncthreads();
    }
    // the chunk to the image, 16 B a lane; the image's last partial piece byte by byte
    const uint32_t units = (uint32_t)((hi - lo + 15) / 16);
    for (uint32_t u = l; u < units; u += 256) {
      const uint64_t p = lo + 16ull * u;
      if (p + 16 <= g.total) *reinterpret_cast<uint4 *>(out + p) = reinterpret_cast<const uint4 *>(buf)[u];
      else
        for (uint64_t i = p; i < g.total; ++i) out[i] = buf[i - lo];
    }
    __syncthreads();
  }
}

// What the formatter reads, on the device: n rows of nparts CSR parts (ptr[q][0] = 0, ptr[q][n] = nnz[q]).
struct JsonSrc {
  uint64_t n = 0;
  int nparts = 3;
  const uint64_t *ptr[3] = {};
  const uint32_t *col[3] = {};
  const uint64_t *val[3] = {};
  uint64_t nnz[3] = {0, 0, 0};
  const uint32_t *from = nullptr;  // the log
  const int32_t *l2w = nullptr;    // the constraints file
  uint64_t n_labels = 0;
};

static void json_scan(rs_engine *E, const uint64_t *in, uint64_t *out, uint64_t n) {
  excl_scan(E->SA, "json.scan", E->st, in, out, (uint64_t)0, n, rocprim::plus<uint64_t>());
}

// The rows of `s` (device, their producers on the main stream or done) as the file at `path`.  t0: when the
// call began; t_in: when the upload of `s` was done (t0 when there was none).  Buffers: the writers' arena.
static void write_json_device(rs_engine *E, const JsonSrc &s, const char *path, double t0, double t_in) {
  hipStream_t st = E->st;
  Arena &A = E->SA;
  uint64_t chunk = env_u64("RS_JSON_CHUNK", kJsonChunk, kJsonChunkMin, kJsonChunkMax);  // (read on every call)
  while (chunk & (chunk - 1)) chunk &= chunk - 1;  // a power of two (rounded down)
  const bool log = s.nparts == 1;
  const char *head = log ? "{" : "{\n\"constraints\": [", *tail = log ? "\n}" : "\n]\n}";
  JsonGeom g{};
  g.n = s.n;
  g.nparts = (uint32_t)s.nparts;
  g.fixed = log ? 9 : 12;
  g.from = s.from;
  g.l2w = s.l2w;
  g.n_labels = s.n_labels;
  g.C = (uint32_t)chunk;
  Events<6> evs(hipEventDefault);  // around pass 1, the scans, pass 2
  uint8_t *img = nullptr;
  if (s.n) {
    const char *nm[3] = {"json.a", "json.b", "json.c"};
    uint64_t *elen[3] = {}, *escan[3] = {};
    int *d_err = A.get<int>("json.err", 1);
    HC(hipMemsetAsync(d_err, 0, 4, st));
    HC(hipEventRecord(evs.e[0], st));
    for (int q = 0; q < s.nparts; ++q) {
      elen[q] = A.get<uint64_t>(std::string(nm[q]) + ".len", s.nnz[q] + 1);
      escan[q] = A.get<uint64_t>(std::string(nm[q]) + ".scan", s.nnz[q] + 1);
      HC(hipMemsetAsync(elen[q], 0, 8 * (s.nnz[q] + 1), st));
      launch(st, k_json_first, s.n, s.ptr[q], s.n, elen[q]);
      if (s.nnz[q]) launch(st, k_json_len, s.nnz[q], s.col[q], s.val[q], s.nnz[q], s.l2w, s.n_labels, elen[q], d_err);
    }
    uint64_t *xlen = nullptr, *xscan = nullptr;
    if (log) {
      xlen = A.get<uint64_t>("json.xlen", s.n + 1);
      xscan = A.get<uint64_t>("json.xscan", s.n + 1);
      launch(st, k_json_from, s.n, s.from, s.n, xlen);
      HC(hipMemsetAsync(xlen + s.n, 0, 8, st));
    }
    HC(hipEventRecord(evs.e[1], st));
    HC(hipEventRecord(evs.e[2], st));
    for (int q = 0; q < s.nparts; ++q) json_scan(E, elen[q], escan[q], s.nnz[q] + 1);
    if (log) json_scan(E, xlen, xscan, s.n + 1);
    HC(hipEventRecord(evs.e[3], st));
    // ---- the totals and the verdict
    uint64_t *h = (uint64_t *)pin_get(E, kPinRead, kPinRb);  // pinned read-back words [0..4]
    h[3] = 0;
    for (int q = 0; q < s.nparts; ++q) HC(hipMemcpyAsync(h + q, escan[q] + s.nnz[q], 8, hipMemcpyDeviceToHost, st));
    if (log) HC(hipMemcpyAsync(h + 3, xscan + s.n, 8, hipMemcpyDeviceToHost, st));
    HC(hipMemcpyAsync(h + 4, d_err, 4, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    const int err = *(const int *)(h + 4);
    if (err & kJsonErrRemoved) throw RsError(RS_E_INTERNAL, "constraint mentions a removed signal (apply_correspondence panics)");
    if (err & kJsonErrOrder) throw RsError(RS_E_INVALID, "a row part's keys are not strictly ascending (the device JSON writer does not sort)");
    g.total = (uint64_t)g.fixed * s.n - 1 + h[3];
    for (int q = 0; q < s.nparts; ++q) {
      g.total += h[q];
      g.p[q] = JsonPart{s.ptr[q], s.col[q], s.val[q], escan[q]};
    }
    g.xscan = xscan;
    img = A.get<uint8_t>("json.img", g.total);
    const uint64_t n_chunks = (g.total + g.C - 1) / g.C;
    const size_t lds = g.C + 256 * 24 + 3 * 256 * sizeof(int);
    if (lds > 48 * 1024) HC(hipFuncSetAttribute((const void *)k_json_emit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HC(hipEventRecord(evs.e[4], st));
    hipLaunchKernelGGL(k_json_emit, dim3((unsigned)std::min<uint64_t>(n_chunks, 65536)), dim3(256), lds, st, g, n_chunks, img);
    HC(hipGetLastError());
    HC(hipEventRecord(evs.e[5], st));
  }
  const double t_valid = now_ms();
  // ---- the file (its blocks up front, while k_json_emit runs), then the image
  float ms[3] = {0, 0, 0};
  write_image_file(E, path, {head, strlen(head)}, {tail, strlen(tail)}, img, g.total, st, [&] {
    HC(hipEventSynchronize(evs.e[5]));
    for (int k = 0; k < 3; ++k) HC(hipEventElapsedTime(&ms[k], evs.e[2 * k], evs.e[2 * k + 1]));
  });
  const double t_end = now_ms();
  rs_json_stats &js = E->jstats;
  js.write_ms = t_end - t0;
  js.in_ms = t_in - t0;
  js.kernel_ms = (t_valid - t_in) + ms[2];
  js.out_ms = js.write_ms - js.in_ms - js.kernel_ms;
  js.bytes = g.total;
  if (g_prof_env)
    fprintf(stderr, "[rs-prof] write_json (%s): %.1f MB out, chunk %u: in %.2f ms, pass 1 %.2f ms, scans %.2f ms, read-back + host %.2f ms, pass 2 %.2f ms, out %.2f ms\n",
            log ? "substitutions" : "constraints", g.total / 1e6, g.C, js.in_ms, ms[0], ms[1], (t_valid - t_in) - ms[0] - ms[1], ms[2], js.out_ms);
}

// A host CSR block for the one-shots: rows [0, n) of `L` in either layout (rs_rows_next) as (ptr, col, val)
// with ptr[0] = 0.  A CSR block that already is one is viewed, anything else compacted into `own`.
struct JsonHostPart {
  const uint64_t *ptr = nullptr;
  const uint32_t *col = nullptr;
  const uint64_t *val = nullptr;
  uint64_t nnz = 0;
  std::vector<uint64_t> optr, oval;
  std::vector<uint32_t> ocol;
};
static void json_host_part(const rs_output *o, int q, const rs_lc &L, uint64_t n, const uint32_t *len, JsonHostPart &hp) {
  if (!n) return;
  if (!len && !L.ptr) throw RsError(RS_E_INVALID, "rows without a ptr array");
  if (!len) {
    bool mono = true;
    for (uint64_t r = 0; r < n && mono; ++r) mono = L.ptr[r] <= L.ptr[r + 1];
    if (!mono || L.ptr[n] > L.nnz) throw RsError(RS_E_INVALID, "bad row pointers");
    if (L.ptr[n] && (!L.col || !L.val)) throw RsError(RS_E_INVALID, "entries without col/val");
    if (L.ptr[0] == 0) {
      hp.ptr = L.ptr;
      hp.col = L.col;
      hp.val = L.val;
      hp.nnz = L.ptr[n];
      return;
    }
  }
  if (L.nnz && (!L.col || !L.val)) throw RsError(RS_E_INVALID, "entries without col/val");
  rs_rows it;
  if (o) rs_rows_begin(o, q, &it);
  else it = rs_rows{&L, nullptr, nullptr, 0, 0};
  const uint64_t *jump = it.jump;
  const uint64_t njump = !o || !len ? 0 : (q == 0 ? o->a_njump : (q == 1 ? o->b_njump : o->c_njump));
  hp.optr.assign(n + 1, 0);
  for (uint64_t r = 0; r < n; ++r) {
    if (len && (len[r] & RS_ROW_JUMP) && (it.j >= njump || !jump)) throw RsError(RS_E_INVALID, "row layout: more jumping rows than jump offsets");
    uint64_t rb, rl;
    rs_rows_next(&it, r, &rb, &rl);
    if (rb > L.nnz || rl > L.nnz - rb) throw RsError(RS_E_INVALID, "row layout reaches past the block's entries");
    if (rl) {
      hp.ocol.insert(hp.ocol.end(), L.col + rb, L.col + rb + rl);
      hp.oval.insert(hp.oval.end(), L.val + 4 * rb, L.val + 4 * (rb + rl));
    }
    hp.optr[r + 1] = hp.optr[r] + rl;
  }
  hp.ptr = hp.optr.data();
  hp.col = hp.ocol.data();
  hp.val = hp.oval.data();
  hp.nnz = hp.optr[n];
}

// `hp` to the device (the writers' arena, names under `nm`) as part q of `s`
static void json_upload_part(rs_engine *E, const JsonHostPart &hp, uint64_t n, const std::string &nm, int q, JsonSrc &s) {
  uint64_t *ptr = E->SA.get<uint64_t>(nm + ".ptr", n + 1);
  uint32_t *col = E->SA.get<uint32_t>(nm + ".col", hp.nnz);
  uint64_t *val = E->SA.get<uint64_t>(nm + ".val", 4 * hp.nnz);
  if (n) {
    HC(hipMemcpyAsync(ptr, hp.ptr, 8 * (n + 1), hipMemcpyHostToDevice, E->st));
    if (hp.nnz) {
      HC(hipMemcpyAsync(col, hp.col, 4 * hp.nnz, hipMemcpyHostToDevice, E->st));
      HC(hipMemcpyAsync(val, hp.val, 32 * hp.nnz, hipMemcpyHostToDevice, E->st));
    }
  }
  s.ptr[q] = ptr;
  s.col[q] = col;
  s.val[q] = val;
  s.nnz[q] = hp.nnz;
}
#endif  // __HIPCC__
