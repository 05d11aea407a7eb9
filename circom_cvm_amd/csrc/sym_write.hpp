// sym_write.hpp -- SURVEY A21 on the device: an --O0 .sym with its witness column rewritten
// (rs_engine_write_sym / rs_write_sym_device, include/rs_simplify.h), the bytes rs_write_sym
// (r1cs_io.cpp) writes: every line `L,W,rest` becomes `L,label_to_wire[L],rest`
// (constraint_list/src/sym_porting.rs:5-37, constraint_writers/src/sym_writer.rs:10-13).
//
// The rewrite is position-local, so there is no line table.  For byte i of the N input bytes:
//   line start    i == 0 or in[i - 1] == '\n'.  A line start holding '\n' is an empty line: the byte is
//                 dropped, delta(i) = -1.
//   second comma  a comma at i such that walking back from i - 1 passes 1-10 digits, an optional '-' and
//                 a comma c1, and walking back from c1 - 1 passes 1-10 digits (no leading zero unless the
//                 field is "0") and meets a line start.  At most 23 bytes before i are looked at.  There
//                 delta(i) = len(decimal(label_to_wire[L])) - (i - c1 - 1); the old W bytes (c1, i) are
//                 dropped and the new text goes to [out(i) - len, out(i)).
//   every kept byte goes to out(i) = i + sum of delta(j), j <= i; the output is N + sum of delta bytes,
//   one more when the last line has no '\n'.
// A name made of digits and commas cannot fake a second comma: the walk must end at a line start, so c1
// is the line's first comma and i its second.  The file is in the accepted grammar (rs_simplify.h) iff
// the non-empty line starts are as many as the second commas (every line has at most one) and no byte is
// NUL; that is known before anything is written.
//   k_sym_count   a workgroup per chunk of C bytes (RS_SYM_CHUNK): the chunk and the 32 bytes before it in
//                 LDS (16 B a lane), delta / line starts / second commas / NULs summed over the
//                 workgroup: the chunk's delta to cdelta[chunk], the four totals to tot[0..3].  Launched
//                 per staging buffer as it lands, on the copy stream
//   (rocprim exclusive scan of cdelta)
//   k_sym_emit    a workgroup per chunk: delta again, an inclusive scan over the chunk (a lane owns
//                 C / 256 consecutive bytes, at least 16), then the kept bytes and the new decimal texts
// A line's new W text may lie partly in the output range of the neighbouring chunk: every output byte has
// exactly one writer (the kept input byte it comes from, or the second comma whose text it belongs to)
// and every store is one byte wide, so no store touches a byte another chunk owns.
#pragma once
// (included by engine.hip inside namespace rs, after its scan helpers)

constexpr uint64_t kSymChunk = 4096, kSymChunkMin = 64, kSymChunkMax = 32768;  // a power of two
constexpr int kSymHalo = 32;  // bytes before a chunk kept in LDS (23 are looked at; 16 B units)

__host__ __device__ __forceinline__ bool sym_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// bytes of the decimal text of w ('-' included)
__host__ __device__ __forceinline__ int sym_declen(int32_t w) {
  uint32_t m = w < 0 ? 0u - (uint32_t)w : (uint32_t)w;
  int n = w < 0 ? 2 : 1;
  while (m >= 10) {
    m /= 10;
    ++n;
  }
  return n;
}

// `at(j)`: input byte j, for j >= 0 within 32 bytes before the position asked about
template <class At>
__host__ __device__ __forceinline__ bool sym_line_start(const At &at, int64_t i) {
  return i == 0 || at(i - 1) == '\n';
}

// the label field that ends before the comma at c1: 1-10 digits from a line start, no leading zero
// unless it is "0".  Reads back to c1 - 11.
template <class At>
__host__ __device__ __forceinline__ bool sym_label(const At &at, int64_t c1, uint64_t *L) {
  int64_t j = c1 - 1;
  int k = 0;
  while (k < 10 && j >= 0 && sym_digit(at(j))) {
    ++k;
    --j;
  }
  if (k == 0 || !(j < 0 || at(j) == '\n')) return false;  // (an 11th digit is no line start either)
  if (k > 1 && at(j + 1) == '0') return false;
  uint64_t v = 0;
  for (int64_t x = j + 1; x < c1; ++x) v = v * 10 + (uint64_t)(at(x) - '0');
  *L = v;
  return true;
}

// the comma at i is its line's second: *c1 the first comma, *L the label.  Reads back to i - 23.
template <class At>
__host__ __device__ __forceinline__ bool sym_second_comma(const At &at, int64_t i, int64_t *c1, uint64_t *L) {
  int64_t j = i - 1;
  int k = 0;
  while (k < 10 && j >= 0 && sym_digit(at(j))) {
    ++k;
    --j;
  }
  if (k == 0) return false;
  if (j >= 0 && at(j) == '-') --j;
  if (j < 0 || at(j) != ',') return false;
  *c1 = j;
  return sym_label(at, j, L);
}

// byte j (a digit or '-') of a VALID file lies in its line's W field: only digits and '-' between it and
// a comma that follows a label from a line start (the line's first comma; the field it opens is W).
// Reads back to j - 22.
template <class At>
__host__ __device__ __forceinline__ bool sym_in_w(const At &at, int64_t j) {
  int64_t t = j;
  int k = 0;
  while (k < 11 && t >= 0 && (sym_digit(at(t)) || at(t) == '-')) {
    ++k;
    --t;
  }
  if (t < 0 || at(t) != ',') return false;
  uint64_t L;
  return sym_label(at, t, &L);
}

__host__ __device__ __forceinline__ int32_t sym_wire(const int32_t *l2w, uint64_t n_labels, uint64_t L) {
  return L < n_labels ? l2w[L] : -1;
}

// what byte i adds to the counts: delta, a non-empty line start, a second comma, a NUL
struct SymCnt {
  int delta, starts, commas, nuls;
};
template <class At>
__host__ __device__ __forceinline__ void sym_count_byte(const At &at, int64_t i, const int32_t *l2w, uint64_t n_labels, SymCnt &s) {
  const uint8_t c = at(i);
  if (c == 0) ++s.nuls;
  if (sym_line_start(at, i)) {
    if (c == '\n') --s.delta;
    else ++s.starts;
  }
  if (c == ',') {
    int64_t c1;
    uint64_t L;
    if (sym_second_comma(at, i, &c1, &L)) {
      ++s.commas;
      s.delta += sym_declen(sym_wire(l2w, n_labels, L)) - (int)(i - c1 - 1);
    }
  }
}

// Byte i of a valid file into the output image; *pre: the sum of delta before i on entry, through i on
// return.  Stores are one byte wide and bounded by out_size.
template <class At>
__host__ __device__ __forceinline__ void sym_emit_byte(const At &at, int64_t i, uint64_t N, const int32_t *l2w, uint64_t n_labels,
                                                       int64_t *pre, uint8_t *out, uint64_t out_size) {
  const uint8_t c = at(i);
  bool keep = true;
  if (c == '\n') {
    if (sym_line_start(at, i)) {
      --*pre;
      keep = false;
    }
  } else if (c == ',') {
    int64_t c1;
    uint64_t L;
    if (sym_second_comma(at, i, &c1, &L)) {
      const int32_t w = sym_wire(l2w, n_labels, L);
      const int len = sym_declen(w);
      *pre += len - (int)(i - c1 - 1);
      uint32_t m = w < 0 ? 0u - (uint32_t)w : (uint32_t)w;
      uint64_t p = (uint64_t)(i + *pre);  // the comma's place; the text ends before it
      for (int d = (w < 0 ? len - 1 : len); d > 0; --d) {
        --p;
        if (p < out_size) out[p] = (uint8_t)('0' + m % 10);
        m /= 10;
      }
      if (w < 0 && --p < out_size) out[p] = '-';
    }
  } else if (sym_digit(c) || c == '-') {
    keep = !sym_in_w(at, i);
  }
  const uint64_t p = (uint64_t)(i + *pre);
  if (keep && p < out_size) out[p] = c;
  if ((uint64_t)i == N - 1 && c != '\n' && out_size) out[out_size - 1] = '\n';  // a last line without '\n' gets one
}

#ifdef __HIPCC__
// the chunk's window in LDS: w[0] is input byte `lo`
struct SymWin {
  const uint8_t *w;
  int64_t lo;
  __device__ __forceinline__ uint8_t operator()(int64_t j) const { return w[j - lo]; }
};

struct SymGeom {
  uint64_t N;        // input bytes
  uint64_t n_load;   // bytes that may be loaded: N rounded up to 16 (the array's extent at least)
  uint32_t C;        // bytes a chunk: a power of two, 64 .. 32768
  uint32_t per;      // consecutive bytes a lane owns: max(16, C / 256)
};

// input bytes [base - 32, base + C) into LDS, 16 B a lane (zero outside [0, n_load))
__device__ __forceinline__ void sym_load(const uint8_t *in, const SymGeom &g, uint64_t base, uint8_t *w) {
  const uint32_t units = (g.C + kSymHalo) / 16;
  for (uint32_t u = threadIdx.x; u < units; u += blockDim.x) {
    const int64_t p = (int64_t)base - kSymHalo + 16 * (int64_t)u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p >= 0 && (uint64_t)p < g.n_load) v = *reinterpret_cast<const uint4 *>(in + p);
    reinterpret_cast<uint4 *>(w)[u] = v;
  }
}

// LDS (dynamic, 16 B aligned): C + 32 bytes, then 4 ints.  Chunks [c0, c0 + nc).  tot: delta (wrapping),
// non-empty line starts, second commas, NULs.
__global__ void __launch_bounds__(256) k_sym_count(const uint8_t *in, SymGeom g, uint64_t c0, uint64_t nc, const int32_t *l2w,
                                                   uint64_t n_labels, uint64_t *cdelta, unsigned long long *tot) {
  extern __shared__ __attribute__((aligned(16))) uint8_t sym_lds[];
  uint8_t *w = sym_lds;
  int *acc = reinterpret_cast<int *>(sym_lds + g.C + kSymHalo);
  unsigned long long sum[4] = {0, 0, 0, 0};  // lane 0's: this workgroup's chunks together
  for (uint64_t c = c0 + blockIdx.x; c < c0 + nc; c += gridDim.x) {
    const uint64_t base = c * g.C;
    sym_load(in, g, base, w);
    if (threadIdx.x < 4) acc[threadIdx.x] = 0;
    __syncthreads();
    const SymWin at{w, (int64_t)base - kSymHalo};
    SymCnt s{0, 0, 0, 0};
    const uint64_t lo = base + (uint64_t)threadIdx.x * g.per;
    if (threadIdx.x * g.per < g.C)
      for (uint64_t i = lo; i < lo + g.per && i < g.N; ++i) sym_count_byte(at, (int64_t)i, l2w, n_labels, s);
    if (s.delta) atomicAdd(&acc[0], s.delta);
    if (s.starts) atomicAdd(&acc[1], s.starts);
    if (s.commas) atomicAdd(&acc[2], s.commas);
    if (s.nuls) atomicAdd(&acc[3], s.nuls);
    __syncthreads();
    if (threadIdx.x == 0) {
      cdelta[c] = (uint64_t)(int64_t)acc[0];
      sum[0] += (unsigned long long)(long long)acc[0];
      for (int k = 1; k < 4; ++k) sum[k] += (unsigned long long)acc[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0)
    for (int k = 0; k < 4; ++k)
      if (sum[k]) atomicAdd(&tot[k], sum[k]);
}

// LDS: C + 32 bytes, then 2 * 256 ints.  coff: the exclusive scan of cdelta.
__global__ void __launch_bounds__(256) k_sym_emit(const uint8_t *in, SymGeom g, uint64_t n_chunks, const int32_t *l2w, uint64_t n_labels,
                                                  const uint64_t *coff, uint8_t *out, uint64_t out_size) {
  extern __shared__ __attribute__((aligned(16))) uint8_t sym_lds[];
  uint8_t *w = sym_lds;
  int *scan = reinterpret_cast<int *>(sym_lds + g.C + kSymHalo);  // [2][256]
  const uint32_t l = threadIdx.x;
  for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint64_t base = c * g.C;
    sym_load(in, g, base, w);
    __syncthreads();
    const SymWin at{w, (int64_t)base - kSymHalo};
    const uint64_t lo = base + (uint64_t)l * g.per;
    const bool mine = l * g.per < g.C;
    SymCnt s{0, 0, 0, 0};
    if (mine)
      for (uint64_t i = lo; i < lo + g.per && i < g.N; ++i) sym_count_byte(at, (int64_t)i, l2w, n_labels, s);
    // inclusive scan of the lanes' deltas (Hillis-Steele, 8 rounds)
    int cur = 0;
    scan[l] = s.delta;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
      scan[(cur ^ 1) * 256 + l] = scan[cur * 256 + l] + (l >= d ? scan[cur * 256 + l - d] : 0);
      cur ^= 1;
      __syncthreads();
    }
    int64_t pre = (int64_t)coff[c] + (int64_t)(scan[cur * 256 + l] - s.delta);
    if (mine)
      for (uint64_t i = lo; i < lo + g.per && i < g.N; ++i) sym_emit_byte(at, (int64_t)i, g.N, l2w, n_labels, &pre, out, out_size);
    __syncthreads();
  }
}

// The --O0 .sym at o0_sym rewritten with l2w (device, n_labels entries) to path.  The input goes up through
// StageIn (stage_io.hpp), a pread a piece, each piece followed on the copy stream by k_sym_count over its
// chunks (a buffer is a whole number of chunks; a chunk's 32 bytes of look-back landed with the buffer before).
static_assert(kIoStageMin % kSymChunkMax == 0, "a staging buffer is a whole number of .sym chunks");
static void write_sym_device(rs_engine *E, const char *o0_sym, const char *path, const int32_t *l2w, uint64_t n_labels) {
  const double t0 = now_ms();
  hipStream_t st = E->st, stc = E->stc;
  const std::string cannot_read = std::string("cannot read ") + o0_sym;
  Fd src;
  src.fd = open(o0_sym, O_RDONLY);
  struct stat sb;
  if (src.fd < 0 || fstat(src.fd, &sb) != 0 || !S_ISREG(sb.st_mode)) throw RsError(RS_E_INVALID, cannot_read);
  const uint64_t N = (uint64_t)sb.st_size;
  uint64_t chunk = env_u64("RS_SYM_CHUNK", kSymChunk, kSymChunkMin, kSymChunkMax);  // (read on every call)
  while (chunk & (chunk - 1)) chunk &= chunk - 1;  // a power of two (rounded down)
  SymGeom g{};
  g.N = N;
  g.n_load = (N + 15) & ~15ull;
  g.C = (uint32_t)chunk;
  g.per = std::max<uint32_t>(16, g.C / 256);
  const uint64_t n_chunks = (N + g.C - 1) / g.C;
  Arena &A = E->SA;
  uint64_t out_size = 0;
  uint8_t *out = nullptr;
  double t_in = t0, t_valid = t0;
  Events<2> emit(hipEventDefault);  // around k_sym_emit
  if (N) {
    uint8_t *in = A.get<uint8_t>("sym.in", g.n_load);
    uint64_t *cdelta = A.get<uint64_t>("sym.cdelta", n_chunks), *coff = A.get<uint64_t>("sym.coff", n_chunks);
    unsigned long long *tot = A.get<unsigned long long>("sym.tot", 4);
    unsigned long long *h_tot = (unsigned long long *)pin_get(E, kPinRead, kPinRb);  // pinned read-back words [0..3]
    const size_t lds_count = g.C + kSymHalo + 16, lds_emit = g.C + kSymHalo + 2 * 256 * sizeof(int);
    uint8_t last = '\n';
    {
      const int fd = src.fd;
      StageIn up(E, N, g.C);
      HC(hipMemsetAsync(tot, 0, 32, stc));
      up.send(in, N, cannot_read, [fd](uint8_t *buf, uint64_t off, uint64_t len) { return pread_all(fd, buf, len, off); },
              [&](const uint8_t *buf, uint64_t off, uint64_t len) {
                if (off + len == N) last = buf[len - 1];
                const uint64_t c0 = off / g.C, nc = (len + g.C - 1) / g.C;
                hipLaunchKernelGGL(k_sym_count, dim3((unsigned)std::min<uint64_t>(nc, 65536)), dim3(256), lds_count, stc, (const uint8_t *)in, g,
                                   c0, nc, l2w, n_labels, cdelta, tot);
                HC(hipGetLastError());
              });
      HC(hipStreamSynchronize(stc));  // the file has landed and is counted
    }
    t_in = now_ms();
    // ---- the chunks' offsets, the totals, the verdict
    excl_scan(A, "sym.scan", st, (const uint64_t *)cdelta, coff, (uint64_t)0, n_chunks, rocprim::plus<uint64_t>());
    HC(hipMemcpyAsync(h_tot, tot, 32, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    if (h_tot[3]) throw RsError(RS_E_INVALID, "bad sym file: a NUL byte");
    if (h_tot[1] != h_tot[2])
      throw RsError(RS_E_INVALID, "bad sym line: not `label,witness,rest` (label 0|[1-9][0-9]{0,9}, witness -?[0-9]{1,10})");
    const int64_t sz = (int64_t)N + (int64_t)h_tot[0] + (last != '\n' ? 1 : 0);
    if (sz < 0 || (uint64_t)sz > 4 * N + 1) throw RsError(RS_E_INTERNAL, "sym image size out of range");  // (a line grows by < 4x)
    out_size = (uint64_t)sz;
    t_valid = now_ms();
    if (out_size) {
      out = A.get<uint8_t>("sym.out", out_size);
      HC(hipEventRecord(emit.e[0], st));
      hipLaunchKernelGGL(k_sym_emit, dim3((unsigned)std::min<uint64_t>(n_chunks, 65536)), dim3(256), lds_emit, st, (const uint8_t *)in, g,
                         n_chunks, l2w, n_labels, (const uint64_t *)coff, out, out_size);
      HC(hipGetLastError());
      HC(hipEventRecord(emit.e[1], st));
    }
  }
  // ---- the file (its blocks up front, while k_sym_emit runs), then the image
  float emit_ms = 0;
  write_image_file(E, path, {}, {}, out, out_size, st, [&] {
    HC(hipEventSynchronize(emit.e[1]));
    HC(hipEventElapsedTime(&emit_ms, emit.e[0], emit.e[1]));
  });
  const double t_end = now_ms();
  E->stats.sym_write_ms = t_end - t0;
  E->stats.sym_in_ms = t_in - t0;
  E->stats.sym_kernel_ms = (t_valid - t_in) + emit_ms;
  E->stats.sym_out_ms = E->stats.sym_write_ms - E->stats.sym_in_ms - E->stats.sym_kernel_ms;
  if (g_prof_env)
    fprintf(stderr, "[rs-prof] write_sym: %.1f MB in, %.1f MB out: in %.2f ms, scan + read-back %.2f ms, emit %.2f ms, out %.2f ms\n", N / 1e6,
            out_size / 1e6, t_in - t0, t_valid - t_in, emit_ms, E->stats.sym_out_ms);
}
#endif  // __HIPCC__
