// r1cs_read.hpp -- SURVEY 8 row A2 on the device: an --O0 .r1cs file -> rs_input
// (rs_engine_read_r1cs_o0 / rs_read_r1cs_o0_device, include/rs_simplify.h), equal field for field to
// rs_read_r1cs_o0 (r1cs_io.cpp), which classifies like dag/src/map_to_constraint_list.rs:12-44.
//
// The host parses the section table and the small sections (header, custom gates) through preads
// (r1cs_o0_open) and never looks at the constraint section: it is streamed through the pinned
// staging buffers (StageIn, stage_io.hpp) to the device, where it is an array of E = size / 4 four-byte slots (every
// size in the format is a multiple of 4, so every linear combination -- `u32 n`, then n x (u32
// signal, fs bytes) -- starts at a slot).  Where the LCs start is sequentially dependent: LC j + 1
// starts where LC j ends.  The device finds the starts in parallel by treating EVERY slot i as a
// candidate count, nxt(i) = i + 1 + word[i] * (1 + fs / 4) (64-bit; past E: the sink), and asking
// which slots the chain from slot 0 visits:
//   k_r1cs_exits    a workgroup per chunk of C slots: nxt in LDS, pointer-jumped log2(C) rounds until
//                   every slot knows its exit, the first position >= the chunk's end its chain reaches
//   k_r1cs_group    a lane per slot of each group's (G chunks) first chunk: follows exits to the group's
//                   exit, at most G dependent loads (every step clears a chunk)
//   k_r1cs_chain    one lane walks the groups from slot 0 and notes each group's entry slot; an entry
//                   outside the group's first chunk (an LC longer than a chunk straddles the group
//                   boundary) walks that group's chunk exits instead: the group table is a fast path only
//   k_r1cs_entries  a lane per group notes every chunk's entry slot (chunks the chain jumps over: none)
//   k_r1cs_mark     a workgroup per chunk: the chunk's words in LDS, one lane walks from the entry and
//                   marks the LCs that fit in the section (one bit a slot), a count per 32 slots
//   (rocprim scan of the counts)
//   k_r1cs_pos      a lane per 32 slots: lc_pos[ordinal] = slot, ordinals >= 3 * n_cons dropped
// Fewer than 3 * n_cons marked LCs: the chain left the section, RS_E_INVALID.  Then
//   k_r1cs_classify a lane per constraint: its class from the three counts, the first two C keys and
//                   p - v[1] == v[0] (r1cs_io.cpp's rule); row and entry counts per destination
//   (one rocprim scan of the ten counts)
//   k_r1cs_emit     a workgroup per 256 constraints: ptr of the six blocks, and the tile's entries dealt
//                   to the lanes in file order (consecutive lanes move consecutive 4 + fs byte entries
//                   to consecutive col / val places); a key >= n_labels sets the error word
// Positions are computed in 64 bits and stored in 32: a section of 2^32 - 1 slots or more (16 GiB) is
// refused before any kernel runs.  Every read of the section is at a slot < E: exits, entries and
// marks are only ever positions <= E that were reached from a slot < E, and an LC is marked (so later
// read) only if it ends at or before E.
#pragma once
// (included by engine.hip inside namespace rs, after its scan helpers and flatten.hpp)

constexpr uint32_t kRrSink = 0xffffffffu;  // a chain that leaves the section; also "no entry"
constexpr uint64_t kRrMaxSlots = 0xffffffffull;
// the sizes (RS_R1CS_CHUNK / RS_R1CS_GROUP override them, for tests): slots a chunk -- a power of two,
// 2 * 4 bytes of LDS a slot in k_r1cs_exits -- and chunks a group
constexpr uint64_t kRrChunk = 2048, kRrChunkMin = 64, kRrChunkMax = 4096;
constexpr uint64_t kRrGroup = 256, kRrGroupMin = 2, kRrGroupMax = 65536;

struct RrGeom {
  uint64_t E;         // slots of the section
  uint32_t W;         // slots of an entry: 1 + fs / 4
  uint32_t C, G;      // slots a chunk (a power of two), chunks a group
  uint64_t n_chunks, n_groups;
};

__device__ __forceinline__ uint32_t rr_nxt(uint64_t i, uint32_t w, uint32_t W, uint64_t E) {
  const uint64_t n = i + 1 + (uint64_t)w * W;  // < 2^36: no overflow
  return n > E ? kRrSink : (uint32_t)n;         // E < 2^32 - 1: a position is never the sink
}

// LDS: 2 * C words
__global__ void __launch_bounds__(256) k_r1cs_exits(const uint32_t *sec, RrGeom g, uint32_t *exitp) {
  extern __shared__ uint32_t rr_lds[];
  for (uint64_t c = blockIdx.x; c < g.n_chunks; c += gridDim.x) {
    const uint64_t base = c * g.C, cend = min(base + g.C, g.E);
    uint32_t *cur = rr_lds, *nx = rr_lds + g.C;
    for (uint32_t j = threadIdx.x; j < g.C; j += blockDim.x) {
      const uint64_t i = base + j;
      cur[j] = i < g.E ? rr_nxt(i, sec[i], g.W, g.E) : kRrSink;
    }
    __syncthreads();
    // a slot's chain has at most C links inside the chunk; round k doubles the links followed
    for (uint32_t r = 1; r < g.C; r <<= 1) {
      int moved = 0;
      for (uint32_t j = threadIdx.x; j < g.C; j += blockDim.x) {
        uint32_t v = cur[j];
        if (v < cend) {  // still inside: base < v (nxt(i) > i)
          v = cur[v - base];
          moved = 1;
        }
        nx[j] = v;
      }
      uint32_t *t = cur;
      cur = nx;
      nx = t;
      if (!__syncthreads_or(moved)) break;
    }
    for (uint32_t j = threadIdx.x; j < g.C; j += blockDim.x)
      if (base + j < g.E) exitp[base + j] = cur[j];
    __syncthreads();
  }
}

__global__ void k_r1cs_group(const uint32_t *exitp, RrGeom g, uint32_t *gexit) {
  const uint64_t GC = (uint64_t)g.G * g.C;
  for (uint64_t x = gtid(); x < g.n_groups * g.C; x += gstride()) {
    const uint64_t grp = x / g.C, i = grp * GC + x % g.C, gend = min((grp + 1) * GC, g.E);
    uint32_t p = kRrSink;
    if (i < g.E) {
      p = exitp[i];
      while (p < gend) p = exitp[p];  // p < gend <= E; the sink is >= E
    }
    gexit[x] = p;
  }
}

// gentry: preset to kRrSink
__global__ void k_r1cs_chain(const uint32_t *exitp, const uint32_t *gexit, RrGeom g, uint32_t *gentry) {
  if (gtid() != 0) return;
  const uint64_t GC = (uint64_t)g.G * g.C;
  uint32_t pos = 0;
  while (pos < g.E) {
    const uint64_t grp = pos / GC, off = pos - grp * GC;
    gentry[grp] = pos;
    if (off < g.C) {
      pos = gexit[grp * g.C + off];
    } else {
      const uint64_t gend = min((grp + 1) * GC, g.E);
      while (pos < gend) pos = exitp[pos];
    }
  }
}

// centry: preset to kRrSink
__global__ void k_r1cs_entries(const uint32_t *exitp, const uint32_t *gentry, RrGeom g, uint32_t *centry) {
  const uint64_t GC = (uint64_t)g.G * g.C;
  for (uint64_t grp = gtid(); grp < g.n_groups; grp += gstride()) {
    uint32_t p = gentry[grp];
    const uint64_t gend = min((grp + 1) * GC, g.E);
    while (p < gend) {
      centry[p / g.C] = p;
      p = exitp[p];
    }
  }
}

// LDS: C words + C / 32 mask words.  mask / cnt: one word per 32 slots (chunk c's at c * C / 32)
__global__ void __launch_bounds__(64) k_r1cs_mark(const uint32_t *sec, const uint32_t *centry, RrGeom g, uint32_t *mask,
                                                   uint64_t *cnt) {
  extern __shared__ uint32_t rr_lds[];
  uint32_t *w = rr_lds, *m = rr_lds + g.C;
  const uint32_t nm = g.C / 32;
  for (uint64_t c = blockIdx.x; c < g.n_chunks; c += gridDim.x) {
    const uint64_t base = c * g.C, cend = min(base + g.C, g.E);
    const uint32_t ent = centry[c];
    for (uint32_t j = threadIdx.x; j < nm; j += blockDim.x) m[j] = 0;
    if (ent != kRrSink)
      for (uint32_t j = threadIdx.x; j < g.C; j += blockDim.x) w[j] = base + j < g.E ? sec[base + j] : 0u;
    __syncthreads();
    if (threadIdx.x == 0 && ent != kRrSink) {
      uint64_t p = ent;  // base <= ent < cend
      while (p < cend) {
        const uint32_t n = rr_nxt(p, w[p - base], g.W, g.E);
        if (n == kRrSink) break;  // this LC runs past the section: the chain ends before it
        const uint32_t j = (uint32_t)(p - base);
        m[j >> 5] |= 1u << (j & 31);
        p = n;
      }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nm; j += blockDim.x) {
      mask[c * nm + j] = m[j];
      cnt[c * nm + j] = (uint64_t)__popc(m[j]);
    }
    __syncthreads();
  }
}

__global__ void k_r1cs_pos(const uint32_t *mask, const uint64_t *ord, uint64_t n_words, uint64_t n_lc, uint32_t *lc_pos) {
  for (uint64_t x = gtid(); x < n_words; x += gstride()) {
    uint32_t m = mask[x];
    uint64_t o = ord[x];
    while (m && o < n_lc) {
      lc_pos[o++] = (uint32_t)(x * 32 + (uint64_t)(__ffs(m) - 1));
      m &= m - 1;
    }
  }
}

// per-constraint counts, scanned together: rows ce, eq, lin, nl | entries ce, eq, lin, nl_a, nl_b, nl_c
constexpr int kRrN = 10;
struct RrCnt {
  uint64_t v[kRrN];
};
struct RrCntPlus {
  __host__ __device__ RrCnt operator()(const RrCnt &x, const RrCnt &y) const {
    RrCnt r;
    for (int i = 0; i < kRrN; ++i) r.v[i] = x.v[i] + y.v[i];
    return r;
  }
};
struct RrPrime {
  uint64_t p[4];
};

// limb i of the value of entry e of the LC at slot pos (W - 1 = fs / 4 words in the file, zero above)
__device__ __forceinline__ uint64_t rr_limb(const uint32_t *sec, uint64_t pos, uint64_t e, uint32_t W, int i) {
  if (2 * (uint32_t)i + 1 >= W) return 0;
  const uint32_t *v = sec + pos + 1 + e * W + 1 + 2 * i;
  return (uint64_t)v[0] | ((uint64_t)v[1] << 32);
}

// cls: 0 constant equality, 1 equality, 2 linear, 3 non-linear (r1cs_io.cpp rs_read_r1cs_o0)
__global__ void k_r1cs_classify(const uint32_t *sec, const uint32_t *lc_pos, uint64_t n_cons, uint32_t W, RrPrime P, uint8_t *cls,
                                RrCnt *cnt) {
  for (uint64_t r = gtid(); r < n_cons; r += gstride()) {
    const uint64_t pc = lc_pos[3 * r + 2];
    const uint32_t na = sec[lc_pos[3 * r]], nb = sec[lc_pos[3 * r + 1]], nc = sec[pc];
    uint8_t c = 3;
    if (na == 0 && nb == 0) {
      c = 2;
      if (nc == 1 || nc == 2) {
        const bool has0 = sec[pc + 1] == 0 || (nc == 2 && sec[pc + 1 + W] == 0);
        if ((has0 && nc == 2) || (!has0 && nc == 1)) {
          c = 0;  // signal_equals_constant
        } else if (!has0 && nc == 2) {
          bool same = true;  // p - v[1] == v[0], limb by limb with the borrow (neg_equal)
          uint64_t borrow = 0;
          for (int i = 0; i < 4; ++i) {
            const uint64_t a = rr_limb(sec, pc, 1, W, i), b = rr_limb(sec, pc, 0, W, i);
            const uint64_t t = P.p[i] - a, d = t - borrow;
            if (d != b) { same = false; break; }
            borrow = (uint64_t)(P.p[i] < a) | (uint64_t)(t < borrow);
          }
          if (same) c = 1;  // signal_equals_signal
        }
      }
    }
    cls[r] = c;
    RrCnt k{};
    k.v[c] = 1;
    if (c == 3) {
      k.v[7] = na;
      k.v[8] = nb;
      k.v[9] = nc;
    } else {
      k.v[4 + c] = nc;
    }
    cnt[r] = k;
  }
}

struct RrOut {
  uint64_t *ptr[6];  // 0 ce, 1 eq, 2 lin, 3 nl_a, 4 nl_b, 5 nl_c
  uint32_t *key[6];
  uint64_t *val[6];
};

// A workgroup per tile of 256 constraints (a lane each for the row pointers), then the tile's entries
// in file order over the lanes.  err |= 2: a key >= n_labels.
__global__ void __launch_bounds__(256) k_r1cs_emit(const uint32_t *sec, const uint32_t *lc_pos, const uint8_t *cls, const RrCnt *pre,
                                                    uint64_t n_cons, uint32_t W, uint64_t n_labels, RrOut O, int *err) {
  __shared__ uint32_t s_pre[257];     // entries of the tile before constraint l (all three parts)
  __shared__ uint32_t s_scan[2][256];
  __shared__ uint32_t s_pos[3][256], s_n[3][256];
  __shared__ uint64_t s_dst[3][256];
  __shared__ uint8_t s_cls[256];
  const uint32_t l = threadIdx.x;
  const uint64_t n_tiles = (n_cons + 255) / 256;
  for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const uint64_t r = tile * 256 + l;
    uint32_t tot = 0;
    if (r < n_cons) {
      const uint8_t c = cls[r];
      const RrCnt P = pre[r];
      s_cls[l] = c;
      for (int q = 0; q < 3; ++q) {
        const uint32_t p = lc_pos[3 * r + q];
        s_pos[q][l] = p;
        s_n[q][l] = sec[p];
        tot += s_n[q][l];
      }
      if (c == 3) {
        for (int q = 0; q < 3; ++q) {
          s_dst[q][l] = P.v[7 + q];
          O.ptr[3 + q][P.v[3]] = P.v[7 + q];
        }
      } else {
        s_dst[0][l] = s_dst[1][l] = 0;  // (a linear row's A and B are empty)
        s_dst[2][l] = P.v[4 + c];
        O.ptr[c][P.v[c]] = P.v[4 + c];
      }
    }
    // inclusive scan of tot over the tile (Hillis-Steele, 8 rounds); E < 2^32 bounds every sum
    int cur = 0;
    s_scan[0][l] = tot;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
      s_scan[cur ^ 1][l] = s_scan[cur][l] + (l >= d ? s_scan[cur][l - d] : 0u);
      cur ^= 1;
      __syncthreads();
    }
    s_pre[l + 1] = s_scan[cur][l];
    if (l == 0) s_pre[0] = 0;
    __syncthreads();
    const uint32_t T = s_pre[256];
    for (uint32_t x = l; x < T; x += 256) {
      uint32_t lo = 0, hi = 256;  // the last constraint whose first entry is <= x
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_pre[mid] <= x) lo = mid;
        else hi = mid;
      }
      uint32_t e = x - s_pre[lo];
      int q = 0;
      while (q < 2 && e >= s_n[q][lo]) e -= s_n[q++][lo];  // which part (x < s_pre[lo + 1]: inside part 2 at the latest)
      const uint32_t *src = sec + (uint64_t)s_pos[q][lo] + 1 + (uint64_t)e * W;
      const int ob = s_cls[lo] == 3 ? 3 + q : s_cls[lo];
      const uint64_t z = s_dst[q][lo] + e;
      const uint32_t k = src[0];
      if (k >= n_labels) atomicOr(err, 2);
      O.key[ob][z] = k;
      uint64_t *o = O.val[ob] + 4 * z;
      for (int i = 0; i < 4; ++i)
        o[i] = 2 * (uint32_t)i + 1 < W ? ((uint64_t)src[1 + 2 * i] | ((uint64_t)src[2 + 2 * i] << 32)) : 0ull;
    }
    __syncthreads();
  }
}

// buf(slot, bytes): as flatten_dag's -- slots 3q, 3q + 1, 3q + 2 for block q's ptr, col, val, 18 for
// forbidden.  The section goes up through StageIn (stage_io.hpp), a pread a piece, on the calling thread.
static void read_r1cs_device(rs_engine *E, const char *path, rs_input *in, const std::function<void *(int, size_t)> &buf) {
  hipStream_t st = E->st;
  const double t0 = now_ms();
  R1csSections S;
  R1csO0Head H;
  Fd file;
  if (!r1cs_o0_open(path, &file.fd, S, H)) throw RsError(RS_E_INVALID, rs_last_error());
  const uint64_t n_cons = H.n_cons, n_lc = 3 * n_cons;
  RrGeom g{};
  g.E = S.size[2] / 4;
  g.W = 1 + H.fs / 4;
  uint64_t chunk = env_u64("RS_R1CS_CHUNK", kRrChunk, kRrChunkMin, kRrChunkMax);
  while (chunk & (chunk - 1)) chunk &= chunk - 1;  // a power of two (rounded down)
  g.C = (uint32_t)chunk;
  g.G = (uint32_t)env_u64("RS_R1CS_GROUP", kRrGroup, kRrGroupMin, kRrGroupMax);
  g.n_chunks = (g.E + g.C - 1) / g.C;
  g.n_groups = (g.n_chunks + g.G - 1) / g.G;
  if (g.E >= kRrMaxSlots) throw RsError(RS_E_INVALID, "r1cs constraint section of 16 GiB or more: positions are stored in 32 bits");
  if (n_cons && g.E == 0) throw RsError(RS_E_INVALID, "truncated r1cs section");
  Arena &A = E->A;
  uint64_t rows[6] = {0, 0, 0, 0, 0, 0}, nnz[6] = {0, 0, 0, 0, 0, 0};
  RrOut O{};
  double t_up = t0, t_k = t0;
  if (n_cons) {
    // ---- the tables (an arena buffer that grows is a hipFree, which waits for the device: before the upload)
    uint32_t *sec = A.get<uint32_t>("rr.sec", g.E);  // (hipMalloc: aligned)
    const uint64_t n_words = g.n_chunks * (g.C / 32);
    uint32_t *exitp = A.get<uint32_t>("rr.exit", g.E);
    uint32_t *gexit = A.get<uint32_t>("rr.gexit", g.n_groups * g.C);
    uint32_t *gentry = A.get<uint32_t>("rr.gentry", g.n_groups);
    uint32_t *centry = A.get<uint32_t>("rr.centry", g.n_chunks);
    uint32_t *mask = A.get<uint32_t>("rr.mask", n_words);
    uint64_t *mcnt = A.get<uint64_t>("rr.mcnt", n_words), *mord = A.get<uint64_t>("rr.mord", n_words);
    uint32_t *lc_pos = A.get<uint32_t>("rr.lcpos", n_lc);
    uint8_t *cls = A.get<uint8_t>("rr.cls", n_cons);
    RrCnt *cnt = A.get<RrCnt>("rr.cnt", n_cons), *pre = A.get<RrCnt>("rr.pre", n_cons);
    int *d_err = A.get<int>("rr.err", 1);
    HC(hipMemsetAsync(d_err, 0, 4, st));
    HC(hipMemsetAsync(gentry, 0xff, 4 * g.n_groups, st));
    HC(hipMemsetAsync(centry, 0xff, 4 * g.n_chunks, st));
    // ---- section 2 -> device, untouched
    {
      const int fd = file.fd;
      const uint64_t off2 = S.off[2];
      StageIn up(E, 4 * g.E);
      up.send(sec, 4 * g.E, std::string("cannot read r1cs file ") + path,
              [fd, off2](uint8_t *dst, uint64_t off, uint64_t len) { return pread_all(fd, dst, len, off2 + off); });
      HC(hipStreamSynchronize(E->stc));  // the section has landed
    }
    t_up = now_ms();
    Marks mk{{}, st};  // RS_PROF: the time of every step (the stream synchronised at each mark)
    mk.mark("read_r1cs: start");
    // ---- the LC starts
    const unsigned cgrid = (unsigned)std::min<uint64_t>(g.n_chunks, 65536);
    hipLaunchKernelGGL(k_r1cs_exits, dim3(cgrid), dim3(256), 8 * g.C, st, (const uint32_t *)sec, g, exitp);
    HC(hipGetLastError());
    mk.mark("exits");
    launch(st, k_r1cs_group, g.n_groups * g.C, (const uint32_t *)exitp, g, gexit);
    mk.mark("group");
    hipLaunchKernelGGL(k_r1cs_chain, dim3(1), dim3(64), 0, st, (const uint32_t *)exitp, (const uint32_t *)gexit, g, gentry);
    HC(hipGetLastError());
    mk.mark("chain");
    launch(st, k_r1cs_entries, g.n_groups, (const uint32_t *)exitp, (const uint32_t *)gentry, g, centry);
    mk.mark("entries");
    hipLaunchKernelGGL(k_r1cs_mark, dim3(cgrid), dim3(64), 4 * g.C + 4 * (g.C / 32), st, (const uint32_t *)sec, (const uint32_t *)centry, g,
                       mask, mcnt);
    HC(hipGetLastError());
    const uint64_t n_found = excl_scan_u64(E, mcnt, mord, n_words, "rr");
    mk.mark("mark+scan");
    if (n_found < n_lc) throw RsError(RS_E_INVALID, "truncated r1cs constraint");
    launch(st, k_r1cs_pos, n_words, (const uint32_t *)mask, (const uint64_t *)mord, n_words, n_lc, lc_pos);
    mk.mark("pos");
    // ---- classes, counts, their scan
    RrPrime P;
    memcpy(P.p, H.prime, 32);
    launch(st, k_r1cs_classify, n_cons, (const uint32_t *)sec, (const uint32_t *)lc_pos, n_cons, g.W, P, cls, cnt);
    mk.mark("classify");
    excl_scan(A, "rr.scan", st, (const RrCnt *)cnt, pre, RrCnt{}, n_cons, RrCntPlus());
    RrCnt last_c, last_p;
    HC(hipMemcpyAsync(&last_c, cnt + n_cons - 1, sizeof(RrCnt), hipMemcpyDeviceToHost, st));
    HC(hipMemcpyAsync(&last_p, pre + n_cons - 1, sizeof(RrCnt), hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    mk.mark("scan");
    uint64_t tot[kRrN];
    for (int k = 0; k < kRrN; ++k) tot[k] = last_c.v[k] + last_p.v[k];
    for (int q = 0; q < 6; ++q) {
      rows[q] = tot[q < 3 ? q : 3];
      nnz[q] = tot[4 + q];
      const std::string nm = "rr.o" + std::to_string(q);
      O.ptr[q] = A.get<uint64_t>(nm + ".ptr", rows[q] + 1);
      O.key[q] = A.get<uint32_t>(nm + ".key", nnz[q]);
      O.val[q] = A.get<uint64_t>(nm + ".val", 4 * nnz[q]);
    }
    const unsigned egrid = (unsigned)std::min<uint64_t>((n_cons + 255) / 256, 65536);
    hipLaunchKernelGGL(k_r1cs_emit, dim3(egrid), dim3(256), 0, st, (const uint32_t *)sec, (const uint32_t *)lc_pos, (const uint8_t *)cls,
                       (const RrCnt *)pre, n_cons, g.W, H.n_labels, O, d_err);
    HC(hipGetLastError());
    int err = 0;
    HC(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    if (err) throw RsError(RS_E_INVALID, "r1cs constraint: signal >= n_labels");
    mk.mark("emit");
    mk.dump();
    t_k = now_ms();
  }
  // ---- the rs_input
  in->prime_id = H.prime_id;
  memcpy(in->prime, H.prime, 32);
  in->max_signal = H.n_labels;
  in->n_pub_out = H.n_out;
  in->n_pub_in = H.n_pub;
  in->n_priv_in = H.n_prv;
  rs_lc *outs[6] = {&in->cons_eq, &in->eq, &in->linear, &in->nl_a, &in->nl_b, &in->nl_c};
  for (int q = 0; q < 6; ++q) {
    rs_lc &o = *outs[q];
    o.n_rows = rows[q];
    o.nnz = nnz[q];
    o.ptr = (uint64_t *)buf(3 * q, 8 * (rows[q] + 1));
    o.col = (uint32_t *)buf(3 * q + 1, 4 * std::max<uint64_t>(nnz[q], 1));
    o.val = (uint64_t *)buf(3 * q + 2, 32 * std::max<uint64_t>(nnz[q], 1));
    if (rows[q]) HC(hipMemcpyAsync(o.ptr, O.ptr[q], 8 * rows[q], hipMemcpyDeviceToHost, st));
    if (nnz[q]) {
      HC(hipMemcpyAsync(o.col, O.key[q], 4 * nnz[q], hipMemcpyDeviceToHost, st));
      HC(hipMemcpyAsync(o.val, O.val[q], 32 * nnz[q], hipMemcpyDeviceToHost, st));
    }
  }
  in->n_forbidden = H.forbidden.size();
  in->forbidden = (uint32_t *)buf(18, 4 * std::max<size_t>(H.forbidden.size(), 1));
  if (!H.forbidden.empty()) memcpy(in->forbidden, H.forbidden.data(), 4 * H.forbidden.size());
  HC(hipStreamSynchronize(st));
  for (int q = 0; q < 6; ++q) outs[q]->ptr[rows[q]] = nnz[q];  // (row r's pointer came from the device; the end is known here)
  const double t_end = now_ms();
  E->stats.read_ms = t_end - t0;
  E->stats.read_upload_ms = t_up - t0;
  E->stats.read_kernel_ms = t_k - t_up;
  E->stats.read_d2h_ms = t_end - t_k;
  if (g_prof_env)
    fprintf(stderr, "[rs-prof] read_r1cs: %.1f MB section, %llu constraints: open + upload %.2f ms, kernels %.2f ms, D2H %.2f ms\n",
            4.0 * g.E / 1e6, (unsigned long long)n_cons, t_up - t0, t_k - t_up, t_end - t_k);
}
