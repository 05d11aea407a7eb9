// run.hpp -- one simplification run on a loaded engine: struct Run, one member function per phase of
// simplification() (constraint_simplification.rs:442-730), and engine_run, which calls them in order.
// Included by engine.hip inside namespace rs, after everything a run uses: the engine, the load's
// waits, the elimination driver, the result stream's thread (snap_push) and ensure_csr.
#pragma once

// the arena name of part q's buffer: pre + 'a' / 'b' / 'c' + suf
static std::string part_name(const char *pre, int q, const char *suf) { return std::string(pre) + "abc"[q] + suf; }

// Keys-first linear rows (constant_eq): at most max(kUncMin, rows / kUncDiv) rows may need their values
// from the host input; one more and the run waits for the values and takes the frames on values.
constexpr uint64_t kUncMin = 1024, kUncDiv = 16;

// The state of one run: what simplification() (constraint_simplification.rs:442-730) keeps in its
// locals, and one member function per phase, called in order by engine_run.  A field a phase sets for
// a later one says so.
struct Run {
  rs_engine *const E;
  const rs_flags *const fl;
  Arena &A;
  const hipStream_t st;
  const uint64_t S;
  KGroup &kg1;  // kg[1]'s algorithmic bytes: k_make_ragged reads the CSR and writes the ragged copy, 72 B an
                // entry and 20 a row; the linear rows' frames read what they rewrite (+ eq_rep / ce_has per entry)
  const bool apply_linear;  // --O2 (not --O1)
  uint64_t no_rounds;       // rounds still allowed (non_linear_frames and every round take one)
  double T0 = 0, Tf = 0;    // start of the run / of the final assembly
  // the error and signal bitmaps (init; eq_rep: eq_simplification; ce_has / ce_val: constant_eq)
  int *d_err = nullptr;
  uint8_t *d_forb = nullptr, *d_deleted = nullptr;
  int32_t *sub_of = nullptr, *eq_rep = nullptr;
  uint8_t *ce_has = nullptr;
  Fe *ce_val = nullptr;
  LcHeap lc;  // lconst (device): every phase appends, assemble reads
  // working copies (Montgomery): cons_eq (C), linear (C, one spare slot per row)
  DRows ce{}, lin{};
  // the linear rows' keys went first (constant_eq): their values follow in linear_values, which
  // linear_round1 hands to the elimination; lin_fixed: rows already settled from host values
  bool keys_first = false;
  uint8_t *lin_fixed = nullptr;
  // the non-linear rows: input copies (stage_nl, on first use: nl_staged), storage views over the heap
  const uint64_t n_nl;
  // (every triple is indexed by part: 0 = A, 1 = B, 2 = C)
  DRows nl_in[3] = {};
  bool nl_staged = false;
  DRows stor[3] = {};
  uint64_t heap_top = 0;
  uint32_t *heap_k = nullptr;  // (the engine's heap; heap_reserve moves it)
  Fe *heap_v = nullptr;
  unsigned long long *d_bytes = nullptr;
  int *d_fw_err = nullptr;
  FrameArgs fr;  // setup_non_linear; the pool's pointers by head_overlap / non_linear_frames
  uint64_t *cap[3] = {};  // capacity columns of a frames pass
  U3 *cap3 = nullptr, *sc3 = nullptr;
  // the late rows: those touching the head clusters, skipped by the first pass.  Set by head_overlap
  // (hmark, the lists) and its nl_phase (n_late); read by non_linear_frames' second pass and snap_take2
  uint64_t *nl_late = nullptr, *nl_lpos = nullptr;
  uint8_t *hmark = nullptr;
  uint32_t *nl_lids = nullptr;
  uint64_t n_late = 0;
  bool nl_split = false;  // head_overlap ran the first pass: non_linear_frames runs only the late rows
  bool fh_split = false;  // the last nl_phase ran in two halves (ev_fh): set by nl_phase, consumed by nl_ms
  // streamed output: which storage rows are in the early region and where (snap_take and the later
  // snapshots; read by assemble), the rows a round rewrote (rounds)
  uint8_t *so_early = nullptr;
  U3 *so_eoff = nullptr;
  uint8_t *so_dirty = nullptr;
  // round 1's elimination (linear_round1) and the substitution pool of every round
  ElimOut eo;
  Pool P;
  // non_linear_frames: storage rows / rows turned linear (ids into the non-linear rows, DFS order),
  // the compacted storage views, the non-linear signal map's key set, the current linear list (C only)
  uint64_t n_st = 0, n_wl = 0;
  uint32_t *st_ids = nullptr, *wl_ids = nullptr;
  DRows sv[3] = {};
  uint8_t *nlmap = nullptr;
  DRows lv{};
  // rounds >= 2: the round-1 storage rows (the signal map's initial lists are built from them on
  // demand: query_initial), the appended lists (maplists.hpp), the per-round scratch bitmaps
  bool apply_round = false;
  DRows m0[3] = {};
  MapLists ML;
  uint8_t *qflag = nullptr;
  int32_t *rank_of = nullptr, *r_sub_of = nullptr;
  // one round (reset by round_once): its elimination, its ordered substitutions (round_order: `from`,
  // RHS location; usig: the host copy, need_usig), the rows it turned linear (round_apply: (order key,
  // storage id)), RS_PROF's marks
  ElimOut er;
  Marks MK;
  uint64_t nU = 0;
  uint32_t *d_us = nullptr, *d_ulen = nullptr;
  uint64_t *d_uoff = nullptr;
  std::vector<uint32_t> usig;
  std::vector<std::pair<uint64_t, uint32_t>> turned;

  Run(rs_engine *e, const rs_flags *f)
      : E(e), fl(f), A(e->A), st(e->st), S(e->S), kg1(e->kg[1]), apply_linear(!f->flag_s), no_rounds(f->no_rounds), n_nl(e->na.n) {}

  // ======================= init
  // Reads the engine as the load left it.  Leaves: the cleared error word and signal bitmaps
  // (d_err, d_forb, d_deleted, sub_of), the elimination's scratch defaults, an empty lconst heap, no
  // result stream, an empty substitution log.
  void init() {
    E->stats = rs_stats{};
    E->stats.world = E->comm ? (uint64_t)E->comm->world : 1;
    for (int g = 1; g < 3; ++g) {  // (kg[0]: the load's checks, recorded before the run)
      E->kg[g].n = 0;
      E->kg[g].bytes = 0;
    }
    if (E->A.defer || !E->A.graveyard.empty()) {  // an exchange a failed run left mid-way: its deferred frees
      for (hipStream_t q : {E->st, E->st2, E->stc, E->ste, E->stg})  // (nothing still reads them)
        if (q) (void)hipStreamSynchronize(q);
      E->A.defer = false;
      E->A.flush();
    }
    T0 = now_ms();
    d_err = A.get<int>("err", 1);
    HC(hipMemsetAsync(d_err, 0, 4, st));

    // forbidden bitmap, deleted, scratch defaults
    d_forb = A.get<uint8_t>("forb", S);
    d_deleted = A.get<uint8_t>("deleted", S);
    HC(hipMemsetAsync(d_forb, 0, S, st));
    HC(hipMemsetAsync(d_deleted, 0, S, st));
    {
      uint32_t *d_fl = A.get<uint32_t>("forb.list", E->forbidden.size());
      h2d(E, d_fl, E->forbidden.data(), 4 * E->forbidden.size());
      launch(st, k_mark_list, E->forbidden.size(), (const uint32_t *)d_fl, (uint64_t)E->forbidden.size(), d_forb);
    }
    for (const char *nm : {"el.holder_idx", "el.occ", "el.noov", "el.rep_pos"})
      HC(hipMemsetAsync(A.get<int32_t>(nm, S), 0xff, 4 * S, st));
    HC(hipMemsetAsync(A.get<uint8_t>("el.del", S), 0, S, st));
    sub_of = A.get<int32_t>("sub_of", S);
    HC(hipMemsetAsync(sub_of, 0xff, 4 * S, st));

    snap_join(E);
    E->snap_on = false;
    E->lc_snap_n = 0;
    E->csr_ready = false;
    E->log_on = fl->emit_substitution_log != 0;
    E->log_from.clear();
    E->log_key.clear();
    E->log_val.clear();
    E->log_ptr.assign(1, 0);
  }

  // ======================= eq_simplification (:198-251) + renaming of linear / cons_eq rows
  // Reads input group 0 (cons_eq, eq), d_forb, d_deleted.  Leaves: eq_rep (signal -> representative),
  // the forbidden-only constraints in lc, the logged substitutions (log_substitutions, :249 / :271),
  // and the Montgomery working copies ce (renamed) and lin (allocated; filled by constant_eq).
  void eq_simplification() {
    load_wait(E, 0);
    eq_rep = A.get<int32_t>("eq_rep", S);
    HC(hipMemsetAsync(eq_rep, 0xff, 4 * S, st));
    {
      uint32_t *uf = A.get<uint32_t>("uf", S);
      uint32_t *cnt = A.get<uint32_t>("eq.cnt", S);
      int32_t *maxrow = A.get<int32_t>("eq.maxrow", S);
      uint32_t *minf = A.get<uint32_t>("eq.minf", S);
      uint32_t *minr = A.get<uint32_t>("eq.minr", S);
      uint8_t *in_eq = A.get<uint8_t>("eq.in", S);
      uint32_t *bf = A.get<uint32_t>("eq.bf", E->eq.n);
      uint32_t *bfn = A.get<uint32_t>("eq.bfn", 1);
      launch(st, k_iota_u32, S, uf, S);
      HC(hipMemsetAsync(cnt, 0, 4 * S, st));
      HC(hipMemsetAsync(maxrow, 0xff, 4 * S, st));
      HC(hipMemsetAsync(minf, 0xff, 4 * S, st));
      HC(hipMemsetAsync(minr, 0xff, 4 * S, st));
      HC(hipMemsetAsync(in_eq, 0, S, st));
      HC(hipMemsetAsync(bfn, 0, 4, st));
      if (E->eq.n) {
        launch(st, k_eq_union, E->eq.n, (const uint64_t *)E->eq.ptr, (const uint32_t *)E->eq.key, E->eq.n, uf, d_err);
        launch(st, k_eq_stats, E->eq.n, (const uint64_t *)E->eq.ptr, (const uint32_t *)E->eq.key, E->eq.n, uf,
               (const uint8_t *)d_forb, cnt, maxrow, minf, minr, in_eq);
        launch(st, k_eq_assign, E->eq.n, (const uint64_t *)E->eq.ptr, (const uint32_t *)E->eq.key, E->eq.n, uf,
               (const uint8_t *)d_forb, (const uint32_t *)minf, (const uint32_t *)minr, eq_rep, d_deleted, bf, bfn);
      }
      if (E->log_on && E->eq.n) {  // log_substitutions (:249)
        uint64_t *lk = A.get<uint64_t>("lg.eqk", S), *lk2 = A.get<uint64_t>("lg.eqk2", S);
        uint32_t *lr = A.get<uint32_t>("lg.eqr", S), *lr2 = A.get<uint32_t>("lg.eqr2", S);
        unsigned long long *ln = A.get<unsigned long long>("lg.eqn", 1);
        HC(hipMemsetAsync(ln, 0, 8, st));
        launch(st, k_eq_log_keys, S, (const int32_t *)eq_rep, uf, (const uint32_t *)cnt, (const int32_t *)maxrow, S, lk, lr, ln);
        unsigned long long nlog = 0;
        HC(hipMemcpyAsync(&nlog, ln, 8, hipMemcpyDeviceToHost, st));
        HC(hipStreamSynchronize(st));
        sort_pairs(E, (const uint64_t *)lk, lk2, (const uint32_t *)lr, lr2, nlog, 64, "lgeq");
        std::vector<uint64_t> hk(nlog);
        std::vector<uint32_t> hr(nlog);
        if (nlog) {
          HC(hipMemcpyAsync(hk.data(), lk2, 8 * nlog, hipMemcpyDeviceToHost, st));
          HC(hipMemcpyAsync(hr.data(), lr2, 4 * nlog, hipMemcpyDeviceToHost, st));
          HC(hipStreamSynchronize(st));
        }
        const uint64_t one[4] = {1, 0, 0, 0};
        for (uint64_t i = 0; i < nlog; ++i) log_push(E, (uint32_t)hk[i], &hr[i], one, 1);  // Substitution::new(Signal)
      }
      // eq cons (forbidden-only constraints), ordered by cluster index (= max row) then signal
      uint64_t nf = E->forbidden.size();
      uint32_t *fl_d = A.get<uint32_t>("forb.list", nf);
      uint32_t *g_root = A.get<uint32_t>("eq.g_root", nf);
      HC(hipMemsetAsync(g_root, 0, 4 * nf, st));
      launch(st, k_uf_roots, nf, uf, (const uint32_t *)fl_d, g_root, nf);
      uint32_t nbf = 0;
      HC(hipMemcpyAsync(&nbf, bfn, 4, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
      struct EqCon {  // a row of C: keys ascending, canonical values
        int64_t order;
        uint32_t f;
        std::vector<uint32_t> k;
        std::vector<uint64_t> v;
      };
      std::vector<EqCon> eqc;
      // per forbidden signal: in an eq cluster?  cluster size, min forbidden, max row (one gather)
      std::vector<uint32_t> finfo(4 * nf);
      if (nf) {
        uint32_t *d_fi = A.get<uint32_t>("eq.finfo", 4 * nf);
        launch(st, k_eq_forb_info, nf, (const uint32_t *)fl_d, nf, (const uint32_t *)g_root, (const uint8_t *)in_eq,
               (const uint32_t *)cnt, (const uint32_t *)minf, (const int32_t *)maxrow, d_fi);
        HC(hipMemcpyAsync(finfo.data(), d_fi, 16 * nf, hipMemcpyDeviceToHost, st));
        HC(hipStreamSynchronize(st));
      }
      for (uint64_t i = 0; i < nf; ++i) {
        uint32_t f = E->forbidden[i];
        if (!finfo[4 * i]) continue;
        uint32_t c = finfo[4 * i + 1], mf = finfo[4 * i + 2];
        int32_t mr = (int32_t)finfo[4 * i + 3];
        if (c <= 1 || f == mf) continue;
        // transform(sub(Signal f, Signal rh)) = {0: 0, rh: 1, f: -1}
        EqCon e;
        e.order = mr;
        e.f = f;
        uint64_t one[4] = {1, 0, 0, 0}, m1[4];
        memcpy(m1, E->prime, 32);
        m1[0] -= 1;
        e.k = {0};
        e.v = {0, 0, 0, 0};
        if (mf < f) {
          e.k.push_back(mf); e.v.insert(e.v.end(), one, one + 4);
          e.k.push_back(f); e.v.insert(e.v.end(), m1, m1 + 4);
        } else {
          e.k.push_back(f); e.v.insert(e.v.end(), m1, m1 + 4);
          e.k.push_back(mf); e.v.insert(e.v.end(), one, one + 4);
        }
        eqc.push_back(std::move(e));
      }
      if (nbf) {  // rows with both ends forbidden: kept as is when they are a cluster of their own
        std::vector<uint64_t> rec(11 * (uint64_t)nbf);
        uint64_t *d_rec = A.get<uint64_t>("eq.bfrec", 11 * (uint64_t)nbf);
        // staged load: the eq values were never uploaded; these rows take theirs from the host input
        launch(st, k_eq_bf_info, nbf, (const uint32_t *)bf, (uint64_t)nbf, (const uint64_t *)E->eq.ptr,
               (const uint32_t *)E->eq.key, E->hin ? (const Fe *)nullptr : (const Fe *)E->eq.val, (const uint32_t *)uf,
               (const uint32_t *)cnt, d_rec);
        HC(hipMemcpyAsync(rec.data(), d_rec, 88 * (uint64_t)nbf, hipMemcpyDeviceToHost, st));
        HC(hipStreamSynchronize(st));
        for (uint32_t q = 0; q < nbf; ++q) {
          uint64_t *x = &rec[11 * (uint64_t)q];
          if (x[2] != 1) continue;  // a single-constraint cluster with both ends forbidden: kept as is
          if (E->hin) {
            const rs_lc &H = E->hin->eq;
            const uint64_t p0 = H.ptr[x[0]];
            for (int t = 0; t < 4; ++t) { x[3 + t] = H.val[4 * p0 + t]; x[7 + t] = H.val[4 * (p0 + 1) + t]; }
            for (int e2 = 0; e2 < 2; ++e2) {
              const uint64_t *v = x + 3 + 4 * e2;
              if ((v[0] | v[1] | v[2] | v[3]) == 0 || geq4(v, E->prime))
                throw RsError(RS_E_INVALID, "eq block: zero or non-canonical value");
            }
            if ((uint32_t)x[1] > (uint32_t)(x[1] >> 32)) {  // the device sorted rows; these are as given
              x[1] = (x[1] << 32) | (x[1] >> 32);
              for (int t = 0; t < 4; ++t) std::swap(x[3 + t], x[7 + t]);
            }
          }
          EqCon e;
          e.order = (int64_t)x[0];
          e.f = 0;
          e.k = {(uint32_t)x[1], (uint32_t)(x[1] >> 32)};
          e.v.assign(x + 3, x + 11);
          eqc.push_back(std::move(e));
        }
      }
      std::sort(eqc.begin(), eqc.end(), [](const EqCon &x, const EqCon &y) {
        return x.order != y.order ? x.order < y.order : x.f < y.f;
      });
      if (!eqc.empty()) {  // to the device (canonical -> Montgomery), then into the lconst heap
        const uint64_t ne = eqc.size();
        std::vector<uint64_t> ho(ne);
        std::vector<uint32_t> hl(ne), hk;
        std::vector<uint64_t> hv;
        for (uint64_t i = 0; i < ne; ++i) {
          ho[i] = hk.size();
          hl[i] = (uint32_t)eqc[i].k.size();
          hk.insert(hk.end(), eqc[i].k.begin(), eqc[i].k.end());
          hv.insert(hv.end(), eqc[i].v.begin(), eqc[i].v.end());
        }
        DRows src{};
        src.n = ne;
        src.off = A.get<uint64_t>("lc.eo", ne);
        src.len = A.get<uint32_t>("lc.el", ne);
        src.key = A.get<uint32_t>("lc.ek", hk.size());
        src.val = A.get<Fe>("lc.ev", hk.size());
        h2d(E, src.off, ho.data(), 8 * ne);
        h2d(E, src.len, hl.data(), 4 * ne);
        h2d(E, src.key, hk.data(), 4 * hk.size());
        h2d(E, src.val, hv.data(), 8 * hv.size());
        launch(st, k_to_mont, hk.size(), E->F, (const Fe *)src.val, src.val, (uint64_t)hk.size());
        lc.append(E, src, nullptr, ne);
      }
    }

    // working copies (Montgomery): cons_eq (C), linear (C, one spare slot per row)
    ce.n = E->ce.n;
    ce.off = A.get<uint64_t>("ce.off", ce.n);
    ce.len = A.get<uint32_t>("ce.len", ce.n);
    ce.key = A.get<uint32_t>("ce.key", E->ce.nnz);
    ce.val = A.get<Fe>("ce.val", E->ce.nnz);
    // kg[1]'s algorithmic bytes: k_make_ragged reads the CSR and writes the ragged copy, 72 B an entry
    // and 20 a row; the linear rows' frames read what they rewrite (+ eq_rep / ce_has per entry)
    if (ce.n)
      kg1.run(st, 72 * E->ce.nnz + 20 * ce.n + 8, [&] {
        launch(st, k_make_ragged, ce.n, E->F, (const uint64_t *)E->ce.ptr, (const uint32_t *)E->ce.key, (const Fe *)E->ce.val, ce.n,
               (uint64_t)0, ce.off, ce.len, ce.key, ce.val);
      });
    lin.n = E->lin.n;
    lin.off = A.get<uint64_t>("lin.off", lin.n);
    lin.len = A.get<uint32_t>("lin.len", lin.n);
    lin.key = A.get<uint32_t>("lin.key", E->lin.nnz + lin.n);
    lin.val = A.get<Fe>("lin.val", E->lin.nnz + lin.n);
    if (ce.n) launch(st, k_rename_rows, ce.n, E->F, ce, (const int32_t *)eq_rep);
    if (E->log_on && ce.n) {  // log_substitutions (:271), row order
      uint32_t *lsig = A.get<uint32_t>("lg.cesig", ce.n);
      uint64_t *lval = A.get<uint64_t>("lg.ceval", 4 * ce.n);
      launch(st, k_const_log, ce.n, E->F, ce, (const uint8_t *)d_forb, lsig, lval);
      std::vector<uint32_t> hs(ce.n);
      std::vector<uint64_t> hv(4 * ce.n);
      HC(hipMemcpyAsync(hs.data(), lsig, 4 * ce.n, hipMemcpyDeviceToHost, st));
      HC(hipMemcpyAsync(hv.data(), lval, 32 * ce.n, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
      const uint32_t k0 = 0;
      for (uint64_t r = 0; r < ce.n; ++r)
        if (hs[r] != RS_NONE) log_push(E, hs[r], &k0, &hv[4 * r], is_zero4(&hv[4 * r]) ? 0 : 1);
    }

  }

  // ======================= constant_eq_simplification (:253-273), then the linear rows' frames
  // Reads ce, eq_rep, input group 1 (and 2 unless the keys go first).  Leaves: ce_has / ce_val (signal
  // -> constant), the kept constant rows in lc, lin renamed and with its constants folded -- or, keys
  // first (keys_first, lin_fixed: set here, read by linear_values and linear_round1), lin's keys only.
  void constant_eq() {
    int32_t *ce_last = A.get<int32_t>("ce.last", S);
    ce_has = A.get<uint8_t>("ce.has", S);
    ce_val = A.get<Fe>("ce.val_s", S);
    HC(hipMemsetAsync(ce_last, 0xff, 4 * S, st));
    HC(hipMemsetAsync(ce_has, 0, S, st));
    {
      uint32_t *cl = A.get<uint32_t>("ce.cons", ce.n);
      uint32_t *cn = A.get<uint32_t>("ce.consn", 1);
      HC(hipMemsetAsync(cn, 0, 4, st));
      if (ce.n) {
        launch(st, k_const_pick, ce.n, ce, (const uint8_t *)d_forb, ce_last, d_deleted, cl, cn, d_err);
        launch(st, k_const_value, ce.n, E->F, ce, (const uint8_t *)d_forb, (const int32_t *)ce_last, ce_val, ce_has);
      }
      uint32_t ncons = 0;
      HC(hipMemcpyAsync(&ncons, cn, 4, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
      if (ncons) {  // the kept rows in row order (k_const_pick listed them in any order)
        uint32_t *sorted = A.get<uint32_t>("ce.cons_sorted", ncons);
        sort_keys(E, (const uint32_t *)cl, sorted, ncons, 32, "ce");
        lc.append(E, ce, sorted, ncons);
      }
    }
    // the linear rows: keys first when their values are still on the way (staged load, sorted rows,
    // no renaming collision) -- build_clusters needs keys only; the values follow in
    // `linear_values`, run just before the elimination reads them
    load_wait(E, 1);
    if (E->staged && apply_linear && lin.n && !E->h_vflag[8]) {
      // rows that keys alone cannot settle (a renaming collision, or no non-constant key left) take
      // their values from the host input now (hundreds of rows out of millions, typically); the rest
      // wait for their values
      const uint64_t unc_cap = std::max<uint64_t>(kUncMin, lin.n / kUncDiv);
      int *unc = A.get<int>("lin.unc", 1);
      uint32_t *unc_list = A.get<uint32_t>("lin.unc_list", unc_cap);
      lin_fixed = A.get<uint8_t>("lin.fixed", lin.n);
      HC(hipMemsetAsync(unc, 0, 4, st));
      HC(hipMemsetAsync(lin_fixed, 0, lin.n, st));
      kg1.run(st, 13 * E->lin.nnz + 20 * lin.n + 8, [&] {
        launch(st, k_lin_keyframes, lin.n, (const uint64_t *)E->lin.ptr, (const uint32_t *)E->lin.key, lin.n, lin,
               (const int32_t *)eq_rep, (const uint8_t *)ce_has, unc, unc_list, unc_cap);
      });
      int hu = 0;
      HC(hipMemcpyAsync(&hu, unc, 4, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
      keys_first = (uint64_t)hu <= unc_cap;
      if (keys_first && hu) {
        std::vector<uint32_t> rows(hu);
        HC(hipMemcpyAsync(rows.data(), unc_list, 4 * (uint64_t)hu, hipMemcpyDeviceToHost, st));
        HC(hipStreamSynchronize(st));
        const rs_lc &H = E->hin->linear;
        std::vector<uint64_t> hp(1, 0);
        std::vector<uint32_t> hk;
        std::vector<uint64_t> hv;
        for (uint32_t r : rows) {
          const uint64_t b = H.ptr[r], e = H.ptr[r + 1];
          hk.insert(hk.end(), H.col + b, H.col + e);
          hv.insert(hv.end(), H.val + 4 * b, H.val + 4 * e);
          hp.push_back(hk.size());
        }
        uint64_t *d_hp = A.get<uint64_t>("lin.fx_ptr", hp.size());
        uint32_t *d_hk = A.get<uint32_t>("lin.fx_key", std::max<size_t>(hk.size(), 1));
        Fe *d_hv = A.get<Fe>("lin.fx_val", std::max<size_t>(hk.size(), 1));
        uint32_t *d_rows = A.get<uint32_t>("lin.fx_rows", hu);
        h2d(E, d_hp, hp.data(), 8 * hp.size());
        h2d(E, d_hk, hk.data(), 4 * hk.size());
        h2d(E, d_hv, hv.data(), 8 * hv.size());
        h2d(E, d_rows, rows.data(), 4 * rows.size());
        launch(st, k_lin_fixrows, (uint64_t)hu, E->F, (const uint64_t *)d_hp, (const uint32_t *)d_hk, (const Fe *)d_hv,
               (const uint32_t *)d_rows, (uint64_t)hu, lin, (const int32_t *)eq_rep, (const uint8_t *)ce_has,
               (const Fe *)ce_val, lin_fixed);
      }
      if (g_prof_env && keys_first) fprintf(stderr, "[rs-prof] keys-first: %d rows settled from host values\n", hu);
    }
    if (!keys_first) {
      load_wait(E, 2);
      if (lin.n) {
        kg1.run(st, 72 * E->lin.nnz + 20 * lin.n + 8 + 77 * E->lin.nnz + 16 * lin.n, [&] {
          launch(st, k_make_ragged, lin.n, E->F, (const uint64_t *)E->lin.ptr, (const uint32_t *)E->lin.key, (const Fe *)E->lin.val,
                 lin.n, (uint64_t)1, lin.off, lin.len, lin.key, lin.val);
          launch(st, k_linear_frames12, lin.n, E->F, lin, (const int32_t *)eq_rep, (const uint8_t *)ce_has, (const Fe *)ce_val);
        });
      }
    }
    if (g_prof_env) fprintf(stderr, "[rs-prof] linear rows: %s\n", keys_first ? "keys first" : "keys + values");
    HC(hipStreamSynchronize(st));
    E->stats.eq_ms = now_ms() - T0;
  }
  // keys first: the linear rows' values, once the elimination is about to read them (the
  // elimination driver calls this through linear_round1)
  void linear_values() {
    load_wait(E, 2);
    kg1.run(st, 77 * E->lin.nnz + 20 * lin.n + 8, [&] {
      launch(st, k_lin_valframes, lin.n, E->F, (const uint64_t *)E->lin.ptr, (const uint32_t *)E->lin.key, (const Fe *)E->lin.val,
             lin.n, lin, (const int32_t *)eq_rep, (const uint8_t *)ce_has, (const Fe *)ce_val, (const uint8_t *)lin_fixed);
    });
  }

  // the ragged Montgomery copy of input block B on stream ms (kg[1])
  void mk_in(rs_engine::Blk &B, DRows &R, const char *nm, hipStream_t ms) {
    R.n = B.n;
    R.off = A.get<uint64_t>(std::string(nm) + ".off", R.n);
    R.len = A.get<uint32_t>(std::string(nm) + ".len", R.n);
    R.key = A.get<uint32_t>(std::string(nm) + ".key", B.nnz);
    R.val = A.get<Fe>(std::string(nm) + ".val", B.nnz);
    if (R.n)
      kg1.run(ms, 72 * B.nnz + 20 * R.n + 8, [&] {
        launch(ms, k_make_ragged, R.n, E->F, (const uint64_t *)B.ptr, (const uint32_t *)B.key, (const Fe *)B.val, R.n, (uint64_t)0,
               R.off, R.len, R.key, R.val);
      });
  }
  // the non-linear blocks are staged where the frames first need them: their upload (group 2)
  // overlaps the clustering and elimination
  void stage_nl() {
    if (nl_staged) return;
    load_wait(E, 3);
    // the conversion on the copy stream (in order after the blocks' upload and checks), beside what
    // the main stream still runs (the tail's finish): the frames wait for it there
    static const bool on_main = env_flag("RS_NLC_MAIN");
    hipStream_t cs = on_main ? st : E->stc;
    rs_engine::Blk *blk[3] = {&E->na, &E->nb, &E->nc};
    const char *nm[3] = {"nla", "nlb", "nlc"};
    for (int q = 0; q < 3; ++q) mk_in(*blk[q], nl_in[q], nm[q], cs);
    HC(hipEventRecord(E->ev_nlc, cs));
    HC(hipStreamWaitEvent(st, E->ev_nlc, 0));
    nl_staged = true;
  }
  // storage rows live in one growable heap of (key, value) entries, owned by the engine
  void heap_reserve(uint64_t need) {
    if (heap_top + need <= E->heap_cap && E->heap_k) return;
    // grows by a quarter (doubling left the 20 M-row circuit's heap at 12 GB for 6 GB of rows; eight
    // in-process ranks on one GPU did not fit)
    uint64_t ncap = std::max<uint64_t>(heap_top + need + (heap_top + need) / 16, E->heap_cap + E->heap_cap / 4);
    ncap = std::max<uint64_t>(ncap, 1 << 16);
    uint32_t *nk = nullptr;
    Fe *nv = nullptr;
    HC(hipStreamSynchronize(st));
    HC(hipMalloc((void **)&nk, 4 * ncap));
    HC(hipMalloc((void **)&nv, 32 * ncap));
    if (heap_top) {
      HC(hipMemcpyAsync(nk, E->heap_k, 4 * heap_top, hipMemcpyDeviceToDevice, st));
      HC(hipMemcpyAsync(nv, E->heap_v, 32 * heap_top, hipMemcpyDeviceToDevice, st));
      HC(hipStreamSynchronize(st));
    }
    if (E->snap_on) HC(hipStreamSynchronize(E->stc));  // the early gather reads the old heap
    if (E->heap_k) { HC(hipFree(E->heap_k)); HC(hipFree(E->heap_v)); }
    E->heap_k = heap_k = nk;
    E->heap_v = heap_v = nv;
    E->heap_cap = ncap;
  }

  // ======================= obtain_and_simplify_non_linear (non_linear_utils.rs:6-31): setup
  // Reads eq_rep, ce_has, ce_val, sub_of.  Leaves: the frames' arguments fr, the (empty) storage views
  // stor over the engine's heap (heap_top, heap_k, heap_v), the capacity columns cap with
  // their packed scan buffers, and the frames' byte and error words (d_bytes, d_fw_err).
  void setup_non_linear() {
    heap_top = 0;
    heap_k = E->heap_k;
    heap_v = E->heap_v;
    d_bytes = A.get<unsigned long long>("nl.bytes", 1);
    HC(hipMemsetAsync(d_bytes, 0, 8, st));
    d_fw_err = A.get<int>("fw.err", 1);  // k_frames_wave batch bounds (checked with the input checks)
    HC(hipMemsetAsync(d_fw_err, 0, 4, st));
    fr.F = E->F;
    fr.eq_rep = eq_rep;
    fr.ce_has = ce_has;
    fr.ce_val = ce_val;
    fr.sub_of = sub_of;
    for (int q = 0; q < 3; ++q) {
      stor[q].n = n_nl;
      stor[q].off = A.get<uint64_t>(part_name("st.", q, ".off"), n_nl);
      stor[q].len = A.get<uint32_t>(part_name("st.", q, ".len"), n_nl);
    }
    if (n_nl) {
      for (int q = 0; q < 3; ++q) cap[q] = A.get<uint64_t>(part_name("nl.cap", q, ""), n_nl);
      cap3 = A.get<U3>("nl.c3", n_nl); sc3 = A.get<U3>("nl.s3", n_nl);
    }
  }

  // The gathers of a snapshot read copies of the selected rows' views (ViewCopy, output.hpp): cp = src
  // with off / len in the buffers "<pre>{a,b,c}.off/.len", which vc hands to the selecting kernel.
  void snap_views(const DRows (&src)[3], const char *pre, DRows (&cp)[3], ViewCopy &vc) {
    for (int q = 0; q < 3; ++q) {
      cp[q] = src[q];
      cp[q].off = vc.off[q] = A.get<uint64_t>(part_name(pre, q, ".off"), src[q].n);
      cp[q].len = vc.len[q] = A.get<uint32_t>(part_name(pre, q, ".len"), src[q].n);
    }
  }
  // The common end of every snapshot.  Part q's n[q] new entries go behind its snap_e[q] earlier ones:
  // `gather(q, col, val, base)` issues their gather on the copy stream (inside kg[2].run) into the
  // device region (col, val), the part's event evs[q] is recorded, the D2H of its columns and values is
  // queued on the result stream's thread, and snap_e[q] advances; then ev_snap and RS_PROF's line.
  template <class G>
  void snap_tail(const uint64_t n[3], hipEvent_t *evs, const char *what, const char *when, G &&gather) {
    for (int q = 0; q < 3; ++q) {
      const uint64_t b = E->snap_e[q];
      const std::string xn = std::string("out.") + "abc"[q];
      uint32_t *col = A.get<uint32_t>(xn + ".xcol", 1);
      uint64_t *val = A.get<uint64_t>(xn + ".xval", 1);
      if (!n[q]) continue;
      gather(q, col, val, b);
      HC(hipEventRecord(evs[q], E->stc));  // a part's copies start once its own gather is done
      snap_push(E, {(uint32_t *)E->snap_host[2 * q] + b, col + b, 4 * n[q], evs[q]});
      snap_push(E, {(uint64_t *)E->snap_host[2 * q + 1] + 4 * b, val + 4 * b, 32 * n[q], evs[q]});
      E->snap_e[q] = b + n[q];
    }
    HC(hipEventRecord(E->ev_snap, E->stc));
    if (g_prof_env)
      fprintf(stderr, "[rs-prof] stream: %s %llu / %llu / %llu entries (%.1f MB)%s\n", what, (unsigned long long)n[0],
              (unsigned long long)n[1], (unsigned long long)n[2], 36e-6 * (n[0] + n[1] + n[2]), when);
  }
  // streamed result (output.hpp): the non-linear rows round 1's substitution has finished and left
  // non-linear (storage rows) are gathered to the early region and copied to the host on the copy
  // stream while the run goes on.  late: rows a second frames pass still has to do (nullptr: none).
  // hi_rows < n_nl: the first pass's first half only (snap_take_h2 takes the rest once it is done)
  void snap_take(const uint64_t *late, uint64_t hi_rows) {
    if (!E->stream_out || !n_nl) return;
    so_early = A.get<uint8_t>("so.early", n_nl);
    so_eoff = A.get<U3>("so.eoff", n_nl);
    U3 *elen = A.get<U3>("so.elen", n_nl);
    Comm *CM = E->comm.get();
    const bool shard = CM && CM->world > 1;
    // the gather reads copies of the selected rows' views: the second pass and later rounds re-point rows
    DRows cp[3];
    ViewCopy vc;
    snap_views(stor, "so.", cp, vc);
    launch(st, k_snap_flags, n_nl, stor[0], stor[1], stor[2], late, n_nl, shard ? E->nl_lo : (uint64_t)0, shard ? E->nl_hi : hi_rows, so_early, elen,
           vc);
    const U3 et = excl_scan_u3(E, elen, so_eoff, n_nl, "so");
    // single engine: the lconst rows so far (final as they enter the heap) go behind the C part
    E->lc_snap_n = shard ? 0 : lc.n;
    E->lc_snap_base = et.c;
    const uint64_t lc_e = shard ? 0 : lc.top;
    const uint64_t ev[3] = {et.a, et.b, et.c + lc_e};
    E->sh_full = false;
    if (shard) {  // every rank's share of each part gets the same capacity in the shared region
      for (int q = 0; q < 3; ++q) E->sh_cap[q] = CM->max_u64(std::max<uint64_t>(ev[q] + ev[q] / 4 + 65536, E->sh_cap[q]), st);
      E->sh_ent = CM->shared_host(0, sh_ent_bytes(E), st);
      if (!E->sh_ent) {  // every rank alike (shared_host agrees): no stream; each rank fetches the whole result
        if (g_prof_env) fprintf(stderr, "[rs-prof] no shared host memory: unstreamed per-rank result\n");
        E->stream_out = false;
        return;
      }
    }
    HC(hipEventRecord(E->ev_snap0, st));
    HC(hipStreamWaitEvent(E->stc, E->ev_snap0, 0));
    for (int q = 0; q < 3; ++q) {  // the regions: device (the head of the layout's arrays; the late rows follow) and host
      E->snap_e[q] = 0;
      E->snap_hint[q] = std::max(E->snap_hint[q], ev[q]);
      // room for the second snapshot's rows too (the largest early region so far, else a margin)
      // (a first half: room for the whole pass, scaled by rows)
      const uint64_t est = hi_rows < n_nl && hi_rows ? (uint64_t)((double)ev[q] * n_nl / hi_rows) : ev[q];
      const uint64_t cap = std::max<uint64_t>(est + std::max<uint64_t>(est / 4, 1 << 16), E->snap_hint[q]);
      const std::string xn = std::string("out.") + "abc"[q];
      (void)A.get<uint32_t>(xn + ".xcol", cap);
      (void)A.get<uint64_t>(xn + ".xval", 4 * cap);
      E->snap_cap[q] = cap;
      E->snap_host[2 * q] = shard ? (void *)(sh_col(E, q) + CM->rank * E->sh_cap[q]) : pin_get(E, kPinCol + q, 4 * cap);
      E->snap_host[2 * q + 1] = shard ? (void *)(sh_val(E, q) + 4 * CM->rank * E->sh_cap[q]) : pin_get(E, kPinVal + q, 32 * cap);
    }
    // kg[2]'s algorithmic bytes: 72 an entry (key + value read, canonical key + value written) and
    // what a row's selection reads (its flag; its extent when selected)
    snap_tail(ev, E->ev_snapq, "early region", late ? " after the first pass" : "", [&](int q, uint32_t *col, uint64_t *val, uint64_t) {
      E->kg[2].run(E->stc, 13 * n_nl + 72 * ev[q], [&] {
        launch(E->stc, k_snap_gather, n_nl, E->F, cp[q], (const uint8_t *)so_early, (const U3 *)so_eoff, q, n_nl, col, val,
               (const uint64_t *)nullptr, (uint64_t)0);
      });
      if (q == 2 && lc_e) {
        const DRows lcv = lc.view(A);
        E->kg[2].run(E->stc, 72 * lc_e, [&] {
          launch(E->stc, k_lc_snap, lc_e, E->F, (const uint32_t *)lcv.key, (const Fe *)lcv.val, lc_e, col + et.c, val + 4 * et.c);
        });
      }
    });
    E->snap_on = true;
  }
  // The second snapshot (single engine): the rows of the second frames pass -- those touching the head
  // clusters -- that stayed storage rows go behind the first snapshot's, when they fit the regions
  // sized at the first (else they stay late), so they stream during the later rounds too.
  void snap_take2() {
    if (!E->snap_on || !nl_late || !n_late || (E->comm && E->comm->world > 1)) return;
    HC(hipStreamWaitEvent(st, E->ev_snap, 0));  // the first snapshot's gathers read the flags rewritten here
    // (over the list of the pass's rows, nl_lids -- ascending, so the rows land in the same order as a
    // scan over every non-linear row would put them)
    U3 *elen = A.get<U3>("so.elen2", n_late), *eoff2 = A.get<U3>("so.eoff2", n_late);
    DRows cp[3];  // copies of the selected rows' views (the rounds re-point rows)
    ViewCopy vc;
    snap_views(stor, "so2.", cp, vc);
    launch(st, k_snap_lens2_l, n_late, stor[0], stor[1], stor[2], (const uint32_t *)nl_lids, n_late, elen, vc);
    const U3 et = excl_scan_u3(E, elen, eoff2, n_late, "so2");
    const uint64_t e2[3] = {et.a, et.b, et.c};
    for (int q = 0; q < 3; ++q) E->snap_hint[q] = std::max(E->snap_hint[q], E->snap_e[q] + e2[q]);
    for (int q = 0; q < 3; ++q)
      if (E->snap_e[q] + e2[q] > E->snap_cap[q]) return;  // no room this time (the hint grows the next run's)
    launch(st, k_snap_mark2_l, n_late, (const uint32_t *)nl_lids, (const U3 *)elen, (const U3 *)eoff2,
           U3{E->snap_e[0], E->snap_e[1], E->snap_e[2]}, n_late, so_early, so_eoff);
    HC(hipEventRecord(E->ev_snap0, st));
    HC(hipStreamWaitEvent(E->stc, E->ev_snap0, 0));
    snap_tail(e2, E->ev_snapq + 3, "second snapshot", "", [&](int q, uint32_t *col, uint64_t *val, uint64_t) {
      E->kg[2].run(E->stc, 28 * n_late + 72 * e2[q], [&] {
        launch(E->stc, k_snap_gather_l, n_late, E->F, cp[q], (const uint32_t *)nl_lids, (const U3 *)elen, (const U3 *)so_eoff, q, n_late,
               col, val);
      });
    });
  }
  // The first pass's second half (single engine): its rows [h, n_nl) that are done and stayed storage
  // rows go behind the first half's in the regions sized at the first snapshot, when they fit (else
  // they stay late and the capacity hint grows).
  void snap_take_h2(uint64_t h) {
    if (!E->snap_on || (E->comm && E->comm->world > 1)) return;
    HC(hipStreamWaitEvent(st, E->ev_snap, 0));  // the first half's gathers read the flags rewritten here
    U3 *elen = A.get<U3>("so.elenh", n_nl), *eoffh = A.get<U3>("so.eoffh", n_nl);
    DRows cp[3];  // copies of the selected rows' views (the second pass and the rounds re-point rows)
    ViewCopy vc;
    snap_views(stor, "soh.", cp, vc);
    launch(st, k_snap_lens_rng, n_nl, stor[0], stor[1], stor[2], (const uint64_t *)nl_late, h, n_nl, n_nl, elen, vc);
    const U3 et = excl_scan_u3(E, elen, eoffh, n_nl, "soh");
    const uint64_t e2[3] = {et.a, et.b, et.c};
    for (int q = 0; q < 3; ++q) E->snap_hint[q] = std::max(E->snap_hint[q], E->snap_e[q] + e2[q]);
    for (int q = 0; q < 3; ++q)
      if (E->snap_e[q] + e2[q] > E->snap_cap[q]) return;
    launch(st, k_snap_mark_sel, n_nl, (const U3 *)elen, (const U3 *)eoffh, U3{E->snap_e[0], E->snap_e[1], E->snap_e[2]}, n_nl,
           so_early, so_eoff);
    HC(hipEventRecord(E->ev_snap0, st));
    HC(hipStreamWaitEvent(E->stc, E->ev_snap0, 0));
    snap_tail(e2, E->ev_snaph, "the first pass's second half", "", [&](int q, uint32_t *col, uint64_t *val, uint64_t) {
      E->kg[2].run(E->stc, 13 * (n_nl - h) + 72 * e2[q], [&] {
        launch(E->stc, k_snap_gather, n_nl - h, E->F, cp[q], (const uint8_t *)so_early, (const U3 *)so_eoff, q, n_nl, col, val,
               (const uint64_t *)nullptr, h);
      });
    });
  }
  // one pass of the frames over the non-linear rows ids[0, n) (phase: see NLArgs); the fill's
  // kernel time is read from (e0, e1) once the caller synchronises (nl_ms).
  // split < n (phase 1): the frames of rows [0, split), `between` (the first half's snapshot), then the
  // rest; the kernel time excludes what runs between.  Sets fh_split (read by nl_ms) and n_late.
  void nl_phase(int phase, const uint32_t *ids, uint64_t n, hipEvent_t e0, hipEvent_t e1, uint64_t split = ~0ull,
                const std::function<void()> &between = {}) {
    stage_nl();
    NLArgs a{};
    a.fr = fr;
    a.a = nl_in[0]; a.b = nl_in[1]; a.c = nl_in[2];
    a.cap_a = cap[0]; a.cap_b = cap[1]; a.cap_c = cap[2];
    a.bytes = d_bytes;
    a.ids = ids;
    a.n = n;
    a.phase = phase;
    a.hmark = hmark;
    a.late = nl_late;
    launch(st, k_nl_count, n, a);
    const bool lists = phase == 1 && n_nl;
    if (lists) {  // the skipped rows, listed for the second pass (their count comes back with the heap's)
      dev_scan_u64(E, nl_late, nl_lpos, n_nl, st, "nll");
      launch(st, k_scatter_ids, n_nl, (const uint64_t *)nl_late, (const uint64_t *)nl_lpos, n_nl, nl_lids);
    }
    launch(st, k_pack3, n, (const uint64_t *)cap[0], (const uint64_t *)cap[1], (const uint64_t *)cap[2], n, cap3);
    const U3 t3 = lists ? excl_scan_u3(E, cap3, sc3, n, "nl", nl_late + n_nl - 1, nl_lpos + n_nl - 1, &n_late)
                        : excl_scan_u3(E, cap3, sc3, n, "nl");
    if (g_prof_env) fprintf(stderr, "[rs-prof] nl phase %d: %llu rows, %llu heap entries\n", phase, (unsigned long long)n,
                            (unsigned long long)(t3.a + t3.b + t3.c));
    heap_reserve(t3.a + t3.b + t3.c);
    launch(st, k_set_offsets_u3, n, (const U3 *)sc3, heap_top, heap_top + t3.a, heap_top + t3.a + t3.b, n, stor[0].off, stor[1].off,
           stor[2].off, phase == 1 ? (const U3 *)cap3 : nullptr, ids);
    heap_top += t3.a + t3.b + t3.c;
    for (DRows &R : stor) { R.key = heap_k; R.val = heap_v; }
    a.oa = stor[0]; a.ob = stor[1]; a.oc = stor[2];
    // whole waves on batches of rows (frames_wave.hpp); the rows too large for a batch, one lane each
    FrameWaveArgs w{};
    w.fr = fr;
    for (int q = 0; q < 3; ++q) { w.in[q] = nl_in[q]; w.out[q] = stor[q]; w.cap[q] = cap[q]; }
    w.ids = ids;
    w.n = n;
    w.late = phase == 1 ? nl_late : nullptr;
    w.big = A.get<uint32_t>(phase == 1 ? "nl.big1" : "nl.big2", n);
    w.n_big = A.get<unsigned>(phase == 1 ? "nl.nbig1" : "nl.nbig2", 1);
    w.err = d_fw_err;
    w.bytes = d_bytes;
    HC(hipMemsetAsync(w.n_big, 0, 4, st));
#ifdef RS_FWCLK
    w.clk = A.get<unsigned long long>(phase == 1 ? "fw.clk1" : "fw.clk2", 32 + 8 * 64);
    HC(hipMemsetAsync(w.clk, 0, 8 * (32 + 8 * 64), st));
#endif
    a.xlist = w.big;
    a.n_xlist = w.n_big;
    HC(hipEventRecord(e0, st));
    fh_split = split < n;
    if (fh_split) {
      w.n = split;
      launch_capped(st, k_frames_wave<0>, split, kFwBlocks, w);
      launch(st, k_nl_fill, n, a);  // the rows over a batch listed so far
      HC(hipEventRecord(E->ev_fh[0], st));
      between();
      HC(hipMemsetAsync(w.n_big, 0, 4, st));
      HC(hipEventRecord(E->ev_fh[1], st));
      w.x0 = split;
      w.n = n;
      launch_capped(st, k_frames_wave<0>, n - split, kFwBlocks, w);
    } else {
      launch_capped(st, k_frames_wave<0>, n, kFwBlocks, w);
    }
    launch(st, k_nl_fill, n, a);  // a grid for every row: the list may be long, idle lanes leave at once
    HC(hipEventRecord(e1, st));
    if (g_prof_env) {
      unsigned nb = 0;
      HC(hipMemcpyAsync(&nb, w.n_big, 4, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
      fprintf(stderr, "[rs-prof] nl phase %d: %u rows over a wave batch\n", phase, nb);
      if (w.clk) {
        unsigned long long c[32 + 8 * 64];
        HC(hipMemcpy(c, w.clk, sizeof c, hipMemcpyDeviceToHost));
        fprintf(stderr, "[rs-prof] frames clocks (Mcycles summed over waves): groups %.1f entries %.1f terms %.1f rank %.1f "
                "heads %.1f emit %.1f rows %.1f plan %.1f | batches %llu, wave total %.1f over %llu waves\n",
                c[0] / 1e6, c[1] / 1e6, c[2] / 1e6, c[3] / 1e6, c[4] / 1e6, c[5] / 1e6, c[6] / 1e6, c[7] / 1e6, c[8],
                c[9] / 1e6, c[10]);
        fprintf(stderr, "[rs-prof] frames fallbacks: A const %llu, B const %llu | emit: loads %.1f values %.1f sync %.1f stores %.1f\n",
                c[12], c[13], c[16] / 1e6, c[17] / 1e6, c[18] / 1e6, c[19] / 1e6);
      }
    }
    E->stats.apply_kernel_launches++;
  }
  // the kernel time of the last nl_phase into the stats (waits for e1)
  void nl_ms(hipEvent_t e0, hipEvent_t e1) {
    float ms = 0;
    HC(hipEventSynchronize(e1));
    if (fh_split) {  // the two halves, without the snapshot between them
      float m2 = 0;
      HC(hipEventElapsedTime(&ms, e0, E->ev_fh[0]));
      HC(hipEventElapsedTime(&m2, E->ev_fh[1], e1));
      ms += m2;
      fh_split = false;
    } else {
      HC(hipEventElapsedTime(&ms, e0, e1));
    }
    E->stats.apply_kernel_ms += ms;
  }
  // rows that touch none of the largest clusters go through the frames while those clusters are
  // still being eliminated (sharded: after the exchange of the clusters other than the head, which every
  // rank eliminates itself).  Called by the elimination driver through linear_round1; sets hmark and
  // the late-row lists, takes the first snapshot(s), and sets nl_split for non_linear_frames.
  void head_overlap(const uint32_t *ids, uint64_t n_head, const ElimArgs &ea) {
    hmark = A.get<uint8_t>("nl.hmark", E->S);
    nl_late = A.get<uint64_t>("nl.late", n_nl);
    nl_lpos = A.get<uint64_t>("nl.lpos", n_nl);
    nl_lids = A.get<uint32_t>("nl.lids", n_nl);
    HC(hipMemsetAsync(hmark, 0, E->S, st));
    hipLaunchKernelGGL(k_mark_head_keys, dim3(16, (unsigned)n_head), dim3(256), 0, st, ea.rows, (const uint32_t *)ea.perm,
                       (const uint64_t *)ea.cl_off, ids, hmark);
    HC(hipGetLastError());
    fr.h_off = ea.h_off; fr.h_len = ea.h_len; fr.pk = ea.pk; fr.pv = ea.pv;
    // the first pass in two halves with a snapshot after each (single engine, streamed): the result
    // stream starts after half the pass
    const bool halves = E->stream_out && !(E->comm && E->comm->world > 1) &&
                        n_nl >= env_u64("RS_HALVES_MIN", 1ull << 20, 0, UINT64_MAX) && !env_flag("RS_NO_HALVES");
    const double frac = env_f64("RS_HALF_FRAC", 0.5, 0.0, 1.0);
    const uint64_t h = halves ? std::max<uint64_t>(1, std::min<uint64_t>(n_nl - 1, (uint64_t)(n_nl * frac))) : n_nl;
    nl_phase(1, nullptr, n_nl, E->ev[kEvNl0], E->ev[kEvNl1], h, [&] { snap_take(nl_late, h); });
    if (!halves) snap_take(nl_late, n_nl);
    else snap_take_h2(h);
    nl_split = true;
  }

  // ======================= linear round 1 (:544-578)
  // Reads lin (keys first: its values follow through linear_values), the bitmaps, and -- through
  // head_overlap -- everything setup_non_linear left.  Leaves: the round's substitutions (eo, pool P,
  // sub_of), its leftovers in lc; with --O1 the linear rows in lc as they are.
  void linear_round1() {
    P = get_pool(E, 1 << 20);
    const HeadOverlap overlap = [this](const uint32_t *ids, uint64_t n_head, const ElimArgs &ea) { head_overlap(ids, n_head, ea); };
    const std::function<void()> values = [this] { linear_values(); };
    if (apply_linear) {
      // sharded: only the relevant substitutions' right-hand sides travel (the log needs them all)
      uint8_t *relevant = nullptr;
      if (E->comm && E->comm->world > 1 && !E->log_on) {
        relevant = A.get<uint8_t>("x.relevant", S);
        HC(hipMemsetAsync(relevant, 0, S, st));
        if (n_nl) {
          stage_nl();
          for (const DRows &R : nl_in)
            launch(st, k_mark_relevant, R.n, R,(const int32_t *)eq_rep, (const uint8_t *)ce_has, relevant);
        }
      }
      if (E->comm && E->comm->world > 1) load_order_collectives(E);
      run_linear_simplification(E, lin, fl->use_old_heuristics, eo, P, d_err, d_forb, sub_of, d_deleted,
                                n_nl ? &overlap : nullptr, keys_first ? &values : nullptr, relevant);
      if (E->log_on) log_linear_round(E, eo, P);
      collect_leftovers(E, eo, P, lc);
      E->stats.rounds++;
    } else {
      // --O1: the linear rows join lconst as they are after the eq / constant frames (:575-577)
      if (!keys_first) lc.append(E, lin, nullptr, lin.n);
      else throw RsError(RS_E_INTERNAL, "--O1 with keys-first linear rows");
    }
  }

  // ======================= obtain_and_simplify_non_linear (non_linear_utils.rs:6-31)
  // Reads round 1's substitutions (P, sub_of through fr) and, when head_overlap ran (nl_split), the
  // late-row list (nl_lids, n_late).  Leaves: every non-linear row through the frames (stor),
  // the split into storage rows (st_ids, n_st; views sv) and rows turned linear (wl_ids,
  // n_wl; the C-only view lv), both in DFS order, and the non-linear signal map's key set (nlmap, :599-612).
  void non_linear_frames() {
    double Ts = now_ms();
    fr.h_off = A.get<uint64_t>("el.h_off", 1);
    fr.h_len = A.get<uint32_t>("el.h_len", 1);
    fr.pk = P.pk;
    fr.pv = P.pv;
    if (n_nl) {
      if (nl_split) nl_ms(E->ev[kEvNl0], E->ev[kEvNl1]);
      if (!nl_split) {
        nl_phase(0, nullptr, n_nl, E->ev[kEvFill0], E->ev[kEvFill1]);
        snap_take(nullptr, n_nl);
        nl_ms(E->ev[kEvFill0], E->ev[kEvFill1]);
      } else if (n_late) {
        nl_phase(2, nl_lids, n_late, E->ev[kEvFill0], E->ev[kEvFill1]);
        snap_take2();
        nl_ms(E->ev[kEvFill0], E->ev[kEvFill1]);
      }
    }
    unsigned long long bytes = 0;
    HC(hipMemcpyAsync(&bytes, d_bytes, 8, hipMemcpyDeviceToHost, st));
    // split: storage (still non-linear) vs with_linear, both in DFS order
    st_ids = A.get<uint32_t>("st.ids", n_nl);
    wl_ids = A.get<uint32_t>("wl.ids", n_nl);
    uint64_t *h_wl = (uint64_t *)pin_get(E, kPinRead, kPinRb);
    if (n_nl) {  // one scan (of the rows turned linear) places both lists; its total comes back with `bytes`
      uint64_t *fl_lin = A.get<uint64_t>("fl.lin", n_nl), *p_lin = A.get<uint64_t>("fl.plin", n_nl);
      uint64_t *d_wl = A.get<uint64_t>("fl.tot", 1);
      launch(st, k_flag_lin, n_nl, (const uint32_t *)stor[0].len, (const uint32_t *)stor[1].len, n_nl, fl_lin);
      dev_scan_u64(E, fl_lin, p_lin, n_nl, st, "fl");
      launch(st, k_scan_total_u64, 1, (const uint64_t *)fl_lin, (const uint64_t *)p_lin, n_nl, d_wl);
      launch(st, k_split_ids, n_nl, (const uint64_t *)fl_lin, (const uint64_t *)p_lin, n_nl, wl_ids, st_ids);
      HC(hipMemcpyAsync(h_wl, d_wl, 8, hipMemcpyDeviceToHost, st));
    }
    HC(hipStreamSynchronize(st));
    if (n_nl) {
      n_wl = h_wl[0];
      if (n_wl > n_nl) throw RsError(RS_E_INTERNAL, "non-linear split: row counts out of range");
      n_st = n_nl - n_wl;
    }
    E->stats.apply_bytes += bytes;
    if (no_rounds > 0) no_rounds--;

    // storage view (compacted) and the non-linear signal map bitmap (:599-612)
    for (int q = 0; q < 3; ++q) {
      sv[q].n = n_st;
      sv[q].key = heap_k;
      sv[q].val = heap_v;
      sv[q].off = A.get<uint64_t>(part_name("sv.", q, ".off"), n_st);
      sv[q].len = A.get<uint32_t>(part_name("sv.", q, ".len"), n_st);
    }
    // the current linear list: a C-only view
    lv.n = n_wl;
    lv.key = heap_k;
    lv.val = heap_v;
    lv.off = A.get<uint64_t>("lv.off", n_wl);
    lv.len = A.get<uint32_t>("lv.len", n_wl);
    if (n_st + n_wl)
      launch(st, k_view_rows4, n_st + n_wl, stor[0], stor[1], stor[2], (const uint32_t *)st_ids, n_st, (const uint32_t *)wl_ids, n_wl,
             sv[0], sv[1], sv[2], lv);
    nlmap = A.get<uint8_t>("nlmap", S);
    HC(hipMemsetAsync(nlmap, 0, S, st));
    if (n_st) launch(st, k_mark_keys3, n_st, sv[0], sv[1], sv[2], n_st, nlmap);
    HC(hipStreamSynchronize(st));
    E->stats.subst_ms += now_ms() - Ts;
    E->stats.nl_ms += now_ms() - Ts;
  }

  // A round's snapshot (single engine): the storage rows the round rewrote that stay storage rows go
  // behind the early region right away -- final unless a later round rewrites them again (dirty once
  // more: late at the end) -- so a round that rewrites most rows (the templated circuit's round 2)
  // streams them while the run goes on instead of after it.  Skipped when the regions sized at the first
  // snapshot cannot take them (the capacity hint grows for the next run).
  void snap_round(const uint8_t *touched, const int32_t *turn) {
    if (!so_dirty || !n_st || (E->comm && E->comm->world > 1)) return;
    // the earlier snapshots' gathers read the early flags / offsets this one rewrites, and its own buffers
    HC(hipStreamWaitEvent(st, E->ev_snap, 0));
    U3 *elen = A.get<U3>("so.rlen", n_st), *eoff3 = A.get<U3>("so.roff", n_st);
    DRows cp[3];  // copies of the selected rows' views (a later round re-points rows)
    ViewCopy vc;
    snap_views(sv, "sor.", cp, vc);
    launch(st, k_snap_lens_round, n_st, sv[0], sv[1], sv[2], touched, turn, (const uint32_t *)st_ids, (const uint8_t *)so_early, n_st, elen, vc);
    const U3 et = excl_scan_u3(E, elen, eoff3, n_st, "sor");
    const uint64_t e3[3] = {et.a, et.b, et.c};
    if (!(e3[0] | e3[1] | e3[2])) return;
    for (int q = 0; q < 3; ++q) E->snap_hint[q] = std::max(E->snap_hint[q], E->snap_e[q] + e3[q]);
    for (int q = 0; q < 3; ++q)
      if (E->snap_e[q] + e3[q] > E->snap_cap[q]) return;
    launch(st, k_snap_mark_round, n_st, (const uint32_t *)st_ids, (const U3 *)elen, (const U3 *)eoff3,
           U3{E->snap_e[0], E->snap_e[1], E->snap_e[2]}, n_st, so_early, so_eoff, so_dirty);
    // the previous snapshot's gathers still read their view copies and elen / offsets (stc is in order)
    HC(hipEventRecord(E->ev_snap0, st));
    HC(hipStreamWaitEvent(E->stc, E->ev_snap0, 0));
    snap_tail(e3, E->ev_snapq + 3, "round snapshot", "", [&](int q, uint32_t *col, uint64_t *val, uint64_t b) {
      E->kg[2].run(E->stc, 24 * n_st + 72 * e3[q], [&] {
        launch(E->stc, k_snap_gather_st, n_st, E->F, cp[q], (const U3 *)elen, (const U3 *)eoff3, b, q, n_st, col, val);
      });
    });
  }

  // ======================= rounds >= 2 (:613-646)
  // Reads the storage views sv, the linear list lv, nlmap, P, and the streamed-output
  // state (so_early).  Each round_once eliminates over lv, applies the substitutions to the storage
  // rows (apply_substitution_to_map, :345-396) and leaves the next lv.  Leaves: sv, lv and
  // nlmap final, so_dirty (the rows a round rewrote: late at the end), the rounds' leftovers in lc.
  void rounds() {
    apply_round = apply_linear && no_rounds > 0 && n_wl > 0;
    // streamed result: rows a later round touches are taken from the late region
    if (so_early) {
      so_dirty = A.get<uint8_t>("so.dirty", n_st ? n_st : 1);
      if (n_st) HC(hipMemsetAsync(so_dirty, 0, n_st, st));
    }
    if (env_flag("RS_DEBUG")) {
      HC(hipStreamSynchronize(st));
      fprintf(stderr, "[rs-debug] heap %p cap %llu top %llu n_st %llu n_wl %llu\n", (void *)heap_k,
              (unsigned long long)E->heap_cap, (unsigned long long)heap_top, (unsigned long long)n_st, (unsigned long long)n_wl);
      for (uint64_t r = 0; r < std::min<uint64_t>(n_st, 3); ++r) {
        uint64_t o = 0; uint32_t l = 0;
        HC(hipMemcpy(&o, sv[2].off + r, 8, hipMemcpyDeviceToHost));
        HC(hipMemcpy(&l, sv[2].len + r, 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> kk; std::vector<Fe> vv;
        d2h_row(E, sv[2], r, kk, vv);
        fprintf(stderr, "[rs-debug]  st %llu C off %llu len %u:", (unsigned long long)r, (unsigned long long)o, l);
        for (size_t i = 0; i < kk.size(); ++i) fprintf(stderr, " %u:%llu", kk[i], (unsigned long long)ffrom_mont(E->F, vv[i]).l[0]);
        fprintf(stderr, "\n");
      }
    }
    if (apply_round) {
      // the non-linear signal map, kept on the host only for the signals a round substitutes:
      // initial lists (round-1 storage rows, ascending ids; built on the GPU on demand) + appends
      double Tm = now_ms();
      for (int q = 0; q < 3; ++q) {  // snapshot of the round-1 storage rows
        m0[q] = sv[q];
        m0[q].off = A.get<uint64_t>(part_name("m0.", q, ".off"), n_st);
        m0[q].len = A.get<uint32_t>(part_name("m0.", q, ".len"), n_st);
      }
      if (n_st)
        for (int q = 0; q < 3; ++q) {
          HC(hipMemcpyAsync(m0[q].off, sv[q].off, 8 * n_st, hipMemcpyDeviceToDevice, st));
          HC(hipMemcpyAsync(m0[q].len, sv[q].len, 4 * n_st, hipMemcpyDeviceToDevice, st));
        }
      // the appended lists of the non-linear signal map, lazily (maplists.hpp: ML)
      qflag = A.get<uint8_t>("m.qflag", S);
      HC(hipMemsetAsync(qflag, 0, S, st));
      E->stats.subst_ms += now_ms() - Tm;
      E->stats.map_ms += now_ms() - Tm;
      rank_of = A.get<int32_t>("rank_of", S);
      HC(hipMemsetAsync(rank_of, 0xff, 4 * S, st));
      r_sub_of = A.get<int32_t>("r.sub_of", S);
      HC(hipMemsetAsync(r_sub_of, 0xff, 4 * S, st));
      while (apply_round) round_once();
    }
  }
  // the initial lists of the non-linear signal map (build_non_linear_signal_map, :327-343) of the
  // signals not queried before: (signal, row) pairs of the round-1 storage rows m0
  void query_initial(const std::vector<uint32_t> &sigs) {
    auto &minit = ML.minit;  // initial lists, queried signals only
    std::vector<uint32_t> q;
    for (uint32_t s : sigs)
      if (!minit.count(s)) { minit[s]; q.push_back(s); }
    if (q.empty() || n_st == 0) return;
    uint32_t *d_q = A.get<uint32_t>("m.q", q.size());
    h2d(E, d_q, q.data(), 4 * q.size());
    launch(st, k_mark_list, q.size(), (const uint32_t *)d_q, (uint64_t)q.size(), qflag);
    unsigned long long *d_cnt = A.get<unsigned long long>("m.cnt", 1);
    uint64_t cap = std::max<uint64_t>(4 * q.size(), 1 << 16);
    for (;;) {
      uint64_t *d_pairs = A.get<uint64_t>("m.pairs", cap);
      HC(hipMemsetAsync(d_cnt, 0, 8, st));
      for (DRows &R : m0) { R.key = heap_k; R.val = heap_v; }
      launch(st, k_emit_pairs, n_st, m0[0], m0[1], m0[2], (const uint8_t *)qflag, d_pairs, d_cnt, cap);
      unsigned long long cnt = 0;
      HC(hipMemcpyAsync(&cnt, d_cnt, 8, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
      if (cnt > cap) { cap = cnt; continue; }
      std::vector<uint64_t> pairs(cnt);
      if (cnt) {
        HC(hipMemcpyAsync(pairs.data(), d_pairs, 8 * cnt, hipMemcpyDeviceToHost, st));
        HC(hipStreamSynchronize(st));
      }
      std::sort(pairs.begin(), pairs.end());
      for (uint64_t x : pairs) minit[(uint32_t)(x >> 32)].push_back((uint32_t)x);
      break;
    }
    launch(st, k_unmark_list, q.size(), (const uint32_t *)d_q, (uint64_t)q.size(), qflag);
  }
  // the host copy of the round's ordered `from` list, fetched on demand
  void need_usig() {
    if (usig.size() == nU) return;
    usig.resize(nU);
    HC(hipMemcpyAsync(usig.data(), d_us, 4 * nU, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
  }

  // One round of rounds >= 2 (the body of :613-646's loop): linear_simplification over lv, the round's
  // leftovers into lc, its substitutions ordered (round_order) and applied to the storage rows
  // (round_apply), the map appends (:369-377), and the next linear list.  Sets apply_round.
  void round_once() {
    er = ElimOut{};
    MK = Marks{};
    nU = 0;
    usig.clear();
    turned.clear();
    // linear_simplification over the current list
    HC(hipMemsetAsync(r_sub_of, 0xff, 4 * S, st));
    run_linear_simplification(E, lv, fl->use_old_heuristics, er, P, d_err, d_forb, r_sub_of, d_deleted, nullptr, nullptr,
                              E->comm && E->comm->world > 1 && !E->log_on ? nlmap : nullptr);
    if (E->log_on) log_linear_round(E, er, P);
    E->stats.rounds++;
    MK.st = st;
    MK.mark("start");
    collect_leftovers(E, er, P, lc);
    MK.mark("leftovers");
    const double Tr = now_ms();
    round_order();
    MK.mark("order");
    if (n_st && nU) round_apply();
    MK.mark("appends");
    const uint64_t nn = round_next();
    MK.mark("next");
    MK.dump();
    if (g_prof_env) fprintf(stderr, "[rs-prof] round: nU %llu n_st %llu next %llu\n", (unsigned long long)nU, (unsigned long long)n_st, (unsigned long long)nn);
    E->stats.subst_ms += now_ms() - Tr;
    E->stats.rounds_ms += now_ms() - Tr;
    if (no_rounds > 0) no_rounds--;
    apply_round = nn > 0 && no_rounds > 0;
    // rows that turned linear and came out empty (A and C cancelled) are still the reference's next
    // list (:380-394 take linear_id as it is), so its loop makes one more round, over nothing.  Nothing
    // to run here, but the round counts -- as round 2 does after a first round that left only such rows
    if (nn == 0 && !turned.empty() && no_rounds > 0) {
      E->stats.rounds++;
      no_rounds--;
    }
  }
  // ordered substitutions of the round: cluster order, ascending `from` -- one sort of the
  // (cluster, from) keys of the valid slots on the device; the host fetches the list only when
  // a row turned linear or another round follows.  Reads er; sets nU, d_us, d_uoff, d_ulen and the
  // dense signal -> rank index rank_of (read by round_apply, round_next and need_usig).
  void round_order() {
    const uint64_t n_slots = er.n_slots;
    d_us = A.get<uint32_t>("r.us", 1);
    uint32_t *d_U = A.get<uint32_t>("r.U", 1);
    d_ulen = A.get<uint32_t>("r.ulen", 1);
    d_uoff = A.get<uint64_t>("r.uoff", 1);
    if (n_slots) {
      uint64_t *vf = A.get<uint64_t>("r.vf", n_slots), *vp = A.get<uint64_t>("r.vp", n_slots);
      launch(st, k_sub_valid, n_slots, (const uint32_t *)A.get<uint32_t>("cl.cid", 1), (const uint64_t *)A.get<uint64_t>("el.cl", 1),
             (const uint32_t *)A.get<uint32_t>("el.n_sub", 1), n_slots, vf);
      nU = excl_scan_u64(E, vf, vp, n_slots, "vf");
      if (nU) {
        uint64_t *uk = A.get<uint64_t>("r.uk", nU), *uk2 = A.get<uint64_t>("r.uk2", nU);
        uint32_t *uv = A.get<uint32_t>("r.uv", nU);
        d_U = A.get<uint32_t>("r.U", nU);
        d_us = A.get<uint32_t>("r.us", nU);
        d_uoff = A.get<uint64_t>("r.uoff", nU);
        d_ulen = A.get<uint32_t>("r.ulen", nU);
        launch(st, k_sub_keys, n_slots, (const uint32_t *)A.get<uint32_t>("cl.cid", 1), (const uint64_t *)vf,
               (const uint64_t *)vp, (const uint32_t *)A.get<uint32_t>("el.h_sig", 1), n_slots, uk, uv);
        int cbits = 1;
        while (cbits < 32 && (1ull << cbits) <= er.n_clusters) ++cbits;
        sort_pairs(E, (const uint64_t *)uk, uk2, (const uint32_t *)uv, d_U, nU, 32 + cbits, "us");
        launch(st, k_sub_info, nU, (const uint64_t *)uk2, (const uint32_t *)d_U, (const uint64_t *)A.get<uint64_t>("el.h_off", 1),
               (const uint32_t *)A.get<uint32_t>("el.h_len", 1), nU, d_us, d_uoff, d_ulen, rank_of);
      }
    }
  }
  // apply the round's substitutions to every storage row (apply_substitution_to_map, :345-396).
  // Reads sv, the round's order, P.  Leaves the rewritten rows committed to sv
  // (heap_top advanced), so_dirty and the round's snapshot (snap_round), and `turned`: the rows that
  // turned linear, in the order the reference's map walk meets them.
  void round_apply() {
    RoundArgs ra{};
    ra.F = E->F;
    ra.a = sv[0]; ra.b = sv[1]; ra.c = sv[2];
    uint64_t *rcap[3];  // the round's capacity columns
    for (int q = 0; q < 3; ++q) rcap[q] = A.get<uint64_t>(part_name("r.cap", q, ""), n_st);
    ra.cap_a = rcap[0]; ra.cap_b = rcap[1]; ra.cap_c = rcap[2];
    ra.sub_of = r_sub_of;
    ra.rank_of = rank_of;
    ra.h_off = A.get<uint64_t>("el.h_off", 1);
    ra.h_len = A.get<uint32_t>("el.h_len", 1);
    ra.pk = P.pk;
    ra.pv = P.pv;
    ra.turn = A.get<int32_t>("r.turn", n_st);
    ra.touched = A.get<uint8_t>("r.touched", n_st);
    launch(st, k_round_count, n_st, ra);
    U3 *rcap3 = A.get<U3>("r.c3", n_st), *rsc3 = A.get<U3>("r.s3", n_st);
    launch(st, k_pack3, n_st, (const uint64_t *)rcap[0], (const uint64_t *)rcap[1], (const uint64_t *)rcap[2], n_st, rcap3);
    // the touched rows' flags and their scan go along: their count comes back with the capacities' totals
    uint64_t *tfl = A.get<uint64_t>("r.tfl", n_st), *tfp = A.get<uint64_t>("r.tfp", n_st);
    launch(st, k_touch_flags, n_st, (const uint64_t *)rcap[2], n_st, tfl);
    dev_scan_u64(E, tfl, tfp, n_st, st, "tfl");
    const U3 q3 = n_st ? excl_scan_u3(E, rcap3, rsc3, n_st, "r", tfl + n_st - 1, tfp + n_st - 1, &ra.n_ids) : U3{0, 0, 0};
    const uint64_t qt = q3.a + q3.b + q3.c;
    heap_reserve(qt);
    for (DRows *R : {&sv[0], &sv[1], &sv[2], &lv}) { R->key = heap_k; R->val = heap_v; }
    ra.a = sv[0]; ra.b = sv[1]; ra.c = sv[2];
    DRows out[3];  // the rewritten rows (committed to sv by k_commit_round)
    for (int q = 0; q < 3; ++q) {
      out[q] = sv[q];
      out[q].off = A.get<uint64_t>(part_name("r.o", q, ".off"), n_st);
      out[q].len = A.get<uint32_t>(part_name("r.o", q, ".len"), n_st);
    }
    launch(st, k_set_offsets_u3, n_st, (const U3 *)rsc3, heap_top, heap_top + q3.a, heap_top + q3.a + q3.b, n_st, out[0].off,
           out[1].off, out[2].off, (const U3 *)nullptr, (const uint32_t *)nullptr);
    heap_top += qt;
    ra.c_base = heap_top - q3.c;  // row scratch = 2 * (its C offset - c_base)
    ra.oa = out[0]; ra.ob = out[1]; ra.oc = out[2];
    ra.tmpk = A.get<uint32_t>("r.tmpk", 2 * (q3.c + 1));
    ra.tmpv = A.get<Fe>("r.tmpv", 2 * (q3.c + 1));
    MK.mark("count");
    {  // compact the touched rows: the fill's lanes all have work
      uint32_t *tids = A.get<uint32_t>("r.touch_ids", n_st);
      if (ra.n_ids > n_st) throw RsError(RS_E_INTERNAL, "round: touched rows out of range");
      if (ra.n_ids) launch(st, k_scatter_ids, n_st, (const uint64_t *)tfl, (const uint64_t *)tfp, n_st, tids);
      ra.ids = tids;
      HC(hipMemsetAsync(ra.turn, 0xff, 4 * n_st, st));
      HC(hipMemsetAsync(ra.touched, 0, n_st, st));
    }
    ra.bytes = A.get<unsigned long long>("r.bytes", 1);
    HC(hipMemsetAsync(ra.bytes, 0, 8, st));
    if (ra.n_ids) {
      FrameWaveArgs w{};
      w.fr.F = E->F;
      w.fr.sub_of = r_sub_of;
      w.fr.h_off = ra.h_off; w.fr.h_len = ra.h_len; w.fr.pk = ra.pk; w.fr.pv = ra.pv;
      for (int q = 0; q < 3; ++q) { w.in[q] = sv[q]; w.out[q] = out[q]; w.cap[q] = rcap[q]; }
      w.cap_by_row = 1;
      w.ids = ra.ids;
      w.n = ra.n_ids;
      w.big = A.get<uint32_t>("r.big", ra.n_ids);
      w.n_big = A.get<unsigned>("r.nbig", 2);
      w.round = 1;
      w.touched = ra.touched;
      w.turn_list = A.get<uint32_t>("r.turnlist", ra.n_ids);
      w.n_turn = w.n_big + 1;
      w.err = d_fw_err;
      w.bytes = ra.bytes;
      HC(hipMemsetAsync(w.n_big, 0, 8, st));
#ifdef RS_FWCLK
      w.clk = A.get<unsigned long long>("fw.clkr", 32);
      HC(hipMemsetAsync(w.clk, 0, 8 * 32, st));
#endif
      RoundArgs rb = ra, rt = ra;
      rb.rlist = w.big; rb.n_rlist = w.n_big;
      rt.rlist = w.turn_list; rt.n_rlist = w.n_turn;
      HC(hipEventRecord(E->ev[kEvFill0], st));
      launch_capped(st, k_frames_wave<1>, ra.n_ids, kFwBlocks, w);
      {  // the rows too long for a wave's LDS batch: A / B / C expanded by one device-wide sort
        unsigned nbig = 0;
        HC(hipMemcpyAsync(&nbig, w.n_big, 4, hipMemcpyDeviceToHost, st));
        HC(hipStreamSynchronize(st));
#ifdef RS_FWCLK
        if (g_prof_env) {
          unsigned long long c[32];
          HC(hipMemcpy(c, w.clk, sizeof c, hipMemcpyDeviceToHost));
          fprintf(stderr, "[rs-prof] round frames clocks (Mcycles summed over waves): groups %.1f entries %.1f terms %.1f "
                  "rank %.1f emit %.1f rows %.1f plan %.1f | batches %llu, wave total %.1f over %llu waves | emit: loads %.1f "
                  "values %.1f sync %.1f stores %.1f | %u rows over a batch of %llu\n", c[0] / 1e6, c[1] / 1e6, c[2] / 1e6,
                  c[3] / 1e6, c[5] / 1e6, c[6] / 1e6, c[7] / 1e6, c[8], c[9] / 1e6, c[10], c[16] / 1e6, c[17] / 1e6,
                  c[18] / 1e6, c[19] / 1e6, nbig, (unsigned long long)ra.n_ids);
        }
#endif
        if (nbig) {
          const uint64_t nseg = 3ull * nbig;
          uint64_t *xc = A.get<uint64_t>("x.cnt", nseg), *xo = A.get<uint64_t>("x.off", nseg + 1);
          launch(st, k_xrow_count, nseg, rb, nseg, xc);
          const uint64_t T = excl_scan_u64(E, xc, xo, nseg, "xrow");
          h2d(E, xo + nseg, &T, 8);
          if (T) {
            uint64_t *xk = A.get<uint64_t>("x.k", T), *xk2 = A.get<uint64_t>("x.k2", T);
            uint32_t *xi = A.get<uint32_t>("x.i", T), *xi2 = A.get<uint32_t>("x.i2", T);
            Fe *xv = A.get<Fe>("x.v", T);
            launch(st, k_xrow_expand, 64 * nseg, rb, nseg, (const uint64_t *)xo, xk, xv, xi);
            int sbits = 1;
            while (sbits < 32 && (1ull << sbits) <= nseg) ++sbits;
            sort_pairs(E, (const uint64_t *)xk, xk2, (const uint32_t *)xi, xi2, T, 32 + sbits, "xrow");
            launch(st, k_xrow_combine, 64 * nseg, rb, nseg, (const uint64_t *)xo, (const uint64_t *)xk2,
                   (const uint32_t *)xi2, (const Fe *)xv);
          } else {
            launch(st, k_xrow_combine, 64 * nseg, rb, nseg, (const uint64_t *)xo, (const uint64_t *)nullptr,
                   (const uint32_t *)nullptr, (const Fe *)nullptr);
          }
          rb.pre_expanded = 1;
        }
      }
      launch(st, k_round_fill, ra.n_ids, rb);
      launch(st, k_round_turn, ra.n_ids, rt);
      HC(hipEventRecord(E->ev[kEvFill1], st));
      if (g_prof_env) {
        unsigned nb[2] = {0, 0};
        HC(hipMemcpyAsync(nb, w.n_big, 8, hipMemcpyDeviceToHost, st));
        HC(hipStreamSynchronize(st));
        fprintf(stderr, "[rs-prof] round: %llu rows, %u over a wave batch, %u turn\n", (unsigned long long)ra.n_ids, nb[0], nb[1]);
      }
      float fm = 0;
      unsigned long long fb = 0;
      HC(hipMemcpyAsync(&fb, ra.bytes, 8, hipMemcpyDeviceToHost, st));
      HC(hipEventSynchronize(E->ev[kEvFill1]));
      HC(hipStreamSynchronize(st));
      HC(hipEventElapsedTime(&fm, E->ev[kEvFill0], E->ev[kEvFill1]));
      E->stats.round_fill_ms += fm;
      E->stats.round_fill_bytes += fb;
      E->stats.round_fill_launches++;
    }
    MK.mark("fill");
    if (env_flag("RS_DEBUG")) debug_check_round(E, ra, n_st, qt);
    launch(st, k_commit_round, n_st, (const uint8_t *)ra.touched, (const int32_t *)ra.turn, n_st, sv[0], sv[1], sv[2], out[0], out[1],
           out[2]);
    if (so_dirty) launch(st, k_or_u8, n_st, (const uint8_t *)ra.touched, n_st, so_dirty);
    snap_round(ra.touched, ra.turn);
    // turned rows
    uint64_t *tf = A.get<uint64_t>("r.tf", n_st), *tp = A.get<uint64_t>("r.tp", n_st);
    launch(st, k_turn_flags, n_st, (const int32_t *)ra.turn, n_st, tf);
    uint64_t n_turn = excl_scan_u64(E, tf, tp, n_st, "tf");
    uint32_t *tids = A.get<uint32_t>("r.tids", n_turn);
    launch(st, k_scatter_ids, n_st, (const uint64_t *)tf, (const uint64_t *)tp, n_st, tids);
    std::vector<uint32_t> htids(n_turn);
    std::vector<int32_t> hturn(n_turn);  // turn value of each turned row (aligned with htids)
    if (n_turn) {
      int32_t *d_tt = A.get<int32_t>("r.tturn", n_turn);
      launch(st, k_gather_u32, n_turn, (const uint32_t *)ra.turn, (const uint32_t *)tids, (uint32_t *)d_tt, n_turn);
      HC(hipMemcpyAsync(htids.data(), tids, 4 * n_turn, hipMemcpyDeviceToHost, st));
      HC(hipMemcpyAsync(hturn.data(), d_tt, 4 * n_turn, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
      need_usig();
    }
    std::unordered_map<uint32_t, std::vector<uint32_t>> ext;  // appended lists of those signals
    {  // initial map lists of the turning substitutions' signals only
      double Tq = now_ms();
      std::vector<uint32_t> qs;
      for (uint64_t i = 0; i < n_turn; ++i) qs.push_back(usig[hturn[i]]);
      std::sort(qs.begin(), qs.end());
      qs.erase(std::unique(qs.begin(), qs.end()), qs.end());
      query_initial(qs);
      ext = ML.resolve(qs, [this](const std::vector<uint32_t> &sigs) { query_initial(sigs); });
      E->stats.map_ms += now_ms() - Tq;
    }
    // order key: (rank of the turning substitution, first position in map[from])
    for (uint64_t ti = 0; ti < n_turn; ++ti) {
      const uint32_t r = htids[ti];
      int32_t q = hturn[ti];
      uint32_t from = usig[q];
      uint64_t pos = UINT64_MAX;
      const std::vector<uint32_t> &L0 = ML.minit[from];
      auto lb = std::lower_bound(L0.begin(), L0.end(), r);  // initial lists are ascending
      if (lb != L0.end() && *lb == r) pos = lb - L0.begin();
      if (pos == UINT64_MAX) {
        auto it = ext.find(from);
        if (it != ext.end())
          for (uint64_t t = 0; t < it->second.size(); ++t)
            if (it->second[t] == r) { pos = L0.size() + t; break; }
      }
      if (pos == UINT64_MAX) throw RsError(RS_E_INTERNAL, "substituted row missing from the signal map");
      turned.push_back({((uint64_t)q << 32) | (pos & 0xffffffffu), r});
    }
    std::sort(turned.begin(), turned.end());
    MK.mark("turned");
    if (env_flag("RS_DEBUG")) {
      std::vector<uint8_t> tch(n_st);
      HC(hipMemcpy(tch.data(), ra.touched, n_st, hipMemcpyDeviceToHost));
      uint64_t nt = 0;
      for (auto x : tch) nt += x;
      fprintf(stderr, "[rs-debug] round: nU=%llu touched=%llu turned=%llu:", (unsigned long long)nU,
              (unsigned long long)nt, (unsigned long long)n_turn);
      for (auto &t : turned) fprintf(stderr, " %u(q%llu)", t.second, (unsigned long long)(t.first >> 32));
      fprintf(stderr, "\n");
    }
  }
  // the end of a round: the dense rank index reset, the map appends (:369-377; the key set on the
  // device, the row lists only when another round follows), the next linear list lv (the turned rows,
  // non-empty, in linear_id order), the turned storage rows emptied.  Returns the next list's length.
  uint64_t round_next() {
    if (nU) launch(st, k_unset_rank, nU, (const uint32_t *)d_us, nU, rank_of);  // reset the dense rank index
    // next linear list: the turned rows, non-empty, in linear_id order
    std::vector<uint32_t> next_ids;
    {
      if (!turned.empty()) {  // C lengths of the turned rows only
        std::vector<uint32_t> tid_(turned.size()), tlen(turned.size());
        for (size_t i = 0; i < turned.size(); ++i) tid_[i] = turned[i].second;
        uint32_t *d_t = A.get<uint32_t>("r.tid", tid_.size()), *d_tl = A.get<uint32_t>("r.tlen", tid_.size());
        h2d(E, d_t, tid_.data(), 4 * tid_.size());
        launch(st, k_gather_u32, tid_.size(), (const uint32_t *)sv[2].len, (const uint32_t *)d_t, d_tl, (uint64_t)tid_.size());
        HC(hipMemcpyAsync(tlen.data(), d_tl, 4 * tlen.size(), hipMemcpyDeviceToHost, st));
        HC(hipStreamSynchronize(st));
        for (size_t i = 0; i < turned.size(); ++i)
          if (tlen[i]) next_ids.push_back(turned[i].second);
      }
    }
    uint64_t nn = next_ids.size();
    // map appends (:369-377): the key set on the device; the row lists (positions for a later
    // round's ordering) only when another round follows
    if (nU) {
      launch(st, k_append_marks, nU, (const uint32_t *)d_us, (const uint64_t *)d_uoff, (const uint32_t *)d_ulen, nU,
             (const uint32_t *)P.pk, nlmap);
    }
    const bool another = nn > 0 && (no_rounds > 0 ? no_rounds - 1 : 0) > 0;
    if (another) {
      double Tq = now_ms();
      need_usig();
      // this round's batch of appends: every substitution's `from` and RHS keys (no values).  The
      // keys are copied on the device now (the next round's elimination reuses the pool) and come to
      // the host only if a later round resolves a list through this batch -- most never do (the
      // templated circuit's round 2: 9.8 ms of D2H and host copies saved per call)
      MapLists::Batch B;
      B.from = usig;
      const size_t bi = ML.batches.size();
      const std::string bn = "ml." + std::to_string(bi);
      uint64_t *d_optr = A.get<uint64_t>(bn + ".ptr", nU + 1);
      uint64_t *d_len64 = A.get<uint64_t>(bn + ".len", nU + 1);
      launch(st, k_u32_to_u64, nU, (const uint32_t *)d_ulen, d_len64, nU);
      HC(hipMemsetAsync(d_len64 + nU, 0, 8, st));
      const uint64_t tot = excl_scan_u64(E, d_len64, d_optr, nU + 1, "mlb");
      uint32_t *d_keys = A.get<uint32_t>(bn + ".keys", std::max<uint64_t>(tot, 1));
      if (tot)
        launch(st, k_pool_keys, 64 * nU, (const uint64_t *)d_uoff, (const uint32_t *)d_ulen, (const uint64_t *)d_optr, nU,
               (const uint32_t *)P.pk, d_keys);
      B.load = [E = E, d_optr, d_keys, nU = nU, tot](MapLists::Batch &Bt) {  // (this round's nU, by value)
        Bt.ptr.resize(nU + 1);
        Bt.keys.resize(tot);
        HC(hipMemcpyAsync(Bt.ptr.data(), d_optr, 8 * (nU + 1), hipMemcpyDeviceToHost, E->st));
        if (tot) HC(hipMemcpyAsync(Bt.keys.data(), d_keys, 4 * tot, hipMemcpyDeviceToHost, E->st));
        HC(hipStreamSynchronize(E->st));
      };
      ML.add_batch(std::move(B));
      E->stats.map_ms += now_ms() - Tq;
    }
    MK.mark("appends2");
    lv.n = nn;
    lv.off = A.get<uint64_t>("lv.off", nn);
    lv.len = A.get<uint32_t>("lv.len", nn);
    lv.key = heap_k;
    lv.val = heap_v;
    if (nn) {
      uint32_t *d_ids = A.get<uint32_t>("lv.ids", nn);
      h2d(E, d_ids, next_ids.data(), 4 * nn);
      launch(st, k_view_rows, nn, (const uint64_t *)sv[2].off, (const uint32_t *)sv[2].len, (const uint32_t *)d_ids, nn, lv.off, lv.len);
    }
    // emptied storage rows (storage.replace(c_id, C::empty()))
    if (!turned.empty()) {
      std::vector<uint32_t> all;
      for (auto &t : turned) all.push_back(t.second);
      uint32_t *d_all = A.get<uint32_t>("r.all", all.size());
      h2d(E, d_all, all.data(), 4 * all.size());
      launch(st, k_zero_c, all.size(), (const uint32_t *)d_all, (uint64_t)all.size(), sv[2].len);
    }
    HC(hipStreamSynchronize(st));
    if (env_flag("RS_DEBUG")) {
      for (uint64_t r = 0; r < std::min<uint64_t>(n_st, 24); ++r) {
        uint32_t la = 0, lb = 0, lc = 0;
        HC(hipMemcpy(&la, sv[0].len + r, 4, hipMemcpyDeviceToHost));
        HC(hipMemcpy(&lb, sv[1].len + r, 4, hipMemcpyDeviceToHost));
        HC(hipMemcpy(&lc, sv[2].len + r, 4, hipMemcpyDeviceToHost));
        std::vector<uint32_t> kk;
        std::vector<Fe> vv;
        d2h_row(E, sv[2], r, kk, vv);
        fprintf(stderr, "[rs-debug] storage %llu lens %u %u %u C:", (unsigned long long)r, la, lb, lc);
        for (size_t i = 0; i < kk.size(); ++i) fprintf(stderr, " %u:%llu", kk[i], (unsigned long long)ffrom_mont(E->F, vv[i]).l[0]);
        fprintf(stderr, "\n");
      }
    }
    return nn;
  }

  // The streamed layout of a single engine, all three parts per pass (output.hpp, the fused layout):
  // late lengths -> scan -> extents, ABI 8 lengths and jump flags -> scan -> one read of the totals ->
  // jump tables and the late rows' gathers.  tots / h_tots: assemble's device words [5..13] and their pinned copy.
  void assemble_fused(const DRows &lcv, const uint32_t *keep_ids, uint32_t *const (&x_ids)[2], uint64_t n_keep, const uint64_t (&n_x)[2],
                      uint32_t *zero_len, uint64_t *tots, uint64_t *h_tots) {
    const char *nm[3] = {"out.a", "out.b", "out.c"};
    const uint64_t m = n_keep + n_x[0] + n_x[1];
    OutRows R{};
    for (int q = 0; q < 3; ++q) {
      R.st[q] = sv[q];
      E->fin_parts[q] = sv[q];
      E->fin_xq[0][q] = lv;
      E->fin_xq[1][q] = lcv;
      if (q < 2) E->fin_xq[0][q].len = E->fin_xq[1][q].len = zero_len;
    }
    R.xl = lv;
    R.xc = lcv;
    R.keep = keep_ids;
    R.xl_ids = x_ids[0];
    R.xc_ids = x_ids[1];
    R.n_keep = n_keep;
    R.n_xl = n_x[0];
    R.n_xc = n_x[1];
    R.nl_of = st_ids;
    R.early = so_early;
    R.dirty = so_dirty;
    R.eoff = so_eoff;
    R.lc_snap_n = E->lc_snap_n;
    R.lc_snap_base = E->lc_snap_base;
    R.base = U3{E->snap_e[0], E->snap_e[1], E->snap_e[2]};
    U3 *late = A.get<U3>("fin.late3", m), *lptr = A.get<U3>("fin.lptr3", m), *beg = A.get<U3>("fin.beg3", m);
    U3 *jf = A.get<U3>("fin.jf3", m), *jpos = A.get<U3>("fin.jpos3", m);
    uint32_t *len32[3];
    for (int q = 0; q < 3; ++q) len32[q] = A.get<uint32_t>(std::string(nm[q]) + ".len32", m + 1);
    if (m) {
      // (capped: its per-wave atomics on three words serialise in the L2 -- 1.7 ms from an uncapped grid of 3 M rows)
      launch_capped(st, k_out_late3, m, 1024, R, m, late, (unsigned long long *)(tots + 11));
      dev_scan_u3(E, late, lptr, m, st, "late");
      launch(st, k_scan_total_u3, 1, (const U3 *)late, (const U3 *)lptr, m, tots + 5);
      launch(st, k_out_layout3, m, R, m, (const U3 *)lptr, len32[0], len32[1], len32[2], beg, jf);
      dev_scan_u3(E, jf, jpos, m, st, "jump");
      launch(st, k_scan_total_u3, 1, (const U3 *)jf, (const U3 *)jpos, m, tots + 8);
    }
    HC(hipMemcpyAsync(h_tots + 5, tots + 5, 8 * 9, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    uint64_t *jtab[3];
    bool any_j = false;
    for (int q = 0; q < 3; ++q) {
      const uint64_t L = h_tots[5 + q], nj = h_tots[8 + q];
      if (nj > m) throw RsError(RS_E_INTERNAL, "final assembly: jump count out of range");
      E->out_ext[q] = E->snap_e[q] + L;
      E->out_njump[q] = nj;
      E->out_nnz[q] = h_tots[11 + q];
      jtab[q] = A.get<uint64_t>(std::string(nm[q]) + ".jtab", nj + 1);
      any_j |= nj != 0;
    }
    if (any_j) launch(st, k_out_jtab3, m, (const U3 *)beg, (const U3 *)jf, (const U3 *)jpos, m, jtab[0], jtab[1], jtab[2]);
    for (int q = 0; q < 3; ++q) {
      const uint64_t base = E->snap_e[q], ext = E->out_ext[q], L = ext - base;
      // the device copy of the whole layout grows past the early region when it must (the
      // early region is copied along once its gather is done)
      const std::string xc = std::string(nm[q]) + ".xcol", xv = std::string(nm[q]) + ".xval";
      if (A.cap_bytes(xc) < 4 * ext || A.cap_bytes(xv) < 32 * ext) snap_join(E);  // its D2H reads them
      A.grow_keep<uint32_t>(xc, ext, base, E->stc, st);
      A.grow_keep<uint64_t>(xv, 4 * ext, 4 * base, E->stc, st);
      uint32_t *col = A.get<uint32_t>(xc, ext);
      uint64_t *val = A.get<uint64_t>(xv, 4 * ext);
      if (!L) continue;
      E->kg[2].run(st, 30 * m + 72 * L, [&] {
        launch(st, k_gather_late_all, m, E->F, R, q, m, (const U3 *)lptr, col + base, val + 4 * base);
      });
    }
  }

  // ======================= final assembly (:648-729)
  // Reads sv, lv, lc, nlmap, the bitmaps, st_ids and the streamed-output state (so_early,
  // so_eoff, so_dirty, snap_e).  Leaves in the engine: the witness map (n_wires, npiw, fin.l2w), the
  // output rows' views (fin_*), out_nnz, and -- streamed -- the late region behind the early one with
  // every row's extent (out_ext, out_njump); else the compact CSR.
  void assemble() {
    Tf = now_ms();
    if (g_prof_env) {  // how far the result stream is as the assembly starts (after the device caught up)
      HC(hipStreamSynchronize(st));
      std::lock_guard<std::mutex> lk(E->snap_m);
      E->asm_t0_ms = now_ms();
      E->asm_open = E->snap_open;
    }
    // leftover linear rows (rounds exhausted) and lconst: appended after the storage rows; their
    // signals join the non-linear map (:648-686)
    const DRows lcv = lc.view(A);
    if (lv.n) launch(st, k_mark_keys, lv.n, lv, nlmap);
    if (lcv.n) launch(st, k_mark_keys, lcv.n, lcv, nlmap);
    HC(hipMemsetAsync(nlmap, 0, 1, st));  // the constant key is not a signal
    uint32_t *kept = A.get<uint32_t>("fin.kept", S);
    uint64_t *kept64 = A.get<uint64_t>("fin.kept64", S);
    uint64_t *rank = A.get<uint64_t>("fin.rank", S);
    int32_t *l2w = A.get<int32_t>("fin.l2w", S);
    // every total of this phase is left in one block of device words and read in two copies (two
    // synchronisations): [0] wires [1] inputs not kept [2] kept storage rows [3..4] non-empty extras,
    // then (single engine, streamed) [5..7] late entries [8..10] jumps [11..13] entries per part
    uint64_t *tots = A.get<uint64_t>("fin.tots", 14);
    uint64_t *h_tots = (uint64_t *)pin_get(E, kPinRead, kPinRb);
    HC(hipMemsetAsync(tots, 0, 8 * 14, st));
    launch(st, k_kept_count, S, (const uint8_t *)d_deleted, (const uint8_t *)d_forb, (const uint8_t *)nlmap, kept, kept64, S,
           E->n_pub_out + 1, E->n_pub_out + E->n_pub_in + E->n_priv_in, (unsigned long long *)(tots + 1));
    dev_scan_u64(E, kept64, rank, S, st, "kept");
    launch(st, k_scan_total_u64, 1, (const uint64_t *)kept64, (const uint64_t *)rank, S, tots + 0);
    launch(st, k_l2w, S, (const uint32_t *)kept, (const uint64_t *)rank, l2w, S);
    Comm *CMf = E->comm.get();
    const bool shard = E->snap_on && CMf && CMf->world > 1;
    const bool fused = E->snap_on && !shard;  // single engine, streamed: the fused layout
    // output rows: storage (non-empty) ++ leftover linear ++ lconst, empty rows dropped
    // (extract_with(is_empty), :697); the last two are C-only ("extras")
    {
      const DRows xsrc[2] = {lv, lcv};
      uint64_t *nef = A.get<uint64_t>("fin.nef", n_st), *nep = A.get<uint64_t>("fin.nep", n_st);
      uint64_t *xf[2], *xp[2];
      for (int x = 0; x < 2; ++x) {
        xf[x] = A.get<uint64_t>(x ? "fin.xf1" : "fin.xf0", xsrc[x].n);
        xp[x] = A.get<uint64_t>(x ? "fin.xp1" : "fin.xp0", xsrc[x].n);
      }
      const uint64_t n_cand = n_st + lv.n + lcv.n;
      if (n_cand) launch(st, k_nonempty_flags3, n_cand, sv[0], sv[1], sv[2], n_st, lv, lcv, nef, xf[0], xf[1]);
      dev_scan_u64(E, nef, nep, n_st, st, "ne");
      launch(st, k_scan_total_u64, 1, (const uint64_t *)nef, (const uint64_t *)nep, n_st, tots + 2);
      for (int x = 0; x < 2; ++x) {
        dev_scan_u64(E, xf[x], xp[x], xsrc[x].n, st, x ? "xf1" : "xf0");
        launch(st, k_scan_total_u64, 1, (const uint64_t *)xf[x], (const uint64_t *)xp[x], xsrc[x].n, tots + 3 + x);
      }
      HC(hipMemcpyAsync(h_tots, tots, 8 * 5, hipMemcpyDeviceToHost, st));
      HC(hipStreamSynchronize(st));
      E->n_wires = h_tots[0];
      E->npiw = E->n_priv_in - h_tots[1];
      const uint64_t n_keep = h_tots[2];
      uint64_t n_x[2] = {h_tots[3], h_tots[4]}, x_at[2];
      uint32_t *keep_ids = A.get<uint32_t>("fin.keep", n_keep);
      uint32_t *x_ids[2] = {A.get<uint32_t>("fin.lvids", lv.n), A.get<uint32_t>("fin.lcids", lcv.n)};
      if (n_keep > n_st || n_x[0] > lv.n || n_x[1] > lcv.n) throw RsError(RS_E_INTERNAL, "final assembly: row counts out of range");
      if (n_cand)
        launch(st, k_scatter_ids3, n_cand, (const uint64_t *)nef, (const uint64_t *)nep, n_st, (const uint64_t *)xf[0],
               (const uint64_t *)xp[0], lv.n, (const uint64_t *)xf[1], (const uint64_t *)xp[1], lcv.n, keep_ids, x_ids[0], x_ids[1]);
      const uint64_t zn = std::max<uint64_t>(lv.n, lcv.n);
      uint32_t *zero_len = A.get<uint32_t>("fin.zlen", zn);
      if (zn) HC(hipMemsetAsync(zero_len, 0, 4 * zn, st));
      x_at[0] = n_keep;
      x_at[1] = n_keep + n_x[0];
      const uint64_t n_out = n_keep + n_x[0] + n_x[1];
      E->out_n_dev = n_out;
      const DRows *parts[3] = {&sv[0], &sv[1], &sv[2]};
      const char *nm[3] = {"out.a", "out.b", "out.c"};
      if (fused) assemble_fused(lcv, keep_ids, x_ids, n_keep, n_x, zero_len, tots, h_tots);
      // the streamed layout covers this engine's rows: all of them, or sharded its share -- the kept
      // storage rows of its non-linear rows (a run [k_lo, k_hi) of the keep list), the last rank also
      // the two C-only tails
      uint64_t k_lo = 0, k_hi = n_keep;
      bool with_x = true;
      if (shard) {
        uint64_t kr[2] = {0, 0};
        if (n_keep) {
          uint64_t *d_kr = A.get<uint64_t>("fin.krange", 2);
          launch(st, k_keep_range, 2, (const uint32_t *)keep_ids, n_keep, (const uint32_t *)st_ids, E->nl_lo, E->nl_hi, d_kr);
          HC(hipMemcpyAsync(kr, d_kr, 16, hipMemcpyDeviceToHost, st));
          HC(hipStreamSynchronize(st));
        }
        k_lo = kr[0];
        k_hi = std::max(kr[0], kr[1]);
        with_x = CMf->rank == CMf->world - 1;
      }
      E->sh_klo = k_lo;
      E->sh_khi = k_hi;
      const uint64_t own = k_hi - k_lo;
      const uint32_t *own_ids = keep_ids + k_lo;
      const uint64_t xl_at[2] = {own, own + (with_x ? n_x[0] : 0)};
      const uint64_t xl_n[2] = {with_x ? n_x[0] : 0, with_x ? n_x[1] : 0};
      const uint64_t m_loc = own + xl_n[0] + xl_n[1];
      E->csr_rows_ready = !fused;  // (the fused layout leaves the compact CSR's row pointers to ensure_csr)
      for (int q = 0; q < 3 && !fused; ++q) {  // not streamed, or sharded: one part at a time
        uint64_t *lens = A.get<uint64_t>(std::string(nm[q]) + ".lens", n_out + 1);
        uint64_t *ptr = A.get<uint64_t>(std::string(nm[q]) + ".ptr", n_out + 1);
        if (n_keep) launch(st, k_row_lens, n_keep, *parts[q], (const uint32_t *)keep_ids, n_keep, lens);
        DRows xq[2];
        for (int x = 0; x < 2; ++x) {
          xq[x] = xsrc[x];
          if (q < 2) xq[x].len = zero_len;
          if (n_x[x]) launch(st, k_row_lens, n_x[x], xq[x], (const uint32_t *)x_ids[x], n_x[x], lens + x_at[x]);
          E->fin_xq[x][q] = xq[x];
        }
        HC(hipMemsetAsync(lens + n_out, 0, 8, st));
        uint64_t tot = excl_scan_u64(E, lens, ptr, n_out + 1, nm[q]);
        E->out_nnz[q] = tot;
        E->fin_parts[q] = *parts[q];
        if (!E->snap_on) continue;
        // streamed layout: the rows not reused from the early region, after it
        uint64_t *late = A.get<uint64_t>(std::string(nm[q]) + ".late", m_loc + 1);
        uint64_t *lptr = A.get<uint64_t>(std::string(nm[q]) + ".lptr", m_loc + 1);
        if (own) launch(st, k_out_late_lens, own, *parts[q], own_ids, own, (const uint32_t *)st_ids, (const uint8_t *)so_early,
                        (const uint8_t *)so_dirty, late);
        if (xl_n[0]) launch(st, k_row_lens, xl_n[0], xq[0], (const uint32_t *)x_ids[0], xl_n[0], late + xl_at[0]);
        if (xl_n[1]) launch(st, k_lc_late_lens, xl_n[1], xq[1], (const uint32_t *)x_ids[1], xl_n[1], E->lc_snap_n, late + xl_at[1]);
        HC(hipMemsetAsync(late + m_loc, 0, 8, st));
        const uint64_t L = excl_scan_u64(E, late, lptr, m_loc + 1, "late");
        const uint64_t base = E->snap_e[q], ext = base + L;
        E->out_ext[q] = ext;
        uint64_t *beg = A.get<uint64_t>(std::string(nm[q]) + ".beg", m_loc + 1);
        uint64_t *end = A.get<uint64_t>(std::string(nm[q]) + ".end", m_loc + 1);

        if (own) launch(st, k_out_extent, own, *parts[q], own_ids, own, (const uint32_t *)st_ids, (const uint8_t *)so_early,
                        (const uint8_t *)so_dirty, (const U3 *)so_eoff, q, base, (const uint64_t *)lptr, beg, end);
        if (xl_n[0])
          launch(st, k_out_extent, xl_n[0], xq[0], (const uint32_t *)x_ids[0], xl_n[0], (const uint32_t *)nullptr, (const uint8_t *)nullptr,
                 (const uint8_t *)nullptr, (const U3 *)nullptr, q, base, (const uint64_t *)(lptr + xl_at[0]), beg + xl_at[0], end + xl_at[0]);
        if (xl_n[1])
          launch(st, k_lc_extent, xl_n[1], xq[1], (const uint32_t *)x_ids[1], xl_n[1], E->lc_snap_n, E->lc_snap_base, q, base,
                 (const uint64_t *)(lptr + xl_at[1]), beg + xl_at[1], end + xl_at[1]);
        launch(st, k_set_u64, 1, beg + m_loc, ext);
        {  // ABI 8: per row its length (+ RS_ROW_JUMP) and the jump table -- what crosses the link
          uint32_t *len32 = A.get<uint32_t>(std::string(nm[q]) + ".len32", m_loc + 1);
          uint64_t *jf = A.get<uint64_t>(std::string(nm[q]) + ".jf", m_loc + 1);
          uint64_t *jpos = A.get<uint64_t>(std::string(nm[q]) + ".jpos", m_loc + 1);
          uint64_t nj = 0;
          if (m_loc) {
            launch(st, k_out_jumps, m_loc, (const uint64_t *)beg, (const uint64_t *)end, m_loc, shard ? 1 : 0, len32, jf);
            nj = excl_scan_u64(E, jf, jpos, m_loc, "jump");
          }
          uint64_t *jtab = A.get<uint64_t>(std::string(nm[q]) + ".jtab", nj + 1);
          if (nj) launch(st, k_out_jtab, m_loc, (const uint64_t *)beg, (const uint64_t *)jf, (const uint64_t *)jpos, m_loc, (uint64_t)0, jtab);
          E->out_njump[q] = nj;
          if (shard) (void)A.get<uint64_t>(std::string(nm[q]) + ".jtabx", nj + 1);  // fetch_result_shared's rebased copy
        }
        // the device copy of the whole layout grows past the early region when it must (the
        // early region is copied along once its gather is done)
        const std::string xc = std::string(nm[q]) + ".xcol", xv = std::string(nm[q]) + ".xval";
        if (A.cap_bytes(xc) < 4 * ext || A.cap_bytes(xv) < 32 * ext) snap_join(E);  // its D2H reads them
        A.grow_keep<uint32_t>(xc, ext, base, E->stc, st);
        A.grow_keep<uint64_t>(xv, 4 * ext, 4 * base, E->stc, st);
        uint32_t *col = A.get<uint32_t>(xc, ext);
        uint64_t *val = A.get<uint64_t>(xv, 4 * ext);
        E->kg[2].run(st, 30 * (own + xl_n[0] + xl_n[1]) + 72 * L, [&] {
          if (own) launch(st, k_gather_late, own, E->F, *parts[q], own_ids, own, (const uint32_t *)st_ids, (const uint8_t *)so_early,
                          (const uint8_t *)so_dirty, (const uint64_t *)lptr, col + base, val + 4 * base);
          if (xl_n[0])
            launch(st, k_gather_late, xl_n[0], E->F, xq[0], (const uint32_t *)x_ids[0], xl_n[0], (const uint32_t *)nullptr,
                   (const uint8_t *)nullptr, (const uint8_t *)nullptr, (const uint64_t *)(lptr + xl_at[0]), col + base, val + 4 * base);
          if (xl_n[1])
            launch(st, k_lc_gather_late, xl_n[1], E->F, xq[1], (const uint32_t *)x_ids[1], xl_n[1], E->lc_snap_n,
                   (const uint64_t *)(lptr + xl_at[1]), col + base, val + 4 * base);
        });
      }
      if (shard) {  // a share past its capacity: the region regrows and every rank copies its whole layout
        uint64_t over = 0;
        for (int q = 0; q < 3; ++q) over |= E->out_ext[q] > E->sh_cap[q];
        if (CMf->max_u64(over, st)) {
          snap_join(E);  // the early copies into the old region are done (they are redone below)
          for (int q = 0; q < 3; ++q) E->sh_cap[q] = CMf->max_u64(E->out_ext[q] + E->out_ext[q] / 4 + 65536, st);
          E->sh_ent = CMf->shared_host(0, sh_ent_bytes(E), st);
          // (the first snapshot's shared_host already fell back when the host had no room; a regrow
          // that fails here is an error every rank reports alike)
          if (!E->sh_ent) throw RsError(RS_E_RCCL, "no shared host memory for the sharded result");
          E->sh_full = true;
        }
      }
      E->fin_keep = n_keep;
      E->fin_keep_ids = keep_ids;
      for (int x = 0; x < 2; ++x) {
        E->fin_xn[x] = n_x[x];
        E->fin_x_ids[x] = x_ids[x];
      }
      E->fin_gen = A.gen;
      if (!E->snap_on) ensure_csr(E);
    }
    if (g_prof_env) {
      HC(hipStreamSynchronize(st));
      std::lock_guard<std::mutex> lk(E->snap_m);
      E->asm_end_ms = now_ms();
      fprintf(stderr, "[rs-prof] final assembly: %.2f ms (device done); the result stream had %d copies unfinished at its start, "
                      "%d at its end (its last copy was done %.2f ms before the end)\n",
              E->asm_end_ms - E->asm_t0_ms, E->asm_open, E->snap_open, E->asm_end_ms - E->snap_last_ms);
    }
  }

  // ======================= the end of the run: the device checks' verdict, the stats, RS_PROF's memory report
  void finish() {
    load_wait_all(E);  // a group the path never needed (e.g. no non-linear rows) is still checked
    int err = 0, fw_err = 0;
    HC(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st));
    HC(hipMemcpyAsync(&fw_err, d_fw_err, 4, hipMemcpyDeviceToHost, st));
    HC(hipStreamSynchronize(st));
    if (err) throw RsError(RS_E_INVALID, "input rejected by the device checks (code " + std::to_string(err) + ")");
    if (fw_err) throw RsError(RS_E_INTERNAL, "frames batch over its bounds (code " + std::to_string(fw_err) + ")");
    E->stats.final_ms = now_ms() - Tf;
    E->stats.total_ms = now_ms() - T0;
    if (g_prof_env) {
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) == hipSuccess)
        fprintf(stderr, "[rs-prof] device memory in use after the run: %.1f of %.1f GB (heap %.1f GB)\n", (tot - fr) / 1e9, tot / 1e9,
                36e-9 * E->heap_cap);
      std::vector<std::pair<size_t, std::string>> big;
      size_t sum = 0;
      for (auto &kv : A.bufs) {
        big.push_back({kv.second.cap, kv.first});
        sum += kv.second.cap;
      }
      std::sort(big.rbegin(), big.rend());
      fprintf(stderr, "[rs-prof] arena %.1f GB in %zu buffers; largest:", sum / 1e9, big.size());
      for (size_t i = 0; i < big.size() && i < 16; ++i) fprintf(stderr, " %s %.2f", big[i].second.c_str(), big[i].first / 1e9);
      fprintf(stderr, "\n");
    }
    E->stats.h2d_wait_ms = E->h2d_wait_ms;
    E->kg[0].collect(E->stats.check_ms, E->stats.check_bytes, E->stats.check_launches);
    E->kg[1].collect(E->stats.ragged_ms, E->stats.ragged_bytes, E->stats.ragged_launches);
    E->kg[2].collect(E->stats.gather_ms, E->stats.gather_bytes, E->stats.gather_launches);
    {  // B_alg: the in-kernel counters + input / output entries and rows + the label map
      const uint64_t z_in = E->ce.nnz + E->eq.nnz + E->lin.nnz + E->na.nnz + E->nb.nnz + E->nc.nnz;
      const uint64_t r_in = E->ce.n + E->eq.n + E->lin.n + E->na.n;
      const uint64_t z_out = E->out_nnz[0] + E->out_nnz[1] + E->out_nnz[2], r_out = E->out_n_dev;
      const rs_stats &s = E->stats;
      E->stats.alg_bytes = s.elim_bytes + s.big_main_bytes + s.big_finish_bytes + s.apply_bytes + s.round_fill_bytes +
                           s.cluster_bytes + 36 * (z_in + z_out) + 8 * (r_in + r_out) + 8 * S;
    }
    E->have_result = true;
  }
};

// simplification() (constraint_simplification.rs:442-730) on the loaded input, phase by phase
static void engine_run(rs_engine *E, const rs_flags *fl) {
  Run R(E, fl);
  R.init();
  R.eq_simplification();
  R.constant_eq();
  R.setup_non_linear();
  R.linear_round1();
  R.non_linear_frames();
  R.rounds();
  R.assemble();
  R.finish();
}

