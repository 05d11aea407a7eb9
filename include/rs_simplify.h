/*
 * rs_simplify.h -- C ABI of librs_simplify, the MI355X-native R1CS constraint-simplification
 * back end for circom (--O1 / --O2 / --O2round N).
 *
 * This is the drop-in seam.  In the reference (circom 2.2.2, /root/reference) the path is the
 * body of
 *     constraint_list::constraint_simplification::simplification(&mut Simplifier)
 *         -> (ConstraintStorage, SignalMap, usize)
 *     constraint_list/src/constraint_simplification.rs:442-730
 * called only from Simplifier::simplify_constraints (constraint_list/src/lib.rs:131-144).
 * The reference has no FFI and no plugin registry; these entry points are what a Rust shim in
 * constraint_list would bind with `extern "C"` (see INTEGRATION.md for the binding).
 *
 * Conventions
 *   - Field elements are 4 little-endian u64 limbs, canonical (< p).  The field is one of the
 *     eight circom primes (program_structure/src/utils/constants.rs:3-13) or a custom odd prime
 *     < 2^256 (used by tests, e.g. the reference unit tests' F_257).
 *   - Linear combinations are CSR blocks.  Column 0 is the constant-one signal (the reference's
 *     ArithmeticExpression::constant_coefficient(), algebra.rs:155-157).  Within a row the columns
 *     must be distinct; order is free.  Rows must be clean (no zero coefficient), as
 *     DAG::clean_constraints guarantees for every row the reference hands to simplification()
 *     (dag/src/constraint_correctness_analysis.rs:146-157); RS_E_INVALID otherwise.
 *   - All entry points are synchronous and blocking; one call at a time per engine.
 *   - Errors: 0 on success, a negative RS_E_* code otherwise; rs_last_error() explains.  The
 *     reference panics on the same internal invariants (e.g. algebra.rs:1114).
 */
#ifndef RS_SIMPLIFY_H
#define RS_SIMPLIFY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_ABI_VERSION 14

enum rs_status {
  RS_OK = 0,
  RS_E_INVALID = -1,    /* malformed input (shape, unclean row, unknown prime, ...)          */
  RS_E_OOM_DEVICE = -2, /* device allocation failed                                           */
  RS_E_HIP = -3,        /* a HIP runtime call failed                                          */
  RS_E_RCCL = -4,       /* reserved: collective failure (multi-GPU)                           */
  RS_E_INTERNAL = -5,   /* an invariant the reference asserts was violated                    */
  RS_E_NODEVICE = -6    /* no usable gfx950 device: the library never falls back to the CPU   */
};

/* program_structure/src/utils/constants.rs:3-13, the --prime names of circom/src/input_user.rs */
enum rs_prime {
  RS_PRIME_BN128 = 0,
  RS_PRIME_BLS12381 = 1,
  RS_PRIME_GOLDILOCKS = 2,
  RS_PRIME_GRUMPKIN = 3,
  RS_PRIME_PALLAS = 4,
  RS_PRIME_VESTA = 5,
  RS_PRIME_SECQ256R1 = 6,
  RS_PRIME_BLS12377 = 7,
  RS_PRIME_CUSTOM = 255
};

/* One CSR matrix of linear combinations (HashMap<usize, BigInt> per row in the reference). */
typedef struct rs_lc {
  uint64_t n_rows;
  uint64_t nnz;
  uint64_t *ptr; /* n_rows + 1 offsets                                         */
  uint32_t *col; /* nnz signal ids                                             */
  uint64_t *val; /* nnz * 4 limbs (little endian, canonical)                   */
} rs_lc;

/*
 * The Simplifier bundle (constraint_list/src/lib.rs:110-129) as plain arrays.
 *   cons_eq / eq / linear : Simplifier.{cons_equalities, equalities, linear} -- linear rows,
 *                           only their C part (A = B = empty), in the reference's list order
 *                           (DFS order of dag/src/map_to_constraint_list.rs:12-44).
 *   nl_a / nl_b / nl_c    : the non-linear rows of the DAG encoding in EncodingIterator DFS
 *                           order (constraint_list/src/lib.rs:65-108); same n_rows each.
 *   forbidden             : Simplifier.forbidden = {0} u outputs u public inputs u custom-gate
 *                           signals (dag/src/lib.rs:174, 179-204; map_to_constraint_list.rs:22-24).
 */
typedef struct rs_input {
  uint32_t prime_id;     /* enum rs_prime                                                  */
  uint64_t prime[4];     /* only read when prime_id == RS_PRIME_CUSTOM                      */
  uint64_t max_signal;   /* Simplifier.max_signal (= number of labels)                      */
  uint64_t n_pub_out;
  uint64_t n_pub_in;
  uint64_t n_priv_in;
  uint64_t n_forbidden;
  uint32_t *forbidden;
  rs_lc cons_eq;
  rs_lc eq;
  rs_lc linear;
  rs_lc nl_a;
  rs_lc nl_b;
  rs_lc nl_c;
} rs_input;

/* SimplificationFlags (dag/src/lib.rs:546-554) + execution knobs. */
typedef struct rs_flags {
  uint32_t flag_s;             /* --O1: no linear elimination (apply_linear = !flag_s)      */
  uint32_t use_old_heuristics; /* --use_old_simplification_heuristics                        */
  uint64_t no_rounds;          /* UINT64_MAX for --O2, N for --O2round N, 0 for --O1         */
  uint32_t emit_substitution_log; /* --simplification_substitution: fill rs_output.log_*     */
  int32_t device;              /* HIP device ordinal                                        */
} rs_flags;

/*
 * Result: (ConstraintStorage, SignalMap, no_private_inputs_witness) of simplification().
 * Constraints are in storage order with ORIGINAL signal ids (the caller applies label_to_wire,
 * exactly like ConstraintList::r1cs does with apply_correspondence, r1cs_porting.rs:23-33).
 */
typedef struct rs_output {
  uint64_t n_constraints;
  rs_lc a, b, c;                  /* owned by the library; free with rs_output_free         */
  uint64_t n_labels;              /* = max_signal                                           */
  int32_t *label_to_wire;         /* n_labels entries, -1 = not a wire (int32)  */
  uint64_t n_wires;               /* = SignalMap.len()                                      */
  uint64_t no_private_inputs_witness;
  /* The substitution log (--simplification_substitution, constraint_simplification.rs:9-17),
   * only when rs_flags.emit_substitution_log: every Substitution the reference hands to
   * log_substitutions, in its order -- eq_simplification (:249; size-1 clusters, then the others,
   * by cluster index), constant_eq_simplification (:271; row order), then each round's
   * linear_simplification (:320; cluster index order, ascending `from`).  Entry i is
   * log_from[i] := row i of log_to, with ORIGINAL signal ids, keys ascending and the values the
   * reference's `to` map holds (zero values included, e.g. the constant key's {0: 0}). */
  uint64_t n_log;
  uint32_t *log_from;
  rs_lc log_to;
  /* ABI 8: the row layout of a / b / c.  NULL: the block is CSR (row i = [ptr[i], ptr[i+1])), as
   * rs_simplify / rs_engine_fetch return it.  Non-NULL (rs_engine_simplify's streamed result): ptr is
   * NULL and rows are walked in storage order: row i holds {a,b,c}_len[i] & ~RS_ROW_JUMP entries of
   * col / val, starting where row i - 1's ended -- or, when bit 31 (RS_ROW_JUMP) is set, at the next
   * offset of {a,b,c}_jump (row 0 starts at 0 unless it jumps).  The storage rows that were final
   * after the first round went to the host while the later rounds ran and the rest follow them, so
   * col / val may hold entries no row refers to; nnz is the extent of col / val.  rs_rows_begin /
   * rs_rows_next below walk either layout.  (ABI 7 sent a u64 start and a u64 end per row and part:
   * 48 bytes a row on the PCIe link against 12 + a few jumps.) */
  uint32_t *a_len, *b_len, *c_len;
  uint64_t *a_jump, *b_jump, *c_jump;
  uint64_t a_njump, b_njump, c_njump;
} rs_output;

#define RS_ROW_JUMP 0x80000000u
/* The rows of result block q (0 a, 1 b, 2 c) in order, for either layout: rs_rows_begin, then
 * rs_rows_next(&it, r, &beg, &len) for r = 0, 1, 2, ... (a CSR block also allows any order). */
typedef struct rs_rows {
  const rs_lc *L;
  const uint32_t *len;
  const uint64_t *jump;
  uint64_t pos, j;
} rs_rows;
static inline void rs_rows_begin(const rs_output *o, int q, rs_rows *it) {
  it->L = q == 0 ? &o->a : (q == 1 ? &o->b : &o->c);
  it->len = q == 0 ? o->a_len : (q == 1 ? o->b_len : o->c_len);
  it->jump = q == 0 ? o->a_jump : (q == 1 ? o->b_jump : o->c_jump);
  it->pos = 0;
  it->j = 0;
}
static inline void rs_rows_next(rs_rows *it, uint64_t r, uint64_t *beg, uint64_t *len) {
  if (!it->len) {
    *beg = it->L->ptr[r];
    *len = it->L->ptr[r + 1] - it->L->ptr[r];
    return;
  }
  const uint32_t x = it->len[r];
  if (x & RS_ROW_JUMP) it->pos = it->jump[it->j++];
  *beg = it->pos;
  *len = x & ~RS_ROW_JUMP;
  it->pos += *len;
}

/* Phase timings of the last rs_engine_run (milliseconds, HIP events + host clock). */
typedef struct rs_stats {
  double total_ms;             /* device-resident input -> device-resident output             */
  double eq_ms;                /* eq + const-eq renaming                                     */
  double cluster_ms;           /* union-find clustering (all rounds)                         */
  double elim_ms;              /* per-cluster elimination + normalisation + composition      */
  double subst_ms;             /* substitution application (non-linear rows, rounds >= 2)    */
  double final_ms;             /* compaction, rebuild_witness, output assembly               */
  double apply_kernel_ms;      /* device time of the non-linear frames passes (k_frames_wave<0>) */
  uint64_t apply_kernel_launches;
  uint64_t apply_bytes;        /* its algorithmic bytes (sum over launches)                  */
  double elim_kernel_ms;       /* device time of the per-cluster elimination (every kernel)  */
  uint64_t elim_kernel_launches;
  uint64_t elim_bytes;         /* its algorithmic bytes (sum over launches)                  */
  double elim_big_ms;          /* device time of the workgroup kernels (head + tail streams)  */
  double elim_small_ms;        /* device time of the small-cluster kernel (k_eliminate)      */
  double nl_ms;                /* non-linear frames (count, scan, fill, split)               */
  double map_ms;               /* host copy of the non-linear signal map (rounds >= 2)       */
  double rounds_ms;            /* storage updates + bookkeeping of rounds >= 2               */
  double big_prep_ms;          /* k_wide_* + k_big_prep (occurrences + uniques)              */
  double big_main_ms;          /* the ordered elimination loops (k_big_spec<12> + k_big_main<256>) */
  double big_finish_ms;        /* normalisation + composition (k_batch_inv_*, k_big_finish, levels) */
  uint64_t big_main_bytes;     /* algorithmic bytes of the ordered loops (sum over launches)  */
  uint64_t big_finish_bytes;   /* algorithmic bytes of normalisation + composition           */
  uint64_t big_launches;       /* launches of each of the three workgroup kernels            */
  /* Linear-elimination rounds: the reference's calls of linear_simplification
   * (constraint_simplification.rs:613-646), round 1 included, counted also when a round's list holds
   * only rows that turned linear in the round before and came out empty -- LESS the reference's
   * trailing iteration over a list that holds nothing but stale visits: rows an EARLIER round turned
   * linear and emptied, which a later substitution still finds in the never-pruned map[from]
   * (is_linear(empty) holds, so :380-394 list them again and the loop runs once more, over nothing).
   * Finding those visits would mean materialising every map list on the timed path, and such an
   * iteration substitutes nothing: every result equals the reference's, this count can be one lower
   * (it is on most inputs whose later rounds turn rows).  tests/round_cases.py rounds_model restates the
   * definition over pyref. */
  uint64_t rounds;
  uint64_t n_clusters;
  uint64_t n_substitutions;
  uint64_t max_cluster;
  double exchange_ms;          /* sharded runs: the eliminated-signal-map exchange (all rounds) */
  uint64_t exchange_bytes;     /* bytes each rank received + contributed in those collectives  */
  uint64_t world;              /* ranks the elimination was sharded over (1 = single GPU)       */
  /* ABI 4: the ordered elimination loop split into the head (the largest clusters, one launch
   * on the second stream, the critical path) and the tail (every other workgroup cluster), each
   * with its own HIP-event time and in-kernel algorithmic bytes; the storage-row kernel of
   * rounds >= 2; the host -> host legs of rs_engine_simplify. */
  double head_main_ms;         /* k_big_spec<12> (head: the 96 largest clusters)             */
  uint64_t head_main_bytes;
  uint64_t head_launches;
  double tail_main_ms;         /* k_big_main<256> (tail)                                     */
  uint64_t tail_main_bytes;
  uint64_t tail_launches;
  double round_fill_ms;        /* k_frames_wave<1> + k_round_fill (apply_substitution_to_map) */
  uint64_t round_fill_bytes;
  uint64_t round_fill_launches;
  uint64_t alg_bytes;          /* B_alg of the run: every in-kernel counter +
                                  36 (Z_in + Z_out) + 8 (R_in + R_out) + 8 max_signal       */
  double h2d_wait_ms;          /* host time the run spent waiting for input groups to land  */
  double d2h_ms;               /* D2H of the result into the engine's pinned buffers        */
  double host_total_ms;        /* rs_engine_simplify: host input -> host output             */
  double write_ms;             /* ABI 5: the last rs_engine_write_r1cs (device image + file)  */
  /* ABI 8: the rest of the elimination's kernels, each with its HIP-event time (on the stream it runs
   * on) and in-kernel algorithmic bytes, so the per-kernel rooflines cover the GPU time */
  double tail_fin_ms;          /* k_batch_inv_flat + k_big_finish<4>: the tail's normalisation + composition (both groups) */
  uint64_t tail_fin_bytes;
  uint64_t tail_fin_launches;
  double head_fin_ms;          /* the head's k_batch_inv_tree, k_normalize, k_big_finish<8>, Kahn levels, k_big_emit */
  uint64_t head_fin_bytes;
  uint64_t head_fin_launches;
  double small_ms;             /* k_eliminate (clusters under 32 rows, one lane each)               */
  uint64_t small_bytes;
  uint64_t small_launches;
  double prep_ms;              /* the tail's k_big_prep + k_p3_fast (both groups)                    */
  uint64_t prep_launches;
  double cluster_dev_ms;       /* build_clusters on the device (pair sort, union-find, arena replays) */
  uint64_t cluster_bytes;      /* its keys read, (signal, row) pairs written, sorted and linked, per-row arrays */
  uint64_t cluster_launches;
  double giant_ms;             /* the giant path (giant_loop.hpp): component loops of the largest clusters */
  uint64_t giant_bytes;
  uint64_t giant_launches;
  uint64_t giant_merges;        /* merges work = c2*work - c*R the giant path's table loop performed (configs[1]: 21.6 M) */
  double check_ms;             /* the input's device checks (k_check_ptr, k_check_keys, k_sort_validate; copy stream) */
  uint64_t check_bytes;        /* row pointers, keys (+ values: k_sort_validate) read */
  uint64_t check_launches;
  double ragged_ms;            /* CSR -> ragged rows (k_make_ragged) and the linear rows' eq / constant frames */
  uint64_t ragged_bytes;       /* 72 B an entry converted, 77 B an entry framed, + per-row extents */
  uint64_t ragged_launches;
  double gather_ms;            /* the result's gathers: snapshots, late rows, the compact CSR */
  uint64_t gather_bytes;       /* 72 B an entry gathered (read + canonical write) + per-row selection */
  uint64_t gather_launches;
  /* ABI 9: the host's share of the clustering (build_clusters): time the calling thread spent blocked
   * in its read-backs and synchronisations and replaying the largest clusters' arena order, inside the
   * span cluster_dev_ms brackets on the main stream */
  double cluster_host_ms;
  /* ABI 10: the last rs_engine_read_r1cs_o0 -- the whole call; opening the file and streaming the
   * constraint section to the device (until its last chunk has landed); the kernels (from there until
   * the first D2H of the blocks is issued); the blocks' D2H into the page-locked view */
  double read_ms;
  double read_upload_ms;
  double read_kernel_ms;
  double read_d2h_ms;
  /* ABI 11: the last rs_engine_write_sym -- the whole call; until the last input byte has landed on the
   * device (the counting kernel runs under the upload, buffer by buffer); the scan, the totals' read-back
   * and the emitting kernel; the image's D2H and the file (creating it included) */
  double sym_write_ms;
  double sym_in_ms;
  double sym_kernel_ms;
  double sym_out_ms;
} rs_stats;

/* ABI 12: the last rs_engine_write_constraints_json / rs_engine_write_substitution_json on the engine,
 * whichever came last -- the whole call; the upload (the log's; 0 for the constraints file, whose input
 * is resident); both kernel passes, the scans and the read-back of the verdict; the image's D2H and the
 * file (creating it included).  in_ms + kernel_ms + out_ms = write_ms.  bytes: the image, the file
 * without its opening and closing strings. */
typedef struct rs_json_stats {
  double write_ms;
  double in_ms;
  double kernel_ms;
  double out_ms;
  uint64_t bytes;
} rs_json_stats;

typedef struct rs_engine rs_engine;

const char *rs_last_error(void);
int rs_abi_version(void);

/* One-shot: host input -> host output (H2D, simplification on the GPU, D2H). */
int rs_simplify(const rs_input *in, const rs_flags *fl, rs_output **out);
void rs_output_free(rs_output *out);

/* Engine API used by the benchmark: stage the input in HBM once, run many times. */
int rs_engine_create(int device, rs_engine **eng);
int rs_engine_load(rs_engine *eng, const rs_input *in);   /* H2D copy of the host input        */
int rs_engine_run(rs_engine *eng, const rs_flags *fl);    /* the timed region                   */
int rs_engine_fetch(rs_engine *eng, rs_output **out);     /* D2H of the last result             */
int rs_engine_stats(rs_engine *eng, rs_stats *st);
void rs_engine_destroy(rs_engine *eng);

/*
 * Host -> host on a persistent engine: the whole of simplification() (constraint_simplification.rs
 * :442-730) from the host CSR blocks to the host result, the SURVEY 8(d) T_simplify region.
 * The H2D copy of `in` runs on a copy stream in three groups (cons_eq + eq, linear, non-linear),
 * each validated on the device as it lands, and the simplification consumes a group as soon as it
 * is there, so the upload of the later groups overlaps the eq / clustering / elimination phases.
 * The result is copied into pinned buffers the engine owns; *out points at them and stays valid
 * until the next call on `eng` or rs_engine_destroy (do not rs_output_free it).  `in` is read
 * only during the call.  Host buffers from rs_host_alloc move at full PCIe speed; pageable ones
 * work too (HIP stages them), slower.
 * The values of `eq` are never uploaded: values of `eq` rows the run eliminates are not inspected by
 * rs_engine_simplify (the reference does not read them either).  A row it keeps -- both ends forbidden,
 * a cluster of its own -- takes its values from `in` and is RS_E_INVALID when one is zero or >= p.
 * rs_engine_load and rs_simplify validate every value of `eq`.
 */
int rs_engine_simplify(rs_engine *eng, const rs_input *in, const rs_flags *fl, const rs_output **out);

/* The engine's last result written as a .r1cs (constraint_list/src/r1cs_porting.rs:4-124; SURVEY
 * 8(f) rank 2): byte-identical to rs_write_r1cs on the fetched output, with the constraint section
 * (wire correspondence + LE-byte key order per row) built on the device and streamed to the file.
 * o0_r1cs (may be NULL): copy its custom-gate sections like rs_write_r1cs_gates.  Time in
 * rs_stats.write_ms. */
int rs_engine_write_r1cs(rs_engine *eng, const char *path, const char *o0_r1cs);

/* Page-locked host memory (hipHostMalloc) for the CSR blocks a caller marshals the Simplifier into,
 * so rs_engine_simplify's H2D runs at PCIe speed.  NULL without a device. */
void *rs_host_alloc(uint64_t bytes);
void rs_host_free(void *p);

/*
 * Multi-GPU: ONE circuit sharded over W ranks.  Every rank loads the same input;
 * the global phases (eq / const-eq renaming, build_clusters) run on every rank, the clusters are
 * dealt to the ranks by size (snake order), each rank eliminates its own, and the eliminated-signal
 * map (substitutions, leftovers, their pool entries) is exchanged after every round -- RCCL over
 * xGMI in production.  Every rank ends with the complete, identical output (byte-identical to a
 * single-GPU run).  Join before rs_engine_run; all ranks must run with the same flags.
 *
 * RCCL, one process per GPU (what bench.py does under torch.distributed.run):
 *   rank 0: rs_comm_unique_id(id); broadcast the RS_COMM_ID_BYTES bytes to the other ranks;
 *   every rank: rs_engine_join_rccl(eng, world, rank, id)   (collective: blocks until all joined)
 * In one process (threads; a device may be listed twice, e.g. to test on one GPU):
 *   g = rs_group_create(world); rank r's thread: rs_engine_join_group(eng_r, g, r); ...
 *   rs_group_destroy(g) after every engine of the group is destroyed.
 * rs_simplify_multi: the one-shot entry point over n_devices GPUs of this process (threads; RCCL
 * when the devices are distinct, the in-process transport otherwise).
 */
#define RS_COMM_ID_BYTES 128
typedef struct rs_group rs_group;
int rs_comm_unique_id(uint8_t id[RS_COMM_ID_BYTES]);
int rs_engine_join_rccl(rs_engine *eng, int world, int rank, const uint8_t id[RS_COMM_ID_BYTES]);
rs_group *rs_group_create(int world);
int rs_engine_join_group(rs_engine *eng, rs_group *g, int rank);
void rs_group_destroy(rs_group *g);
int rs_simplify_multi(const rs_input *in, const rs_flags *fl, int n_devices, const int *devices, rs_output **out);
/* ABI 9, a test transport: the ranks are processes of one host (e.g. two processes on ONE GPU, where RCCL
 * refuses a second rank), their collectives staged through POSIX shared memory; every rank passes the
 * same `tag` (a name for the group's control block).  The shared result region is made exactly as for
 * RCCL ranks, so the one-GPU box runs the multi-process result path (shared host memory mapped and
 * registered by every process, each rank's share streamed into it). */
int rs_engine_join_host(rs_engine *eng, int world, int rank, const char *tag);

/* Fault injection (tests; SURVEY 5 "failure detection / fault injection"): the engine's next
 * rs_engine_run / rs_engine_simplify fails with RS_E_INTERNAL at `where` (1: the start of the first
 * linear elimination round, after the run's first collectives; 0: cancel).  A failure belongs to the
 * call it happens in: the other ranks of an in-process group leave that call with RS_E_RCCL, and the
 * group runs the ranks' next calls normally.  RCCL ranks are not released (a failed rank there ends
 * the job). */
int rs_engine_inject_fault(rs_engine *eng, int where);

/* --O0 .r1cs -> rs_input (host arrays owned by the library; free with rs_input_free).
 * Classifies rows exactly like dag/src/map_to_constraint_list.rs:12-44.  The signals of the
 * custom-gate applications (section 5, dag/src/r1cs_porting.rs:74-107) join `forbidden`, as
 * map_tree inserts them (map_to_constraint_list.rs:22-24).  Every read is bounds-checked against
 * its section and the file: a truncated or malformed file is RS_E_INVALID. */
int rs_read_r1cs_o0(const char *path, rs_input **in);
void rs_input_free(rs_input *in);
/* ABI 10: the same read on the device.  The result equals rs_read_r1cs_o0's field for
 * field and array for array (rows and entries in file order, values widened to four limbs), and a file
 * rs_read_r1cs_o0 refuses is RS_E_INVALID here too.  The host parses the section table, the header and
 * the custom-gate sections; the constraint section goes to the device untouched (streamed through
 * pinned staging buffers), where the linear combinations' boundaries are found in parallel and the rows
 * classified and copied into the six blocks.  A constraint section of 16 GiB or more is RS_E_INVALID
 * (positions are stored in 32 bits).  RS_E_NODEVICE without a gfx950 device: there is no CPU fallback.
 * rs_engine_read_r1cs_o0: into the page-locked buffers rs_engine_flatten_dag uses (one set, shared):
 * *in views them, valid until the next rs_engine_read_r1cs_o0 or rs_engine_flatten_dag on `eng` or
 * rs_engine_destroy (do not rs_input_free it), and feeds rs_engine_simplify's H2D at full speed.
 * rs_read_r1cs_o0_device: the one-shot (makes and destroys an engine); arrays freed by rs_input_free. */
int rs_engine_read_r1cs_o0(rs_engine *eng, const char *path, const rs_input **in);
int rs_read_r1cs_o0_device(int device, const char *path, rs_input **in);
/* Writes the simplified .r1cs (constraint_list/src/r1cs_porting.rs:4-124). */
int rs_write_r1cs(const char *path, const rs_input *in, const rs_output *out);
/* The same, plus the --O0 file's custom-gate sections as the O2 writer re-emits them
 * (r1cs_porting.rs:54-121): section 4 unchanged, section 5 with its signals mapped label -> wire
 * (5 sections in all).  Without sections 4/5 in `o0_r1cs` the output equals rs_write_r1cs's. */
int rs_write_r1cs_gates(const char *path, const rs_input *in, const rs_output *out, const char *o0_r1cs);
/* Rewrites an --O0 .sym with the witness column of `out` (constraint_list/src/sym_porting.rs). */
int rs_write_sym(const char *o0_sym, const char *path, const rs_output *out);
/* ABI 11: the same rewrite on the device: the engine's last result -- its label_to_wire is
 * resident after a run -- applied to the --O0 .sym at o0_sym and written to path.  The file is streamed to
 * the device through pinned staging buffers, column 2 of every line is replaced there by
 * label_to_wire[column 1] (csrc/sym_write.hpp; no line table: every byte finds its place from the 23
 * bytes before it and one prefix sum), and the image leaves through the buffers and pwrite threads of
 * rs_engine_write_r1cs.  Positions are 64-bit; both images are resident on the device (RS_E_OOM_DEVICE if
 * they do not fit).
 * The accepted grammar: every non-empty line is `L,W,rest` with
 *   L    = 0|[1-9][0-9]{0,9}   (parsed in 64 bits; L >= n_labels writes -1, as rs_write_sym does)
 *   W    = -?[0-9]{1,10}
 *   rest = any bytes but '\n' (may be empty, may hold commas and digits)
 * and no byte of the file is NUL.  Empty lines are dropped, a last line without '\n' gets one, an empty
 * file gives an empty file.  For every such file the output equals rs_write_sym's byte for byte.
 * Anything else is RS_E_INVALID -- deliberately stricter than the host: every line rs_write_sym refuses
 * (fewer than two commas), and the inputs on which its strtoull / %s would silently differ from a byte
 * copy (leading zeros or blanks in L, a non-numeric L, an L of 11 or more digits, an empty or
 * non-numeric W, a NUL).  Validation finishes before `path` is opened: a refused input leaves no
 * output file, and the engine stays usable.
 * RS_E_INVALID too for a null argument and for an engine without a result (like rs_engine_write_r1cs).
 * RS_WRITER_HOST (environment) routes rs_engine_write_sym to rs_write_sym over the fetched
 * label_to_wire, as it does for rs_engine_write_r1cs.  On a sharded engine, as rs_engine_write_r1cs:
 * every rank holds the complete label_to_wire after a run, so any rank may call it (it is no collective)
 * and writes the whole file.  RS_E_NODEVICE without a gfx950 device: there is no CPU fallback.
 * Times in rs_stats.sym_*.
 * rs_write_sym_device: the one-shot (makes and destroys an engine); of `out` it reads ONLY n_labels and
 * label_to_wire. */
int rs_engine_write_sym(rs_engine *eng, const char *o0_sym, const char *path);
int rs_write_sym_device(int device, const char *o0_sym, const char *path, const rs_output *out);
/* --json: <prefix>_constraints.json (constraint_list/src/json_porting.rs:36-48 port_constraints,
 * constraint_writers/src/json_writer.rs:4-45 ConstraintJSON): the rows in storage order with the
 * witness correspondence applied, keys ascending, decimal values. */
int rs_write_constraints_json(const char *path, const rs_output *out);
/* --simplification_substitution: <prefix>_substitutions.json (json_porting.rs:28-33
 * port_substitution, json_writer.rs:94-131 SubstitutionJSON) from out->log_*, original ids. */
int rs_write_substitution_json(const char *path, const rs_output *out);
/* ABI 12: the same two files written on the device (csrc/json_write.hpp): every entry's text length is
 * known from its own 36 bytes, one prefix sum per part places every byte, a workgroup per chunk of
 * RS_JSON_CHUNK output bytes (a power of two, rounded down, 64 .. 65536; read on every call) converts the
 * values (256-bit binary -> decimal) and builds its piece of the image, and the image leaves through the
 * buffers and pwrite threads of rs_engine_write_r1cs.  Positions are 64-bit; the image is resident on the
 * device (RS_E_OOM_DEVICE if it does not fit).
 * rs_engine_write_constraints_json reads the engine's resident result (what rs_engine_write_r1cs reads)
 * and writes the bytes rs_write_constraints_json writes over rs_engine_fetch's output.
 * rs_engine_write_substitution_json sends the engine's substitution log up through pinned staging buffers
 * and writes the bytes rs_write_substitution_json writes over the fetched output; after a run without
 * rs_flags.emit_substitution_log that is `{\n}`.
 * The one-shots make and destroy an engine and upload what they need of `out`:
 * rs_write_constraints_json_device reads n_constraints, a / b / c with their {a,b,c}_len / {a,b,c}_jump
 * arrays, n_labels and label_to_wire; rs_write_substitution_json_device reads ONLY n_log, log_from and
 * log_to.  Both accept either row layout: the rs_output rs_engine_simplify returns works as it is.
 * The contract: the device output equals the host writer's byte for byte for every rs_output whose row
 * parts have strictly ascending mapped keys (label_to_wire[col] in the constraints file, col in the log)
 * -- every result of this library does: rows hold sorted distinct keys and label_to_wire is the
 * order-preserving rank of the kept signals.  A row part out of order (or with a key twice) is
 * RS_E_INVALID -- deliberately stricter than the host, which sorts.  A key at or past n_labels, or one
 * whose label_to_wire is negative ("constraint mentions a removed signal"), is RS_E_INTERNAL, as with the
 * host writer, and wins over the order error.  Malformed row pointers or a row layout that reaches past
 * the block's entries are RS_E_INVALID.  The verdict is known after the first kernel pass and one
 * read-back, before `path` is opened: a refused call leaves no file, and the engine stays usable.
 * RS_E_INVALID too for a null argument and for an engine without a result.  RS_WRITER_HOST (environment)
 * routes both engine calls to the host writers over the fetched result.  On a sharded engine every rank
 * holds the whole result and the whole log after a run, so any rank may call them (they are no
 * collectives) and writes the whole file.  RS_E_NODEVICE without a gfx950 device: there is no CPU
 * fallback.  Times in rs_json_stats (rs_engine_json_stats); rs_stats is unchanged. */
int rs_engine_write_constraints_json(rs_engine *eng, const char *path);
int rs_engine_write_substitution_json(rs_engine *eng, const char *path);
int rs_write_constraints_json_device(int device, const char *path, const rs_output *out);
int rs_write_substitution_json_device(int device, const char *path, const rs_output *out);
int rs_engine_json_stats(rs_engine *eng, rs_json_stats *st);

/* ---- ABI 13: the witness.  A .wtns file (what the reference's generated programs write:
 * code_producers/src/c_elements/common/main.cpp writeBinWitness, and the wasm witness_calculator.js)
 * read, checked against the circuit and the result, and projected onto the result's wires.  At --O0
 * wires equal labels, so the user's witness generator writes one value per label; after --O1 / --O2 the
 * .r1cs is numbered by wire and label_to_wire says which values stay.
 * File format, all integers little endian: `wtns`, u32 version = 2, u32 nSections, then sections
 * (u32 id, u64 length, body): id 1 = u32 n8, the prime in n8 bytes, u32 nVars; id 2 = nVars values of
 * n8 bytes, each canonical.  n8 is the .r1cs header's field size (8 for goldilocks, 32 for the 256-bit
 * primes).
 * rs_witness: n values of 4 limbs (canonical, little endian, like rs_lc.val); prime[] is always filled,
 * prime_id is RS_PRIME_CUSTOM when the prime is none of the eight; n8 is the file's value width. */
typedef struct rs_witness {
  uint32_t prime_id;
  uint64_t prime[4];
  uint32_t n8;
  uint64_t n;
  uint64_t *val;
} rs_witness;

#define RS_WIT_INPUT 1u  /* the rows of the caller's rs_input (four classes)  */
#define RS_WIT_OUTPUT 2u /* the rows of the result                            */
#define RS_WIT_LOG 4u    /* the entries of the substitution log               */
/* The classes of rs_witness_report, in order. */
enum rs_witness_class {
  RS_WITC_CONS_EQ = 0, /* rs_input.cons_eq: holds iff C.w = 0                       */
  RS_WITC_EQ = 1,      /* rs_input.eq: C.w = 0                                      */
  RS_WITC_LINEAR = 2,  /* rs_input.linear: C.w = 0                                  */
  RS_WITC_NONLINEAR = 3, /* rs_input.nl_{a,b,c}: (A.w)(B.w) - C.w = 0               */
  RS_WITC_OUTPUT = 4,  /* rs_output.{a,b,c}: (A.w)(B.w) - C.w = 0                   */
  RS_WITC_LOG = 5,     /* log entry i: w[log_from[i]] = log_to[i].w                 */
  RS_WITC_COUNT = 6
};
/* Per class: the rows evaluated (0 for a class not asked for), how many do not hold, and the smallest
 * failing index within the class (UINT64_MAX when none failed).  in_ms: the uploads (the caller's input,
 * the log); kernel_ms: the evaluation; total_ms: the whole call.  The host check leaves in_ms 0. */
typedef struct rs_witness_report {
  uint64_t checked[6], failed[6], first_failed[6];
  double in_ms, kernel_ms, total_ms;
} rs_witness_report;

/* Reads a .wtns (library-owned arrays: rs_witness_free).  Sections are found by walking the section
 * table; unknown ids are skipped; sections 1 and 2 come in either order.  RS_E_INVALID, with a message
 * naming the cause, for: bad magic; a version other than 2; a missing or duplicated section 1 or 2; a
 * section running past the file; n8 no multiple of 8 or outside 8..32; section 1 not 8 + n8 bytes; a
 * prime that is even or below 3; section 2's length not n8 * nVars; a value >= the prime.  Every size is
 * checked before the allocation it guards. */
int rs_read_wtns(const char *path, rs_witness **w);
void rs_witness_free(rs_witness *w);
/* Writes a .wtns.  out == NULL: `w` as it is.  Otherwise the projection onto the result's wires:
 * out->n_wires values, value label_to_wire[s] = w[s] for every label s with a wire; of `out` only
 * label_to_wire, n_labels and n_wires are read, so either row layout works.  RS_E_INVALID for a null
 * argument, a bad n8 or prime, a value >= the prime, w->n != out->n_labels or a wire >= n_wires.
 * (rs_output carries no prime: the engine call below is the one that refuses a witness of another field.) */
int rs_write_wtns(const char *path, const rs_witness *w, const rs_output *out);
/* The host evaluation of a witness, in plain 256-bit host arithmetic (csrc/wtns_io.hpp): `what` is an OR
 * of RS_WIT_*; `in` may be NULL without RS_WIT_INPUT, `out` without RS_WIT_OUTPUT and RS_WIT_LOG.  Key 0
 * is the constant.  Returns RS_OK whenever the evaluation ran: rows that do not hold are a finding in
 * `rep`, not an error.  RS_E_INVALID for: a null argument that is needed; w[0] != 1; a value >= the
 * prime; w->n != in->max_signal (RS_WIT_INPUT) or != out->n_labels (RS_WIT_OUTPUT, RS_WIT_LOG); a
 * witness prime that is not the input's; malformed row pointers; a key >= w->n.  `out` in either row
 * layout.  Coefficients are taken as canonical (every input and result of this library is). */
int rs_check_witness(const rs_input *in, const rs_output *out, const rs_witness *w, uint32_t what, rs_witness_report *rep);
/* The same on the device (csrc/witness.hpp).  rs_engine_load_witness / rs_engine_load_wtns make a witness
 * resident on the engine until the next load (in the writers' arena: nothing of a result moves); load_wtns
 * parses the two small header pieces on the host and streams section 2 through the pinned staging
 * buffers, each widened, range-checked (value >= the prime, w[0] != 1: RS_E_INVALID, nothing stays
 * resident) and stored in Montgomery form behind its copy.  A load needs neither an input nor a result.
 * rs_engine_check_witness evaluates the resident witness: RS_WIT_INPUT over the caller's `in` (host
 * arrays, uploaded block by block; the engine's own copy of a loaded input is not read), RS_WIT_OUTPUT
 * over the last result's resident rows, RS_WIT_LOG over the last run's substitution log.  One evaluator
 * serves all: a workgroup per chunk of RS_WIT_CHUNK consecutive entries of a part (a power of two,
 * rounded down, 64 .. 8192, default 1024; read on every call), a segmented sum per row, rows that cross a chunk border
 * summed from per-chunk partials in chunk order; no atomics on field values, so the report is
 * deterministic and equals rs_check_witness's over the fetched result.
 * RS_E_INVALID for: a null argument; no resident witness; RS_WIT_INPUT without `in`; RS_WIT_OUTPUT or
 * RS_WIT_LOG without a result; RS_WIT_LOG after a run without rs_flags.emit_substitution_log; a witness
 * whose n is not the labels of what is checked, or whose prime is not its prime; malformed row pointers
 * of `in`; a key >= the labels.  The engine stays usable after each.  On a sharded engine every rank
 * checks its own complete copy (no collective), like rs_engine_write_r1cs.
 * rs_engine_write_wtns: the resident witness projected onto the last result's wires, the bytes
 * rs_write_wtns(path, w, fetched output) writes; the image is built on the device (a lane per label with
 * a wire stores its value, canonical and narrowed to n8 bytes, at n8 * label_to_wire[s]) and leaves
 * through the buffers and pwrite threads of rs_engine_write_r1cs.  RS_E_INVALID without a result, without
 * a witness, or for a witness of another size or prime.  RS_E_NODEVICE without a gfx950 device. */
int rs_engine_load_witness(rs_engine *eng, const rs_witness *w);
int rs_engine_load_wtns(rs_engine *eng, const char *path);
int rs_engine_check_witness(rs_engine *eng, const rs_input *in, uint32_t what, rs_witness_report *rep);
int rs_engine_write_wtns(rs_engine *eng, const char *path);

/* ---- ABI 14: the lift.  The way back from a witness of the simplified circuit (one value per wire, what
 * the witness generator compiled with the --O1 / --O2 circuit writes) to one value per --O0 label, through
 * the substitution log: entry i says w[log_from[i]] = log_to[i] . w.
 * Inputs: a result with L = n_labels, Wn = n_wires, label_to_wire, and a log of n entries (original ids,
 * ascending keys); a wire witness v with v.n == Wn, canonical values and v[0] == 1.
 * Owner: owner(s) is the largest i with log_from[i] == s, or none (constant_eq_simplification logs every
 * row; the map keeps the last).  An entry that is not the owner of its `from` is shadowed: it defines
 * nothing, creates no dependency, and is counted.
 * Values: w[s] = v[label_to_wire[s]] when label_to_wire[s] >= 0; otherwise log_to[owner(s)] . w when s has
 * an owner; otherwise 0 (a free label, counted: it was never constrained, or sat in a part that
 * vanished).  Key 0 is the constant.  A key with coefficient 0 still counts as a key: dependencies follow
 * key presence.
 * Level: an owner entry i has level 0 when no key of log_to[i] has an owner, otherwise 1 + the largest
 * level of its owned keys' owners.  `levels` is 1 + the deepest level, 0 without owner entries.  A level-l
 * entry reads only wire values, free zeros and values of levels < l.
 * RS_E_INVALID, with a message naming the cause, nothing produced (*w stays NULL), the engine usable and
 * its wire witness still resident, for: a null argument; v.n != Wn; a witness prime that is not the
 * result's (engine calls only: rs_output carries no prime); v[0] != 1 or a value >= the prime;
 * log_from[i] >= L, == 0, or a label that still has a wire; a key >= L; malformed log row pointers; an
 * owner entry i with a key whose owner is j <= i (the log is not in elimination order; an entry whose `to`
 * holds its own `from` is one); on the engine: no result, no resident witness, or a last run without
 * rs_flags.emit_substitution_log. */
typedef struct rs_lift_report {
  uint64_t n_labels, n_wires;
  uint64_t lifted;      /* labels an owner entry defines          */
  uint64_t free_labels; /* no wire, no entry: value 0             */
  uint64_t shadowed;    /* entries whose `from` a later one owns  */
  uint64_t levels;      /* 1 + the deepest level; 0 without owners */
  uint64_t entries;     /* (key, value) pairs evaluated: the owner entries' */
  double in_ms, kernel_ms, total_ms;   /* host twin: in_ms = kernel_ms = 0 */
} rs_lift_report;
/* The host twin and the oracle (csrc/wtns_io.hpp, plain 256-bit host arithmetic): owners in one forward
 * pass, the entries evaluated in one pass from the last index to the first, which the order rule makes
 * exact.  `out` in either row layout: only n_labels, n_wires, label_to_wire, n_log, log_from and log_to
 * are read.  *w: library-owned (rs_witness_free), n = L, n8 and the prime as v's. */
int rs_lift_witness(const rs_output *out, const rs_witness *v, rs_witness **w, rs_lift_report *rep);
/* The same on the device (csrc/lift.hpp), as a one-shot: an engine for the call, what is read of `out`
 * and `v` uploaded, the values returned like rs_lift_witness's. */
int rs_lift_witness_device(int device, const rs_output *out, const rs_witness *v, rs_witness **w, rs_lift_report *rep);
/* Replaces the engine's resident wire witness (n = n_wires of the last result) with the lifted one (n = L,
 * same arena: nothing of the result moves); rs_engine_check_witness and rs_engine_write_wtns then work on
 * it unchanged.  The log goes up once; owners by a 64-bit integer atomicMax, the levels by repeated
 * entry-parallel passes (one changed-flag read back per pass), one stable radix sort of the owner rows by
 * level and one scan of their lengths (the virtual row pointers of all levels), then per level the
 * evaluator of rs_engine_check_witness over the level's rows (RS_WIT_CHUNK) and a lane per row that stores
 * w[from]: 2 launches a level.  No atomics on field values: values and report equal rs_lift_witness's.  The
 * resident witness is replaced only after the last error word reads clean.  On a sharded engine every
 * rank lifts its own complete copy (no collective). */
int rs_engine_lift_witness(rs_engine *eng, rs_lift_report *rep);
/* The resident witness, canonical, in library-owned arrays (rs_witness_free); n8 and the prime as loaded. */
int rs_engine_fetch_witness(rs_engine *eng, rs_witness **w);
/* The resident witness as it is (no projection): the bytes rs_write_wtns(path, w, NULL) writes; the image
 * is built on the device and leaves through the buffers and pwrite threads of rs_engine_write_r1cs. */
int rs_engine_write_wtns_resident(rs_engine *eng, const char *path);

/* Seeded synthetic --O0 systems for benchmarks/tests (see DESIGN.md "Workloads").
 * kind: 0 = mixed (metric circuit, BASELINE configs[4]), 1 = purely linear (configs[1]), 2 = chain
 * (configs[3] ECDSA stand-in: deep composition, 8 rounds), 3 = Poseidon(16) Merkle (configs[2]),
 * 4 = sha256-like bit gadgets (configs[0]), 5 = templated (64-row template instances replicated with
 * signal offsets, wired into chains; SURVEY 8(d) config 5's replication), 6 = templated whose first
 * chain has 9,000 instances (one ~2e5-row linear cluster: config 5's replication and its tail). */
int rs_synth(uint32_t kind, uint64_t rows, uint64_t seed, uint32_t prime_id, rs_input **in);

/* ---- the DAG -> constraint-list flattening that produces rs_input.
 * Replaces dag::map_to_constraint_list::map's walk (dag/src/map_to_constraint_list.rs:12-44 map_tree,
 * :111-150 map) and the non-linear rows of the EncodingIterator DFS (constraint_list/src/lib.rs:65-108,
 * state_utils.rs:14-35): every component instance in DFS order from main (offset 0), its local
 * signals appended to the witness list, its constraints with the instance offset applied (key 0 stays
 * the constant) and classified like map_tree -- constant equality, equality, linear (empty
 * constraints only in main; Tree::go_to_subtree drops them), else non-linear.  Custom-gate
 * instances' signals join main's forbidden_if_main.  Instance expansion and the constraint copy run
 * on the device (prefix sums over the instance tree); the per-template classification is a host
 * pass over the templates.  The result is an ordinary rs_input (freed with rs_input_free). */
typedef struct rs_dag {
  uint32_t prime_id;           /* enum rs_prime                                                 */
  uint64_t prime[4];           /* only read when prime_id == RS_PRIME_CUSTOM                     */
  uint64_t n_pub_out, n_pub_in, n_priv_in;
  uint64_t n_forbidden;        /* main's forbidden_if_main (main's offset is 0: global ids)      */
  const uint32_t *forbidden;
  uint32_t n_nodes;            /* DAG nodes (templates with their parameters)                   */
  uint32_t main_node;
  const uint64_t *cons_off;    /* [n_nodes + 1]: node -> its constraints, rows of a / b / c       */
  rs_lc a, b, c;               /* every node's constraints, node-local ids (0 = the constant)     */
  const uint64_t *local_off;   /* [n_nodes + 1]: node -> its local signals                        */
  const uint32_t *locals;      /* node-local ids of the node's own signals, ascending             */
  const uint8_t *custom_gate;  /* [n_nodes]                                                       */
  const uint64_t *edge_off;    /* [n_nodes + 1]: node -> its edges, in adjacency order            */
  const uint32_t *edge_to;     /* child node                                                      */
  const uint64_t *edge_in;     /* the edge's in_number: the child's signal offset in the parent   */
} rs_dag;
/* device: the GPU to run on.  Rejects (RS_E_INVALID) a cyclic graph, an edge to a missing node,
 * malformed CSR blocks (ptr[0] != 0, decreasing pointers, ptr[T] != nnz) and a graph whose offset
 * signal ids (instance offset + node-local id) or signal count reach 2^31. */
int rs_flatten_dag(int device, const rs_dag *dag, rs_input **in);
/* The same on a persistent engine (its device buffers stay allocated across calls), into page-locked
 * buffers the engine owns, so the blocks' D2H runs at PCIe speed and the result feeds
 * rs_engine_simplify's H2D at full speed too.  *in views those buffers: valid until the next
 * rs_engine_flatten_dag or rs_engine_read_r1cs_o0 on `eng` or rs_engine_destroy (do not
 * rs_input_free it). */
int rs_engine_flatten_dag(rs_engine *eng, const rs_dag *dag, const rs_input **in);

#ifdef __cplusplus
}
#endif
#endif /* RS_SIMPLIFY_H */
