// cli.cpp -- circom-simplify: the drop-in seam exercised from files.
//
//   circom-simplify <in_O0.r1cs> [<in_O0.sym>] --O1|--O2|--O2round N
//                   [--use_old_simplification_heuristics] [--json] [--simplification_substitution]
//                   [--wtns <in_O0.wtns>] [--device D] [--host-reader] -o <out_prefix>
//
// Reads an --O0 export (which losslessly holds what simplification() consumes, SURVEY CS-4),
// runs the GPU back end and writes <out_prefix>.r1cs (+ .sym), like `circom --r1cs --sym` at the
// given level (circom/src/input_user.rs:286-306 for the flag semantics); --json adds
// <out_prefix>_constraints.json and --simplification_substitution <out_prefix>_substitutions.json
// (the file names circom derives from its output base, input_user.rs).
//
// The --O0 file is read and classified on the device (rs_engine_read_r1cs_o0) and simplified on the
// same engine (rs_engine_simplify); --host-reader reads it with rs_read_r1cs_o0 and runs the one-shot
// rs_simplify instead.  On the engine path the .sym is rewritten on the device too (rs_engine_write_sym,
// from the label_to_wire the run left there; it accepts the `L,W,rest` lines circom writes, see the
// header); --host-reader keeps rs_write_sym.  The --json and --simplification_substitution files are
// formatted on the device as well on the engine path (rs_engine_write_constraints_json,
// rs_engine_write_substitution_json, from the result and the log the run left with the engine);
// --host-reader keeps rs_write_constraints_json / rs_write_substitution_json.  The files and the summary
// are the same bytes either way.
//
// --wtns <in_O0.wtns>: the witness the --O0 circuit's generator wrote (one value per label; at --O0 wires
// equal labels, SURVEY CS-4).  After the files are written it is checked on the input rows, the output rows
// and -- with --simplification_substitution -- the substitution log, and its projection onto the result's
// wires is written to <out_prefix>.wtns, the witness that fits <out_prefix>.r1cs.  On the engine path the
// witness is streamed to the device, evaluated and projected there (rs_engine_load_wtns,
// rs_engine_check_witness, rs_engine_write_wtns); --host-reader uses rs_read_wtns, rs_check_witness and
// rs_write_wtns: the same file and the same messages.  An input row that fails means the witness is not one
// of this circuit: exit status 3, no .wtns.  The input holding but an output row or log entry failing is a
// simplifier bug: exit status 4, no .wtns.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/rs_simplify.h"

int main(int argc, char **argv) {
  const char *in_r1cs = nullptr, *in_sym = nullptr, *in_wtns = nullptr;
  std::string out;
  bool json = false, host_reader = false;
  rs_flags fl;
  memset(&fl, 0, sizeof(fl));
  fl.flag_s = 1;  // --O1 is circom's default since 2.2.0 (input_user.rs:304)
  fl.no_rounds = 0;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "--O1") { fl.flag_s = 1; fl.no_rounds = 0; }
    else if (a == "--O2") { fl.flag_s = 0; fl.no_rounds = UINT64_MAX; }
    else if (a == "--O2round" && i + 1 < argc) {
      uint64_t n = strtoull(argv[++i], nullptr, 10);
      if (n == 0) { fl.flag_s = 1; fl.no_rounds = 0; }
      else { fl.flag_s = 0; fl.no_rounds = n; }
    } else if (a == "--use_old_simplification_heuristics") fl.use_old_heuristics = 1;
    else if (a == "--json") json = true;
    else if (a == "--host-reader") host_reader = true;
    else if (a == "--simplification_substitution") fl.emit_substitution_log = 1;
    else if (a == "--wtns" && i + 1 < argc) in_wtns = argv[++i];
    else if (a == "--device" && i + 1 < argc) fl.device = atoi(argv[++i]);
    else if (a == "-o" && i + 1 < argc) out = argv[++i];
    else if (!in_r1cs) in_r1cs = argv[i];
    else if (!in_sym) in_sym = argv[i];
    else { fprintf(stderr, "unexpected argument %s\n", argv[i]); return 2; }
  }
  if (!in_r1cs || out.empty()) {
    fprintf(stderr, "usage: circom-simplify in_O0.r1cs [in_O0.sym] --O1|--O2|--O2round N [--json] "
                    "[--simplification_substitution] [--wtns in_O0.wtns] [--host-reader] -o out_prefix\n");
    return 2;
  }
  // (`in` and `o` are the library's either way: owned by the engine, or freed below)
  const rs_input *in = nullptr;
  const rs_output *o = nullptr;
  rs_input *in_own = nullptr;
  rs_output *o_own = nullptr;
  rs_engine *eng = nullptr;
  std::chrono::steady_clock::time_point t0, t1;
  if (host_reader) {
    if (rs_read_r1cs_o0(in_r1cs, &in_own)) { fprintf(stderr, "error: %s\n", rs_last_error()); return 1; }
    in = in_own;
    t0 = std::chrono::steady_clock::now();
    int rc = rs_simplify(in, &fl, &o_own);
    t1 = std::chrono::steady_clock::now();
    if (rc) { fprintf(stderr, "error %d: %s\n", rc, rs_last_error()); rs_input_free(in_own); return 1; }
    o = o_own;
  } else {
    int rc = rs_engine_create(fl.device, &eng);
    if (!rc) rc = rs_engine_read_r1cs_o0(eng, in_r1cs, &in);
    if (rc) { fprintf(stderr, "error: %s\n", rs_last_error()); rs_engine_destroy(eng); return 1; }
    t0 = std::chrono::steady_clock::now();
    rc = rs_engine_simplify(eng, in, &fl, &o);
    t1 = std::chrono::steady_clock::now();
    if (rc) { fprintf(stderr, "error %d: %s\n", rc, rs_last_error()); rs_engine_destroy(eng); return 1; }
  }
  if (rs_write_r1cs_gates((out + ".r1cs").c_str(), in, o, in_r1cs)) { fprintf(stderr, "error: %s\n", rs_last_error()); return 1; }
  if (in_sym && (eng ? rs_engine_write_sym(eng, in_sym, (out + ".sym").c_str()) : rs_write_sym(in_sym, (out + ".sym").c_str(), o))) { fprintf(stderr, "error: %s\n", rs_last_error()); return 1; }
  if (json && (eng ? rs_engine_write_constraints_json(eng, (out + "_constraints.json").c_str()) : rs_write_constraints_json((out + "_constraints.json").c_str(), o))) { fprintf(stderr, "error: %s\n", rs_last_error()); return 1; }
  if (fl.emit_substitution_log && (eng ? rs_engine_write_substitution_json(eng, (out + "_substitutions.json").c_str()) : rs_write_substitution_json((out + "_substitutions.json").c_str(), o))) {
    fprintf(stderr, "error: %s\n", rs_last_error());
    return 1;
  }
  if (in_wtns) {  // the witness: checked on the input, the output and the log, then projected onto the wires
    const uint32_t what = RS_WIT_INPUT | RS_WIT_OUTPUT | (fl.emit_substitution_log ? RS_WIT_LOG : 0u);
    rs_witness_report rep;
    rs_witness *w = nullptr;
    int rc = eng ? rs_engine_load_wtns(eng, in_wtns) : rs_read_wtns(in_wtns, &w);
    if (!rc) rc = eng ? rs_engine_check_witness(eng, in, what, &rep) : rs_check_witness(in, o, w, what, &rep);
    if (rc) { fprintf(stderr, "error: %s\n", rs_last_error()); rs_witness_free(w); return 1; }
    static const char *cls[RS_WITC_COUNT] = {"constant-equality input row", "equality input row", "linear input row",
                                             "non-linear input row", "output row", "substitution"};
    for (int c = 0; c < RS_WITC_COUNT; ++c)
      if (rep.failed[c]) {
        const bool input = c <= RS_WITC_NONLINEAR;
        fprintf(stderr, "witness: %s %llu does not hold (%llu of %llu fail): %s; no .wtns written\n", cls[c],
                (unsigned long long)rep.first_failed[c], (unsigned long long)rep.failed[c], (unsigned long long)rep.checked[c],
                input ? "the witness is not one of this circuit" : "the input rows hold, so this is a simplifier bug");
        rs_witness_free(w);
        return input ? 3 : 4;
      }
    rc = eng ? rs_engine_write_wtns(eng, (out + ".wtns").c_str()) : rs_write_wtns((out + ".wtns").c_str(), w, o);
    rs_witness_free(w);
    if (rc) { fprintf(stderr, "error: %s\n", rs_last_error()); return 1; }
    const unsigned long long n_in = rep.checked[RS_WITC_CONS_EQ] + rep.checked[RS_WITC_EQ] + rep.checked[RS_WITC_LINEAR] + rep.checked[RS_WITC_NONLINEAR];
    if (fl.emit_substitution_log)
      fprintf(stderr, "witness: %llu input rows, %llu output rows, %llu substitutions hold\n", n_in,
              (unsigned long long)rep.checked[RS_WITC_OUTPUT], (unsigned long long)rep.checked[RS_WITC_LOG]);
    else
      fprintf(stderr, "witness: %llu input rows, %llu output rows hold\n", n_in, (unsigned long long)rep.checked[RS_WITC_OUTPUT]);
  }
  // constraint_writers/src/log_writer.rs:24-47
  uint64_t nl = 0, l = 0;
  rs_rows ia, ib;
  rs_rows_begin(o, 0, &ia);
  rs_rows_begin(o, 1, &ib);
  for (uint64_t r = 0; r < o->n_constraints; ++r) {
    uint64_t ba, la, bb, lb;
    rs_rows_next(&ia, r, &ba, &la);
    rs_rows_next(&ib, r, &bb, &lb);
    ((la | lb) == 0 ? l : nl)++;
  }
  printf("non-linear constraints: %llu\n", (unsigned long long)nl);
  printf("linear constraints: %llu\n", (unsigned long long)l);
  printf("public inputs: %llu\n", (unsigned long long)in->n_pub_in);
  if (in->n_priv_in == o->no_private_inputs_witness)
    printf("private inputs: %llu\n", (unsigned long long)in->n_priv_in);
  else if (o->no_private_inputs_witness == 0)
    printf("private inputs: %llu (none belong to witness)\n", (unsigned long long)in->n_priv_in);
  else
    printf("private inputs: %llu (%llu belong to witness)\n", (unsigned long long)in->n_priv_in,
           (unsigned long long)o->no_private_inputs_witness);
  printf("public outputs: %llu\n", (unsigned long long)in->n_pub_out);
  printf("wires: %llu\n", (unsigned long long)o->n_wires);
  printf("labels: %llu\n", (unsigned long long)o->n_labels);
  fprintf(stderr, "simplification: %.3f ms\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
  rs_output_free(o_own);
  rs_input_free(in_own);
  rs_engine_destroy(eng);
  return 0;
}
