"""One keys-first case through rs_engine_simplify in a process of its own (tests/test_gpu_input_contract.py
starts it with RS_PROF set, which the library reads once when it is loaded, and reads the branch taken
from this process's stderr: `[rs-prof] linear rows: keys first | keys + values` and `[rs-prof]
keys-first: N rows settled from host values`).  Prints one JSON line: the comparison with the oracle on
the canonical form, the uncertain-row certificate and unc_cap for the case's linear block.

    python tests/keysfirst_child.py CASE      CASE: cap-1 | cap | cap+1 | cap_reversed | plain | late_bad_value
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, d)

import input_contract as ic  # noqa: E402
import rsio  # noqa: E402
import circom_cvm_amd as M  # noqa: E402

R = rsio.R
CASES = ("cap-1", "cap", "cap+1", "cap_reversed", "plain", "late_bad_value")


def build(case: str):
    """-> (the canonical holder, the holder to run, the uncertain-row certificate, the number of linear rows)."""
    p = R.PRIMES["bn128"]
    if case == "plain":
        sys_ = ic.plain_system(p)
    else:
        # sized by unc_cap's floor: the gadget's linear block must stay too small to raise the cap
        total = ic.unc_cap(0) + {"cap-1": -1, "cap": 0, "cap+1": 1, "cap_reversed": 0, "late_bad_value": -1}[case]
        sys_ = ic.uncertain_gadget(total // 2, total - total // 2, p)
        n_lin = len(R.classify(sys_)[2])
        assert ic.unc_cap(n_lin) == ic.unc_cap(0), (n_lin, ic.unc_cap(n_lin))
    h = rsio.InputHolder(sys_, "bn128")
    g = h
    if case == "cap_reversed":      # one linear row arrives descending: the unsorted flag
        g = ic.copy_holder(h)
        b = g.blocks[ic.LIN]
        s, e = ic.rows_of(b, int(b.lc.n_rows) // 2)
        b.col[s:e] = b.col[s:e][::-1].copy()
        v = b.val.reshape(-1, 4)
        v[s:e] = v[s:e][::-1].copy()
    elif case == "late_bad_value":  # sorted linear keys, a zero value in the last linear row
        g = ic.defect(h, "zero_value", ic.LIN)
    return h, g, ic.uncertain_rows(sys_), len(R.classify(sys_)[2])


def main(case: str) -> int:
    h, g, cert, n_lin = build(case)
    fl = rsio.flags("O2")
    ref, _ = rsio.oracle_arrays(h.inp, fl)
    out = {"case": case, "uncertain": cert, "unc_cap": ic.unc_cap(n_lin), "not_ascending": ic.not_ascending(g.blocks[ic.LIN]),
           "code": 0}
    eng = M.Engine(0)
    try:
        try:
            out["diff"] = rsio.diff_output_arrays(rsio.output_arrays(eng.simplify(g.inp, fl)), ref)
        except M.RsError as ex:
            out["code"] = ex.code
            sys.stderr.write("[child] rejected\n")
            # the engine recovers: the valid input right after
            out["diff"] = rsio.diff_output_arrays(rsio.output_arrays(eng.simplify(h.inp, fl)), ref)
    finally:
        eng.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
