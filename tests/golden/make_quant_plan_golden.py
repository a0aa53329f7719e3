"""Generates tests/golden/quant_plan_parent.json: the five quantized planners -- wg_debug_{gemv_q8,gemv_q4,gemm_q8,gemm_q4,gemm_q8a8}_plan -- as DATA, recorded from
the commit BEFORE they were given one shared core (quant_plan_common.hpp).

    python tests/golden/make_quant_plan_golden.py --lib <that commit's libwgebra_hip.so> --commit <hash> [--out PATH]

The planners are pure host arithmetic, reachable without a device: everything is recorded and checked on the CPU. Per family the file holds
  rows     the explicit queries of tests/_quant_plan.py (the cut cases of the GPU tests on 256, 16 and 8 CUs; both sides of every threshold), each as
           [query fields ..., plan fields ..., status, message, tags] in the order of `query_fields` + `plan_fields`;
  digests  one SHA-256 per generated block of 1000 queries (tests/_quant_plan.py: block), over the concatenated (plan bytes without padding, status, message, tags).
Never run this on the code under test: tests/test_quant_plan_parent.py holds the current library to what THAT commit answered.
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libwgebra_hip.so built from the parent commit")
    ap.add_argument("--commit", required=True, help="the commit that library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "quant_plan_parent.json"))
    args = ap.parse_args()
    import _quant_plan as Q
    fns = Q.bind(ctypes.CDLL(os.path.abspath(args.lib)))
    doc = {"parent_commit": args.commit, "blocks": Q.BLOCKS, "block_size": Q.BLOCK_SIZE, "families": {}}
    for fam in Q.FAMILIES:
        run = Q.Runner(fns, fam)
        rows = [list(v) + run.row(v) for v in Q.explicit(fam)]
        doc["families"][fam] = {"query_fields": Q.query_fields(fam), "plan_fields": Q.plan_fields(fam) + ["status", "message", "tags"], "rows": rows,
                                "digests": [run.digest(Q.block(fam, b)) for b in range(Q.BLOCKS)]}
        nsplit = Q.plan_fields(fam).index("nsplit") + len(Q.query_fields(fam))
        print(f"{fam}: {len(rows)} rows ({sum(r[nsplit] > 1 for r in rows)} cut, {sum(r[-3] != 0 for r in rows)} refused), {Q.BLOCKS} digests", flush=True)
    text = json.dumps(doc, separators=(",", ":"))
    text = "],\n[".join("],[".join(c) for c in (lambda r: [r[i:i + 4] for i in range(0, len(r), 4)])(text.split("],[")))  # four rows to a line
    text = '",\n"'.join('","'.join(c) for c in (lambda r: [r[i:i + 4] for i in range(0, len(r), 4)])(text.split('","')))  # ... and four digests
    assert len(text) <= 256 << 10, f"{len(text)} bytes"
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(f"{args.out}: {len(text)} bytes")


if __name__ == "__main__":
    main()
