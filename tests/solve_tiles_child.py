"""Child process of tests/test_gpu_solve_tiles.py (the library reads its DPGO_* settings once per process, so every plan of
the device solve is a process of its own):

    python solve_tiles_child.py OUT.npz [dynamic]

runs every input of solve_restatement.INPUTS through dpgo_amd.SpdSolverDebug for d = 3, 2 and dof = 1, d and stores, keys
"<input>|<d><dof>|<field>":
  the plan read-back (flags, fwd, bwd, root, root_fine, root_rows_level with their per-node counts, the front table)
  x, x2    scale = +1, twice          xneg   scale = -1          xip   in place (absent, refused = 1, where spd_run refuses)
  three_nodes: for every non-empty subset b of the nodes
    mv<b>  the subset in mask.v, the tile class of the roots chosen for all nodes (class_of)
    mw<b>  mask.v = all nodes, the subset in the device word
    mf<b>  the subset in mask.v and the class chosen for it;  fine<b>: what fine_root_for(b) answers
  dynamic (keep_numeric = True):  x is the first values' solve;  xkept after refactor() with the second values;  xfresh from a
    handle created with the second values, fresh_flags / fresh_levels its plan
Prints nothing."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dpgo_amd  # noqa: E402
import solve_restatement as sr  # noqa: E402

COMBOS = [(3, 1), (3, 3), (2, 1), (2, 2)]


def put_plan(out, prefix, plan):
    out[prefix + "flags"] = np.asarray([plan["fused_root"], plan["root_sym"], plan["root_rows"], plan["root_fine_rows"],
                                        plan["root_fine_below"], plan["stream_once"], plan["nnodes"]], np.int64)
    levels = plan["fwd"] + plan["bwd"] + [plan["root"], plan["root_fine"], plan["root_rows_level"]]
    out[prefix + "nlevels"] = np.asarray([len(plan["fwd"]), len(plan["bwd"])], np.int64)
    out[prefix + "levels"] = np.asarray([[v["rows"], v["nwide"], v["nnarrow"]] for v in levels], np.int64)
    out[prefix + "counts"] = np.asarray([np.stack([v["wcount"], v["ncount"]], axis=1) for v in levels], np.int64)
    for k in ("w", "u", "parent", "height"):
        out[prefix + k] = plan[k]
    out[prefix + "piv_idx"] = np.concatenate([np.zeros(0, np.int32)] + plan["piv_idx"])
    out[prefix + "upd_idx"] = np.concatenate([np.zeros(0, np.int32)] + plan["upd_idx"])


def main(argv):
    dynamic = len(argv) > 2 and argv[2] == "dynamic"
    out = {}
    for name in sr.INPUTS:
        inp = sr.build_input(name)
        for d, dof in COMBOS:
            prefix = "%s|%d%d|" % (name, d, dof)
            _, vin, vout = sr.rhs(name, d, dof)
            S = dpgo_amd.SpdSolverDebug(inp.csr, *inp.args, d=d, dof=dof, node_of_unknown=inp.nodes, keep_numeric=dynamic)
            put_plan(out, prefix, S.plan())
            out[prefix + "x"] = S.run(vin, vout)
            out[prefix + "x2"] = S.run(vin, vout)
            out[prefix + "xneg"] = S.run(vin, vout, scale=-1.0)
            xip = S.run(vin, vout, in_place=True)
            if xip is None:
                out[prefix + "refused"] = np.ones(1)
            else:
                out[prefix + "xip"] = xip
            if inp.nnodes > 1:
                every = (1 << inp.nnodes) - 1
                for b in range(1, every + 1):
                    out[prefix + "mv%d" % b] = S.run(vin, vout, mask=b, class_of=every)
                    out[prefix + "mw%d" % b] = S.run(vin, vout, mask=every, mask_word=b)
                    out[prefix + "mf%d" % b] = S.run(vin, vout, mask=b)
                    out[prefix + "fine%d" % b] = np.asarray([S.fine_root_for(b)])
            if dynamic:
                inp2 = sr.build_input(name, second=True)
                assert np.array_equal(inp2.csr.indices, inp.csr.indices) and np.array_equal(inp2.csr.indptr, inp.csr.indptr)
                _, vin2, vout2 = sr.rhs(name, d, dof, second=True)
                S.refactor(inp2.csr.data)
                out[prefix + "xkept"] = S.run(vin2, vout2)
                S2 = dpgo_amd.SpdSolverDebug(inp2.csr, *inp.args, d=d, dof=dof, node_of_unknown=inp.nodes, keep_numeric=True)
                out[prefix + "xfresh"] = S2.run(vin2, vout2)
                fresh = {}
                put_plan(fresh, "", S2.plan())
                out[prefix + "fresh_flags"], out[prefix + "fresh_levels"] = fresh["flags"], fresh["levels"]
                S2.close()
            S.close()
    np.savez(argv[1], **out)


if __name__ == "__main__":
    main(sys.argv)
