"""Child process of tests/test_factor_fronts_host.py and tests/test_gpu_factor_fronts.py (the library reads its DPGO_*
settings once per process, so every elimination path is a process of its own):

    python factor_fronts_child.py OUT.npz [FAILS.npz]

factors every input of factor_restatement.INPUTS through dpgo_amd.spd_factor_debug and stores what the hook returned, keys
"<input>|<run>|<field>":
  first   the input's values, with the second values factored afterwards through the kept context (-> kept)
  again   the input's values once more (the same bits twice)
  fresh   the second values by a call of their own (what `kept` must equal)
  only    factor_only = True on the first and, through the kept context, on the second values (arrow_wide alone)
FAILS.npz (optional) holds indefinite value arrays "<case>|<input>" in the CSR order of the input; for each of them
  <case>|fail      the verdict, with the input's SPD values factored afterwards through the kept context
  <case>|failonly  the same under factor_only
  <case>|after     the SPD input factored next, by a call of its own
Prints nothing."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dpgo_amd  # noqa: E402
import factor_restatement as fr  # noqa: E402

STRUCT = ("w", "u", "parent", "height", "ldw", "ldm", "w_off", "wt_off")


def put(out, prefix, res, structure=False):
    for k in ("status", "fail_front", "pivot_min", "pivot_max", "on_device", "nfronts"):
        out["%s|%s" % (prefix, k)] = np.asarray(res[k])
    for k in ("W", "WT"):
        if res.get(k) is not None:
            out["%s|%s" % (prefix, k)] = res[k]
    if structure:
        for k in STRUCT:
            out["%s|%s" % (prefix, k)] = res[k]
        out["%s|piv_idx" % prefix] = np.concatenate([np.zeros(0, np.int32)] + res["piv_idx"])
        out["%s|upd_idx" % prefix] = np.concatenate([np.zeros(0, np.int32)] + res["upd_idx"])


def second(res):
    """The second factorisation of a call, in the shape of a first one."""
    return dict(res, status=res["status2"], fail_front=res["fail_front2"], pivot_min=res["pivot_min2"],
                pivot_max=res["pivot_max2"], W=res["W2"], WT=res["WT2"])


def main(argv):
    out = {}
    args = {name: (spec["leaf"], spec["collapse"], spec["block"]) for name, spec in fr.INPUTS.items()}
    for name in fr.INPUTS:
        csr, csr2 = fr.build_input(name)[1], fr.build_input(name, second=True)[1]
        r = dpgo_amd.spd_factor_debug(csr, *args[name], refactor_values=csr2.data)
        put(out, name + "|first", r, structure=True)
        put(out, name + "|kept", second(r))
        put(out, name + "|again", dpgo_amd.spd_factor_debug(csr, *args[name]))
        put(out, name + "|fresh", dpgo_amd.spd_factor_debug(csr2, *args[name]))
    name = "arrow_wide"
    csr, csr2 = fr.build_input(name)[1], fr.build_input(name, second=True)[1]
    r = dpgo_amd.spd_factor_debug(csr, *args[name], factor_only=True, refactor_values=csr2.data)
    assert r["W"] is None and r["W2"] is None
    put(out, name + "|only", r)
    put(out, name + "|onlykept", second(r))
    if len(argv) > 2:
        fails = np.load(argv[2])
        for key in fails.files:
            case, name = key.split("|")
            csr = fr.build_input(name)[1]
            bad = csr.copy()
            bad.data = fails[key].copy()
            r = dpgo_amd.spd_factor_debug(bad, *args[name], refactor_values=csr.data)
            put(out, case + "|fail", r)
            put(out, case + "|failkept", second(r))
            put(out, case + "|failonly", dpgo_amd.spd_factor_debug(bad, *args[name], factor_only=True))
            put(out, case + "|after", dpgo_amd.spd_factor_debug(csr, *args[name]))
    np.savez(argv[1], **out)


if __name__ == "__main__":
    main(sys.argv)
