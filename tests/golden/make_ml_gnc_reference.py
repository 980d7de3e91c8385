"""Writes tests/golden/ml_gnc_reference.npz on the CPU: the restated runs of graduated non-convexity on the maximum-likelihood
objective (tests/ml_gnc_restatement.run) on the inputs of tests/ml_gnc_inputs.py, from the start and from the perturbed start.
tests/test_ml_gnc_host.py checks the file against the restatement on the smallest case; the GPU tests read it, so that none of
them waits for a restated run.

Every committed run must meet the conditions below; they are conditions on the inputs' seeds (ml_gnc_inputs.CASES).  Where one
fails, pick another seed -- never loosen a condition.

    python tests/golden/make_ml_gnc_reference.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ml_gnc_inputs as mgi  # noqa: E402
import ml_gnc_restatement as mgr  # noqa: E402
import newton_restatement as nr  # noqa: E402


def conditions(name, kind, run):
    E, _, R, outlier, _ = mgi.case(name)
    chi2 = mgr.chi2_theta(E, run["X"])[0]
    rejected = (R & (run["w"] == 0)) if kind == mgr.TLS else (R & (chi2 > mgi.C2[E["d"]]))
    return {"the outcome is CONVERGED": run["outcome"] == mgr.CONVERGED,
            "no inner STALLED": nr.STALLED not in run["inner"],
            "the last level's inner is CONVERGED": run["inner"][-1] == nr.CONVERGED,
            "exactly the injected outliers are rejected": bool(np.array_equal(rejected, outlier)) and int(outlier.sum()) >= 1,
            "the TLS margin is >= 1e-6": run["margin"] >= 1e-6,
            "theta <= pi - 0.1 wherever w > 0": run["theta_max"] <= np.pi - 0.1,
            "same_counts": run["same_counts"]}


if __name__ == "__main__":
    out = {}
    for name, kind in mgi.RUNS:
        run = mgi.compute(name, kind)
        for what, ok in conditions(name, kind, run).items():
            assert ok, (name, kind, what)
        out.update(mgi.pack(name, kind, run))
        print("%s %s: %d levels, inner %s, %d outliers, TLS margin %.3g, decision margin %.3g, theta_max %.3g, same_steps %s, "
              "worst relative spread %.3g" % (name, ("TLS", "GM")[kind], run["levels"], run["inner"], run["num_outliers"], run["margin"],
                                              run["decision_margin"], run["theta_max"], run["same_steps"],
                                              float((run["spread"] / np.abs(run["log"][:len(run["spread"]), 1:5])).max())), flush=True)
    np.savez_compressed(os.path.join(HERE, "ml_gnc_reference.npz"), **out)
