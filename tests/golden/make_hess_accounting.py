"""Regenerates tests/golden/hess_accounting.json: the integer and byte fields that covariance, pair_covariance, sensitivity,
robust_sensitivity, edge_reliability, polish, robust_polish, robust_covariance and gnc report -- refused (max_bytes = 1) and
unlimited -- on the cases of tests/test_gpu_hess_accounting.py, which lists the calls and reads the file.  All of these numbers
are computed on the host (the symbolic analysis, the predicted bytes, the column plans), but the calls need a device.  The
committed file was recorded with the build of the commit before the setup, the refusal and the verdict of these entry points
moved into dpgo_amd/csrc/hess.cpp: regenerate it only when a prediction is meant to change.  Needs an MI355X.

    python tests/golden/make_hess_accounting.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_gpu_hess_accounting as tha  # noqa: E402

if __name__ == "__main__":
    fixtures = os.path.join(os.path.dirname(os.path.dirname(HERE)), "fixtures", "g2o")
    out = {"%s/%d" % (name, nn): tha.record(fixtures, name, nn) for name, nn in tha.CASES}
    with open(os.path.join(HERE, "hess_accounting.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for case, calls in out.items():
        for label, modes in calls.items():
            print(case, label, modes["unlimited"])
