"""The library's DPGO_* environment settings are read in one place (dpgo_amd/csrc/settings.cpp), listed with their defaults
in settings.h, named in DESIGN 8, and follow one parse rule: a flag is on when set and not 0."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpgo_amd", "csrc")


def test_only_settings_cpp_reads_the_environment():
    # (exempt: the dist_pgo driver executable, and rdv.h, which tests/test_rendezvous.py compiles on its own)
    readers = set()
    for f in glob.glob(os.path.join(CSRC, "*")):
        if f.endswith((".cpp", ".h", ".hip")) and re.search(r"\bgetenv\b", open(f).read()):
            readers.add(os.path.basename(f))
    assert readers - {"dist_pgo.cpp", "rdv.h"} == {"settings.cpp"}, readers


def test_every_setting_is_in_the_table_and_in_design():
    names = set(re.findall(r'"(DPGO_[A-Z0-9_]+)"', open(os.path.join(CSRC, "settings.cpp")).read()))
    assert len(names) > 40, sorted(names)
    header = open(os.path.join(CSRC, "settings.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in sorted(names):
        assert re.search(r"\b%s\b" % name, header), name
        assert re.search(r"\b%s\b" % name, design), name


@pytest.mark.parametrize("value,on", [("1", True), ("0", False), (None, False)])
def test_setup_timing_flag(fixtures_dir, value, on):
    code = ("import sys; sys.path.insert(0, %r); import dpgo_amd; dpgo_amd.read_g2o(sys.argv[1], 1).chordal_initialization()"
            % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "DPGO_SETUP_TIMING"}
    if value is not None:
        env["DPGO_SETUP_TIMING"] = value
    r = subprocess.run([sys.executable, "-c", code, os.path.join(fixtures_dir, "smallGrid3D.g2o")], env=env,
                       capture_output=True, text=True, check=True)
    assert ("[setup] chordal initialisation" in r.stderr) == on, r.stderr
    if not on:
        assert "[setup]" not in r.stderr, r.stderr
