"""The dist_pgo driver (dpgo_amd/csrc/dist_pgo.cpp) as a whole: the order of its steps after the loop when every flag is given at
once, the exact lines that say why a step is not computed, the errors for flags that go together, and -- without a GPU -- the
help text and the argument checks in front of the loader.  What each step's line and report HOLD is compared bit for bit with the
Python API by the per-flag tests (test_dist_pgo_*_flags and their kin); nothing here repeats that."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "dpgo_amd", "dist_pgo")
LAUNCHER = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TORCHELASTIC_RUN_ID", "MASTER_PORT", "DPGO_FORCE_COMM")


def drive(args, cwd):
    env = {k: v for k, v in os.environ.items() if k not in LAUNCHER}
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, cwd=cwd, env=env, timeout=300)


def common(fixtures_dir):
    return ["--dataset", os.path.join(fixtures_dir, "tinyGrid3D.g2o"), "--num_nodes", "2", "--iters", "30", "--dist_init", "false",
            "--save", "false"]


# every report the trivial-loss steps write, in step order; both spellings of a switch and of a value flag are in all_steps()
REPORTS = ["modes.txt", "edges.txt", "cov.txt", "gate.txt", "sens.txt", "rely.txt", "marg.txt", "sel.txt"]


def all_steps(tmp_path):
    import test_gpu_candidate_set as tcs  # (its candidates; none of its tests is imported)
    import test_gpu_joint_marginal as tjm  # (its kept set)
    cand = tcs.write_candidates(tmp_path)
    (tmp_path / "set.txt").write_text("".join("%d\n" % p for p in tjm.KEPT))
    return ["--polish", "--hessian_modes", "2", "--modes_report=modes.txt", "--staircase=true", "--certify", "--verify=true",
            "--edge_report", "edges.txt", "--verify_reweighted", "--covariance=cov.txt", "--gate_candidates", cand, "--gate_report=gate.txt",
            "--sensitivity_pose=3", "--sensitivity_report", "sens.txt", "--edge_reliability", "rely.txt", "--marginal_set=set.txt",
            "--marginal_report", "marg.txt", "--select_candidates=%s" % cand, "--select_report", "sel.txt"]


def after_summary(stdout):
    lines = stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("time: ")]
    assert len(at) == 1, stdout[-2000:]
    return lines[at[0] + 1:]


@pytest.mark.gpu
def test_order_of_the_steps(fixtures_dir, tmp_path):
    """Every trivial-loss flag at once: one line per step behind the summary, in the order main() runs them, and every report."""
    assert os.path.exists(EXE), "build with __graft_entry__.build()"
    run = drive(common(fixtures_dir) + all_steps(tmp_path), tmp_path)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = after_summary(run.stdout)
    want = ["polish:", "modes:", "staircase:", "certificate:", "verification:", "reweighted verification:", "covariance:", "gate:",
            "sensitivity:", "reliability:", "marginal:", "candidates:"]
    assert len(lines) == len(want), lines
    for line, prefix in zip(lines, want):
        assert line.startswith(prefix + " ") and "not computed" not in line, line
    for name in REPORTS:
        assert (tmp_path / name).exists() and (tmp_path / name).stat().st_size > 0, name


@pytest.mark.gpu
def test_refusals_word_for_word(fixtures_dir, tmp_path):
    """The lines that say why a step is not computed: a robust loss for the trivial-loss steps, the trivial loss for the robust
    ones, no --polish for the two steps that are taken at a critical point."""
    assert os.path.exists(EXE), "build with __graft_entry__.build()"
    run = drive(common(fixtures_dir) + all_steps(tmp_path) + ["--loss", "huber", "--iters", "5"], tmp_path)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = after_summary(run.stdout)
    subject = [("polish", "Hessian"), ("modes", "Hessian"), ("staircase", "relaxation"), ("certificate", "certificate"),
               ("verification", "certificate"), None, ("covariance", "Hessian"), ("gate", "Hessian"), ("sensitivity", "Hessian"),
               ("reliability", "Hessian"), ("marginal", "Hessian"), ("candidates", "Hessian")]
    assert len(lines) == len(subject), lines
    for line, s in zip(lines, subject):
        if s is None:
            assert line.startswith("reweighted verification: ") and "not computed" not in line, line
        else:
            assert line == "%s: not computed (the %s is that of the trivial loss; --loss huber)" % s, line
    assert (tmp_path / "edges.txt").stat().st_size > 0
    for name in REPORTS:
        assert name == "edges.txt" or not (tmp_path / name).exists(), name

    run = drive(common(fixtures_dir) + ["--robust_polish", "--robust_covariance", "f.txt"], tmp_path)
    assert run.returncode == 0, run.stderr[-2000:]
    assert after_summary(run.stdout) == ["robust polish: not computed (the loss is trivial: --polish is the call)",
                                         "robust covariance: not computed (the loss is trivial: --covariance is the call)"]
    assert not (tmp_path / "f.txt").exists()

    run = drive(common(fixtures_dir) + ["--sensitivity_pose", "3", "--sensitivity_report", "f.txt", "--edge_reliability", "g.txt"], tmp_path)
    assert run.returncode == 0, run.stderr[-2000:]
    assert after_summary(run.stdout) == ["sensitivity: not computed (it is taken at a critical point: --polish)",
                                         "reliability: not computed (it is taken at a critical point: --polish)"]
    assert not (tmp_path / "f.txt").exists() and not (tmp_path / "g.txt").exists()


@pytest.mark.gpu
def test_flags_that_go_together(fixtures_dir, tmp_path):
    """One flag of a pair alone, and a --gnc that is no kind: an error on stderr and a non-zero exit status, behind the loop."""
    assert os.path.exists(EXE), "build with __graft_entry__.build()"
    cases = [(["--hessian_modes", "2"], "--hessian_modes and --modes_report go together."),
             (["--gate_candidates", "f.g2o"], "--gate_candidates and --gate_report go together."),
             (["--sensitivity_pose", "3"], "--sensitivity_pose (a pose of the graph) and --sensitivity_report go together."),
             (["--marginal_set", "f.txt"], "--marginal_set and --marginal_report go together."),
             (["--select_candidates", "f.g2o"], "--select_candidates and --select_report go together."),
             (["--gnc", "foo"], "--gnc takes tls or gm.")]
    for extra, message in cases:
        run = drive(common(fixtures_dir) + ["--iters", "1"] + extra, tmp_path)
        assert run.returncode != 0, extra
        assert message in run.stderr.splitlines(), (extra, run.stderr[-2000:])
        assert after_summary(run.stdout) == [], extra


def test_help_and_the_checks_in_front_of_the_loader(golden_dir, tmp_path):
    """No GPU: --help is the recorded text, and each argument check ends the run with its message before the dataset is read (the
    dataset named does not exist, and the loader would say so)."""
    if not os.path.exists(EXE):
        pytest.skip("dpgo_amd/dist_pgo has not been built (__graft_entry__.build())")
    run = drive(["--help"], tmp_path)
    assert run.returncode == 0 and run.stderr == ""
    assert run.stdout == open(os.path.join(golden_dir, "dist_pgo_help.txt")).read()
    cases = [(["--dataset", "none.g2o", "--num_nodes", "2", "--loss", "foo"], ' The loss type can only be "trivial", "huber" or "welsch".\n'),
             (["--num_nodes", "2"], "No dataset has been specfied.\n"),
             (["--dataset", "none.g2o"], "No number of nodes has been specfied.\n"),
             (["--dataset", "none.g2o", "--num_nodes", "2", "--world", "2", "--rank", "2"], "Inconsistent --rank / --world.\n")]
    for args, message in cases:
        run = drive(args, tmp_path)
        assert run.returncode != 0, args
        assert (run.stdout, run.stderr) == ("", message), (args, run.stdout, run.stderr)
