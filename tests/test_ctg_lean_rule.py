"""The rule by which the matrix-core backward pass leaves a problem's interior cost-to-go unwritten (may_exit_within_two, csrc/solver_state.hpp), without a GPU.

tests/native/ctg_lean_rule_host_check.cpp (its own main, -fsanitize=address,undefined) runs every state of a grid through line_search_accept for all four outcomes of two
sweeps: a problem that can exit within two sweeps is never lean, and a fresh problem far from its limits is.  The GPU side -- one iterate(n) against n calls of
iterate(1), bit for bit -- is tests/test_ctg_last_pass.py; whether a lean pass wrote fewer bytes is a counter's matter (profiles/ctg_last_pass.md), not an output's:
the rule exists so that no output can tell."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-ddp_amd", "csrc")


def test_no_state_that_can_exit_within_two_sweeps_is_lean(tmp_path):
    name = "ctg_lean_rule_host_check"
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and name + " ok" in out.stdout, out.stdout + out.stderr
    assert out.stdout.count("states lean") == 4


def test_the_pass_and_its_launcher_use_the_checked_rule():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("bp_mfma.hpp", "pddp_mx.hip", "solver_state.hpp")}
    assert "may_exit_within_two(b.state[pb], flags)" in src["bp_mfma.hpp"] and "lean_flags_max_iter(" in src["pddp_mx.hip"]
    for f in ("bp_mfma.hpp", "pddp_mx.hip"):
        assert "kMxLeanIfRunning =" not in src[f] and "bool may_exit_within_two" not in src[f], f      # defined once, in the header the host check compiles
