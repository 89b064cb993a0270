"""What a control cycle sends and gets back, as bytes: csrc/mpc_record.hpp is the one definition of the input run (measured states | goals | shifts) and of the packed
result record (state | x | u | K | Jout | alphaOut) that k_mpc_store fills and mpc_cycle reads.

Without a GPU: tests/native/mpc_record_host_check.cpp (its own main, -fsanitize=address,undefined) holds the offsets against values written out by hand, the structure
of every record, the input run against the expression "mpc_in" was allocated with before, and a pack / unpack round trip through the functions the kernel and the host
call, on buffers with no slack; and the sources no longer spell either layout anywhere else.  On the GPU: the packed single-transfer path against the polled path
with its direct copies, bit for bit, every output of every problem."""
import os
import re
import subprocess

import numpy as np
import pytest

from backends import make_solver
from oracle_binding import example_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-ddp_amd", "csrc")


def _run_host_check(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and name + ": ok" in out.stdout, out.stdout + out.stderr


def test_record_and_input_run_layouts_and_the_round_trip(tmp_path):
    _run_host_check(tmp_path, "mpc_record_host_check")


def test_the_layouts_are_defined_once():
    for f in ("solver_impl.hpp", "kernels.hpp"):
        src = open(os.path.join(CSRC, f)).read()
        for gone in ("rec_state", "o_xb", "o_KT", "(sizeof(SolverState<T>) + 15) / 16 * 16"):
            assert gone not in src, (f, gone)
    rec = open(os.path.join(CSRC, "mpc_record.hpp")).read()
    assert "getenv" not in rec and not re.search(r"\bhip[A-Z]\w*\s*\(", rec)
    local = [h for h in re.findall(r'#include\s+"([^"]+)"', rec)]
    assert local == ["solver_state.hpp"] and not [h for h in re.findall(r"#include\s+<([^>]+)>", rec) if h.startswith("hip")]


@pytest.mark.gpu
@pytest.mark.parametrize("plant,dtype,kw", [
    (1, np.float64, dict(N=8, M=2, A=4, batch=3, max_iter=3, tol_cost=0.0)),                                                # out_stride 5 (odd) under doubles
    (4, np.float32, dict(N=16, M=2, A=4, batch=3, max_iter=4, wafr_urdf=1, mpc_mode=1, total_time=0.5, tol_cost=0.0)),
], ids=["pendulum-f64", "arm-f32"])
def test_packed_and_polled_cycles_return_the_same_bits(plant, dtype, kw):
    """Two handles loaded alike run the same two cycles (clear_vars = 1, then a warm start shifted by one knot), max_iter = 3: poll_every = 8 takes the single packed
    transfer (k_mpc_store's record, unpacked on the host), poll_every = 1 the polled path whose copy-only store and direct transfers do not know the record.  Three
    problems with their own measured states and goals, so that a wrong offset inside a record or a wrong stride between records lands on other numbers."""
    rng = np.random.default_rng([71, plant])
    B, N = kw["batch"], kw["N"]
    x0, u0, xg = example_inputs(plant, N, dtype)
    n = xg.size
    x0 = np.tile(x0, B) + rng.normal(0, 0.001, B * N * n).astype(dtype)
    u0 = np.tile(u0 if plant != 4 else np.full_like(u0, 0.01), B)
    goals = (np.tile(xg, (B, 1)) + 0.05 * np.arange(B)[:, None]).astype(dtype)
    xact = x0.reshape(B, N, n)[:, 0] + rng.normal(0, 0.002, (B, n)).astype(dtype)
    bump = rng.normal(0, 0.0005, (B, n)).astype(dtype)
    res = []
    for poll in (8, 1):
        s = make_solver("hip", plant, dtype=int(dtype == np.float64), **kw)
        s.load(x0, u0, goals)
        first = s.mpc_solve(xact, goals, 0, clear_vars=1, max_iter=3, poll_every=poll)
        second = s.mpc_solve(first["x"][:, 1] + bump, goals, 1, clear_vars=0, max_iter=3, poll_every=poll)
        res.append((first, second))
        s.close()
    for cycle, (packed, polled) in enumerate(zip(*res)):
        assert (packed["iters"] >= 1).all() and np.isfinite(packed["x"]).all() and np.isfinite(packed["KT"]).all()
        assert len({packed["x"][b].tobytes() for b in range(B)}) == B                      # the problems differ: a stride of zero would not pass
        for name in ("x", "u", "KT", "Jout", "alphaOut", "success", "iters"):
            assert packed[name].tobytes() == polled[name].tobytes(), (cycle, name)
