"""How k_fp_lg divides a problem's candidates over workgroups (csrc/kernel_plan.hpp fp_lg_chunks), held without a GPU.

One 8-lane group rolls out one (candidate, segment); a workgroup holds A_eff * M of them, 128 at the most (1024 threads).  Before this rule existed pddp_create refused
every handle with A_eff * M > 128 (M = 16 with A = 9 .. 15, M = 8 with A = 17 .. 23, M = 4 with A = 33, ...: "(candidates per workgroup) * M must not exceed 128"), so
nothing was ever launched for them.  tests/native/fp_lg_chunks_host_check.cpp (its own main, -fsanitize=address,undefined) sweeps every (M, A) the library accepts: never
more than 1024 threads, the chunks tile A exactly, and every (M, A) that create accepted before keeps its grid and workgroup size.  `create` (its LDS check) and
launch_fp_rollouts both call the function; tests/test_arm_edges.py runs M = 16, A = 12 on the GPU against the oracle."""
import ctypes
import os
import re
import subprocess

import pytest

import pyddp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_accepted_shape_has_a_launch_and_the_old_ones_keep_theirs(tmp_path):
    exe = str(tmp_path / "fp_lg_chunks_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "fp_lg_chunks_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "fp_lg_chunks_host_check: ok" in out.stdout, out.stdout + out.stderr
    assert int(re.search(r"\((\d+) of 1024", out.stdout).group(1)) > 0            # the sweep reached the shapes create refused before


@pytest.mark.parametrize("N,M,A", [(128, 16, 12), (32, 16, 13), (64, 8, 17), (64, 4, 33), (1024, 16, 60)])
def test_create_no_longer_refuses_more_than_128_lane_groups_per_problem(N, M, A):
    """pddp_create validates before it looks for a device (tests/test_boundary.py): these shapes pass the validation on either element type -- the handle exists, or the
    only complaint is the missing device."""
    lib = ctypes.CDLL(pyddp.library_path())
    lib.pddp_last_error.restype = ctypes.c_char_p
    for dtype in (0, 1):
        cfg = pyddp.default_config(4, N=N, M=M, A=A, dtype=dtype)
        h = ctypes.c_void_p()
        rc = lib.pddp_create(ctypes.byref(cfg), ctypes.byref(h))
        msg = lib.pddp_last_error().decode()
        if rc == 0:
            lib.pddp_destroy(h)
        else:
            assert rc == -2 and "must not exceed" not in msg and "LDS" not in msg, (rc, msg)      # PDDP_ENODEVICE
