#!/usr/bin/env python3
"""The load stage of a control cycle in every form mpc_launch_load selects (solver_impl.hpp), in ONE process -- to be run under a kernel trace once per library build,
so that two builds can be compared launch for launch:

    rocprofv3 --kernel-trace --output-format csv -d DIR_A -- python tools/mpc_load_trace.py PATH_A/libpddp.so
    rocprofv3 --kernel-trace --output-format csv -d DIR_B -- python tools/mpc_load_trace.py            (this tree's build)
    python tools/mpc_load_trace.py --compare DIR_A DIR_B

Five handles of four problems: the float32 arm with the Euler integrator and each built-in robot model (the 512-thread pipeline, V = 0 and V = 1), the float32 arm on the
lane-group rollouts and the float64 arm (the 256-thread kernel), the float64 pendulum with Runge-Kutta 3.  On each, after a load: pddp_mpc_load once (k_mpc_load) and
pddp_mpc_load_problems with two named slots once (the movers around k_mpc_load_slots on the intake area).  --compare is tools/fp_launch_trace.py's: the same sequence of
(kernel name with template arguments, grid, workgroup, LDS bytes) in dispatch order, or the first differing launches and exit status 1."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ARM = dict(N=16, M=2, A=4, integrator=1)
# label, plant, dtype, configuration
HANDLES = [("arm float32 Euler, default URDF", 4, 0, dict(ARM, wafr_urdf=0)), ("arm float32 Euler, wafr_urdf = 1", 4, 0, dict(ARM, wafr_urdf=1)),
           ("arm float32, kernels.fp = lg", 4, 0, dict(ARM, wafr_urdf=1, kernels=dict(fp="lg"))), ("arm float64", 4, 1, dict(ARM, wafr_urdf=1)),
           ("pendulum float64 Runge-Kutta 3", 1, 1, dict(N=16, M=2, A=4, integrator=3))]
B, IDX, SHIFT = 4, [3, 1], [2, 0]


def drive(lib):
    import numpy as np
    import pyddp
    for label, plant, dtype, kw in HANDLES:
        s = pyddp.Solver(pyddp.default_config(plant, _lib_path=lib, dtype=dtype, batch=B, max_iter=2, use_graph=0, tol_cost=0.0, **kw), _lib_path=lib)
        try:
            N = s.cfg.N
            x0 = np.zeros((B, N, s.n), s.dtype)
            x0[:, :, 0] = 0.1
            goal = np.full((B, s.n), 0.2, s.dtype)
            s.load(x0, np.full((B, N, s.m), 0.01, s.dtype), goal)
            s.mpc_load(x0[:, 1], goal, np.ones(B, np.int32), clear_vars=0, full_rollout=1)
            s.mpc_load_problems(IDX, x0[IDX, 0], goal[IDX], SHIFT, clear_vars=0, full_rollout=1)
            s.sync()
            print(f"{label}: pddp_mpc_load and pddp_mpc_load_problems({IDX}) ran", flush=True)
        finally:
            s.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        from fp_launch_trace import compare
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    drive(sys.argv[1] if len(sys.argv) > 1 else None)
