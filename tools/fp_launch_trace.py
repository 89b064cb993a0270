#!/usr/bin/env python3
"""Every way a caller can ask for the forward pass, on the eight handles of tests/native/kernel_plan_host_check.cpp check_fp_modes, in ONE process -- to be run under a
kernel trace once per library build, so that two builds can be compared launch for launch:

    rocprofv3 --kernel-trace --output-format csv -d DIR_A -- python tools/fp_launch_trace.py PATH_A/libpddp.so
    rocprofv3 --kernel-trace --output-format csv -d DIR_B -- python tools/fp_launch_trace.py            (this tree's build)
    python tools/fp_launch_trace.py --compare DIR_A DIR_B

Per handle (use_graph = 0, so every launch goes through the launch functions): a load with the forward rollout (the initial rollout), pddp_iterate(1) (production),
pddp_time_kernels(1) (sweep only / rollouts only), pddp_time_sweeps(1, phases) (the traced iteration), pddp_run_phase FP / ROLLOUT (the hook, the hook's rollouts) and
BP_FUSED / SWEEP_FUSED (the hook's fused sweep; refused by handles without one, which launches nothing).  The cart-pole handle once more with a table of diagonal records.
--compare reads the two traces in dispatch order and requires the same sequence of (kernel name with template arguments, grid, workgroup, LDS bytes); it prints the two
lengths and the verdict, and the first differing launches if there are any (exit status 1)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "parallel-ddp_amd"))

# plant, dtype, batch, A, integrator, use_limits, diagonal-record table: N = 64, M = 4
HANDLES = [(4, 0, 1, 8, 1, 0, 0), (4, 0, 512, 8, 1, 0, 0), (4, 1, 2, 8, 1, 0, 0), (4, 0, 1, 8, 1, 1, 0), (2, 0, 4096, 8, 3, 0, 0), (2, 0, 4096, 4, 3, 0, 0), (2, 0, 2, 8, 3, 0, 0),
           (3, 0, 2048, 16, 3, 0, 0), (2, 0, 4096, 8, 3, 0, 1)]


def drive(lib):
    import numpy as np
    import pyddp
    N = 64
    for plant, dtype, B, A, integ, limits, table in HANDLES:
        c = pyddp.default_config(plant, _lib_path=lib, dtype=dtype, N=N, M=4, A=A, integrator=integ, batch=B, use_limits=limits, max_iter=2, use_graph=0, tol_cost=0.0,
                                 **(dict(wafr_urdf=1) if plant == 4 else {}))
        s = pyddp.Solver(c, _lib_path=lib)
        try:
            if table:
                s.set_diag_cost(s.get_diag_cost_problems([0]))
            x0 = np.zeros((B, N, s.n), s.dtype)
            x0[:, :, 0] = 0.1
            s.load(x0, np.full((B, N, s.m), 0.01, s.dtype), np.full((B, s.n), 0.2, s.dtype), forward_rollout=1)
            s.iterate(1)
            s.sync()
            names = [n for n, _ in s.time_kernels(1)]
            s.time_sweeps(1, phases=True)
            refused = []
            for phase in (pyddp.PHASE_FP, pyddp.PHASE_ROLLOUT, pyddp.PHASE_BP_FUSED, pyddp.PHASE_SWEEP_FUSED):
                try:
                    s.run_phase(phase)
                except pyddp.PddpError:
                    refused.append(phase)
            s.sync()
            print(f"plant {plant} dtype {dtype} batch {B} A {A} use_limits {limits} table {table}: {' '.join(names)}; phases refused: {refused}", flush=True)
        finally:
            s.close()


def launches(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        sys.exit(f"{directory}: {len(files)} kernel trace files, expected one")
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    lds = next(k for k in rows[0] if k.startswith("LDS_Block_Size"))
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{d}"]) for d in "XYZ"), tuple(int(r[f"Workgroup_Size_{d}"]) for d in "XYZ"), int(r[lds])) for r in rows]


def compare(dir_a, dir_b):
    a, b = launches(dir_a), launches(dir_b)
    print(f"{dir_a}: {len(a)} launches, {len(set(n for n, *_ in a))} distinct kernels")
    print(f"{dir_b}: {len(b)} launches, {len(set(n for n, *_ in b))} distinct kernels")
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
    if first is None:
        print("the two sequences of (kernel, grid, workgroup, LDS) are identical")
        return 0
    print(f"the sequences differ from launch {first}:")
    for i in range(max(0, first - 2), first + 3):
        print(f"  {i}: {a[i] if i < len(a) else None}\n  {' ' * len(str(i))}  {b[i] if i < len(b) else None}")
    return 1


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    drive(sys.argv[1] if len(sys.argv) > 1 else None)
