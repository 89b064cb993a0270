#!/usr/bin/env python3
"""Record the kernel selection of a grid of configurations: tests/golden/kernel_selection_table.json.

For every row: create a handle, load, run two sweeps, and write down the six names pddp_time_kernels reports and which of the optional arrays
(xw with its record length, segmap, ABc, Hc) the handle knows.  tests/test_kernel_plan.py feeds the same rows through csrc/kernel_plan.hpp on the
host and requires the same answers, so the table is recorded ONCE, from the library whose selection is to be preserved, and regenerated only when
a selection changes on purpose:

    python tools/kernel_plan_table.py tests/golden/kernel_selection_table.json [path of another libpddp build]        (needs a GPU; well under a minute)

The grid straddles every crossover of the selection (batch 1 .. 4096 around 256 / 1024 / 4096 / 8192 (problem, segment) units, 511 / 512 / 513 and
2048 problems; 96 knots per segment; 256 knots per horizon) and every value of every pddp_config.kernels field on the plants it pertains to.
use_finite_diff is left out (tests/test_kernel_selection.py holds its name on the GPU)."""
import ctypes
import json
import sys

import numpy as np

import pyddp

FIELDS = ["plant", "dtype", "N", "M", "A", "integrator", "batch", "ee_cost", "use_limits", "mpc_mode", "tl_variant"]
KFIELDS = ["bp", "fp", "sweep", "ls", "ab", "cf", "cf_bp", "cf_fp", "cf_nis"]
BATCHES = [1, 3, 64, 128, 256, 511, 512, 513, 1024, 2048, 4096]
SHAPES = [(1, 8), (2, 4), (4, 8), (4, 16), (8, 16)]
OPTIONAL = ["xw", "segmap", "ABc", "Hc"]


def grid():
    rows = []

    def add(plant, dtype, batch, M, A, integ=1, N=32, ee=0, limits=0, mpc=0, tl=0, **sel):
        rows.append(dict(plant=plant, dtype=dtype, N=N, M=M, A=A, integrator=integ, batch=batch, ee_cost=ee, use_limits=limits, mpc_mode=mpc,
                         tl_variant=tl if plant == 4 else -1, kernels=[int(sel.get(k, 0)) for k in KFIELDS]))

    for dtype in (0, 1):
        for batch in BATCHES:
            for M, A in SHAPES:
                for plant in (1, 2, 3):
                    for integ in (1, 3):
                        add(plant, dtype, batch, M, A, integ)
                add(4, dtype, batch, M, A)
                add(4, dtype, batch, M, A, ee=1, mpc=1)
            add(4, dtype, batch, 4, 8, limits=1)
            add(4, dtype, batch, 4, 8, ee=1, mpc=1, limits=1)
            add(4, dtype, batch, 4, 8, mpc=1)
            add(4, dtype, batch, 4, 8, ee=1)
        # segments longer than the 96-knot staging area of k_sweep_wg; a horizon above the thread-serial kernels' per-thread tables
        for batch in (1, 512, 513, 4096):
            for plant in (1, 2, 3, 4):
                add(plant, dtype, batch, 1, 8, 3 if plant != 4 else 1, N=128)
        for batch in (1, 512):
            for sweep in (0, 2, 3):
                add(4, dtype, batch, 4, 8, N=512, sweep=sweep)
                add(4, dtype, batch, 4, 8, N=256, sweep=sweep)
        add(2, dtype, 256, 4, 8, 3, N=512)
        add(2, dtype, 256, 4, 8, 3, N=512, cf=1)
        add(2, dtype, 256, 4, 8, 3, N=512, cf_fp=3)
        # robot tables edited after creation: no built-in model
        add(4, dtype, 3, 4, 8, tl=-1)
        add(4, dtype, 64, 4, 8, tl=-1)
        # every value of every field, on the plants it pertains to
        arm = [("bp", 4), ("fp", 5), ("sweep", 4), ("ls", 2), ("ab", 1)]
        for field, nval in arm:
            for v in range(1, nval + 1):
                for batch in (1, 512, 2048):
                    for ee in (0, 1):
                        add(4, dtype, batch, 4, 8, ee=ee, mpc=ee, **{field: v})
                if field in ("fp", "sweep", "ls"):
                    for M, A in ((1, 8), (8, 16)):
                        for ee in (0, 1):
                            add(4, dtype, 1, M, A, ee=ee, mpc=ee, **{field: v})
        for bp, fp in ((1, 1), (1, 5), (2, 2), (3, 3)):
            for batch in (2, 512):
                add(4, dtype, batch, 4, 8, bp=bp, fp=fp)
        cf = [("cf", 2), ("cf_bp", 6), ("cf_fp", 3), ("cf_nis", 8), ("ls", 2), ("sweep", 4)]
        for field, nval in cf:
            for v in range(1, nval + 1):
                for plant, shapes in ((1, [(4, 8)]), (2, [(4, 8)]), (3, [(4, 8), (4, 16)])):
                    for M, A in shapes:
                        for batch in (3, 2048):
                            for integ in (1, 3):
                                add(plant, dtype, batch, M, A, integ, **{field: v})
    return rows


def record(row, lib=None):
    c = pyddp.default_config(row["plant"], _lib_path=lib, dtype=row["dtype"], N=row["N"], M=row["M"], A=row["A"], integrator=row["integrator"], batch=row["batch"],
                             ee_cost=row["ee_cost"], use_limits=row["use_limits"], mpc_mode=row["mpc_mode"], max_iter=2, use_graph=0, tol_cost=0.0,
                             **(dict(wafr_urdf=1) if row["plant"] == 4 else {}))
    for k, v in zip(KFIELDS, row["kernels"]):
        setattr(c.kernels, k, v)
    s = pyddp.Solver(c, _lib_path=lib)
    try:
        B, N = row["batch"], row["N"]
        if row["plant"] == 4 and row["tl_variant"] < 0:
            s.set("model_I", s.get("model_I") * 1.25)
        x0 = np.zeros((B, N, s.n), s.dtype)
        x0[:, :, 0] = 0.1
        u0 = np.full((B, N, s.m), 0.01, s.dtype)
        xg = np.zeros((B, s.n), s.dtype)
        xg[:, :3] = [0.45, 0.15, 0.75][:min(3, s.n)] if row["ee_cost"] else 0.2
        s.load(x0, u0, xg)
        s.iterate(2)
        s.sync()
        names = [n for n, _ in s.time_kernels(1)]            # (the slots a path leaves empty are dropped: every name carries its slot, k_bp* k_sweep* k_fp* k_ls* k_nis*)
        have = {}
        for name in OPTIONAL:
            nb = ctypes.c_size_t(0)
            have[name] = nb.value if s.lib.pddp_array_bytes(s.h, name.encode(), ctypes.byref(nb)) == 0 else 0
        esz = 8 if row["dtype"] else 4
        xw_rec = have["xw"] // (B * N * row["A"] * esz)
        return names, xw_rec, [int(have[k] != 0) for k in OPTIONAL[1:]]
    finally:
        s.close()


def main():
    out_path, lib = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else None)
    rows = grid()
    table = []
    for i, row in enumerate(rows):
        try:
            names, xw_rec, flags = record(row, lib)
        except pyddp.PddpError as e:
            print(f"row {i} {row}: {e}", file=sys.stderr, flush=True)
            continue
        table.append([row[k] for k in FIELDS] + [row["kernels"], names, [xw_rec] + flags])
        if i % 100 == 0:
            print(f"{i} / {len(rows)}", flush=True)
    with open(out_path, "w") as f:
        f.write('{"fields": ' + json.dumps(FIELDS + ["kernels:" + ",".join(KFIELDS), "names", "arrays:xw_rec,segmap,ABc,Hc"]) + ',\n "rows": [\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in table))
        f.write("\n]}\n")
    print(f"{len(table)} rows of {len(rows)} recorded")


if __name__ == "__main__":
    main()
