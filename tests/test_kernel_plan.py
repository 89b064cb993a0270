"""The kernel selection as host code (csrc/kernel_plan.hpp), held without a GPU.

tests/golden/kernel_selection_table.json is what handles of the library REPORTED (pddp_time_kernels) and ALLOCATED (xw, segmap, ABc, Hc) over a grid of configurations
that straddles every crossover and every pddp_config.kernels value, recorded once by tools/kernel_plan_table.py on a GPU.  tests/native/kernel_plan_host_check.cpp
(its own main, -fsanitize=address,undefined) feeds every row's configuration through make_kernel_plan + plan_kernel_names and has to print the same; by hand it asserts
the choices that names do not show, and what plan_fp_launch makes of the plan in each of the seven ways the forward pass is asked for.  The launches follow the same enums
(solver_impl.hpp launch_bp / launch_fp / launch_nis), tests/test_kernel_selection.py holds that on the GPU."""
import json
import os
import re
import subprocess

import pytest

import pyddp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["plant", "dtype", "N", "M", "A", "integrator", "batch", "ee_cost", "use_limits", "mpc_mode", "tl_variant"]
KFIELDS = ["bp", "fp", "sweep", "ls", "ab", "cf", "cf_bp", "cf_fp", "cf_nis"]


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kernel_plan") / "kernel_plan_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "parallel-ddp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "kernel_plan_host_check.cpp"), "-o", exe])
    return exe


def test_choices_that_names_do_not_show(host_check):
    out = subprocess.run([host_check], capture_output=True, text=True)
    assert out.returncode == 0 and "kernel_plan_host_check: ok" in out.stdout, out.stdout + out.stderr


def test_the_header_is_host_code_and_reads_no_environment():
    src = open(os.path.join(ROOT, "parallel-ddp_amd", "csrc", "kernel_plan.hpp")).read()
    assert "getenv" not in src and "std::string" not in src
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["cstddef", "../../include/pddp.h"]


def test_enum_values_are_the_numbers_of_the_header_and_of_the_binding(host_check):
    out = subprocess.run([host_check, "sel"], capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        field, *pairs = line.split()
        got[field] = [tuple(p.split("=")) for p in pairs]
    assert list(got) == KFIELDS == [f for f, _ in pyddp.PddpKernelSelection._fields_]
    header = open(os.path.join(ROOT, "include", "pddp.h")).read()
    struct = header[header.index("typedef struct pddp_kernel_selection {"):header.index("} pddp_kernel_selection;")]
    for field, pairs in got.items():
        assert tuple(n for n, _ in pairs) == pyddp.KERNEL_NAMES[field]                             # the order of the binding's names ...
        assert [int(v) for _, v in pairs] == list(range(1, len(pairs) + 1))                       # ... is the enum's numbering ...
        comment = struct[struct.index(f"    int {field};"):]
        comment = comment[:comment.index("*/")]
        for name, v in pairs:                                                                      # ... and the header documents it
            assert re.search(rf"\b{v} {name}\b", comment), (field, name, v)


def _recorded_rows_through(host_check, command):
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_selection_table.json")))
    assert table["fields"][:len(FIELDS)] == FIELDS and table["fields"][len(FIELDS)] == "kernels:" + ",".join(KFIELDS)
    rows = table["rows"]
    assert len(rows) >= 1000
    text = "".join(" ".join(str(v) for v in r[:len(FIELDS)] + r[len(FIELDS)]) + "\n" for r in rows)
    out = subprocess.run([host_check, command], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(rows)
    return rows, lines


def test_every_recorded_row_resolves_to_the_recorded_kernels_and_arrays(host_check):
    rows, lines = _recorded_rows_through(host_check, "rows")
    wrong = []
    for r, line in zip(rows, lines):
        names, arrays = line.split("|")
        if names.split() != r[len(FIELDS) + 1] or [int(v) for v in arrays.split()] != r[len(FIELDS) + 2]:
            wrong.append((r, line))
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ, the first: {wrong[:5]}"


def test_every_mode_of_the_forward_pass_resolves_on_every_recorded_row(host_check):
    """plan_fp_launch over the recorded rows, all seven modes (under the sanitizers): production launches the recorded names of slots 1 and 2 -- what GPU handles
    reported before the launch followed the plan's enums --, a sweep-only mode no rollout kernel, a mode without a sweep launch none."""
    rows, lines = _recorded_rows_through(host_check, "fp")
    modes = ["production", "sweep only", "rollouts only", "initial rollout", "hook", "hook, fused sweep", "hook, rollouts"]
    wrong = []
    for r, line in zip(rows, lines):
        got = {}
        for mode, rec in zip(modes, line.split(" | ")):
            sweep, fp, seed, flags = rec.split(",")
            got[mode] = dict(sweep=sweep, fp=fp, seed=int(seed), **dict(zip(("store", "maps", "ls", "xw", "stale"), (int(f) for f in flags))))
        assert len(got) == 7, line
        names = r[len(FIELDS) + 1]
        recorded = ["".join(n for n in names if n.startswith(prefix)) or "-" for prefix in ("k_sweep", "k_fp")]
        ok = [got["production"]["sweep"], got["production"]["fp"]] == recorded
        ok = ok and got["sweep only"]["fp"] == got["hook, fused sweep"]["fp"] == "-"
        ok = ok and all(got[m]["sweep"] == "-" for m in ("rollouts only", "initial rollout", "hook, rollouts"))
        ok = ok and all(got[m]["fp"].startswith("k_fp") for m in modes if m not in ("sweep only", "hook, fused sweep"))
        ok = ok and [got[m]["seed"] for m in modes] == [0, 0, 0, 1, 0, 0, 2] and [got[m]["store"] for m in modes] == [0, 0, 0, 0, 1, 1, 1]
        M = r[FIELDS.index("M")]
        ok = ok and (M > 1 or all(got[m]["sweep"] == "-" for m in modes))
        if not ok:
            wrong.append((r, line))
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ, the first: {wrong[:5]}"
