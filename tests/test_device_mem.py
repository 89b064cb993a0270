"""The host-only parts of a handle's memory management, held without a GPU.

csrc/device_mem.hpp is the one owning buffer type behind every block of device and pinned memory a handle keeps (solver_impl.hpp); tests/native/device_mem_host_check.cpp
(its own main, -fsanitize=address,undefined) instantiates it with a counting host policy and asserts what reserve keeps, releases and allocates, what a failed
allocation leaves, what moves transfer, and that every block is released exactly once -- alone, and as an element of a vector.  csrc/slots.hpp for_each_slot_run names
the runs of consecutive slots that the cost-table rows travel in; tests/native/slots_host_check.cpp holds it on six index lists beside the slot tables' addressing."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-ddp_amd", "csrc")


def _run_host_check(tmp_path, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and name + ": ok" in out.stdout, out.stdout + out.stderr


def test_the_owning_buffer_with_a_counting_policy(tmp_path):
    _run_host_check(tmp_path, "device_mem_host_check")


def test_runs_of_consecutive_slots_and_the_slot_tables(tmp_path):
    _run_host_check(tmp_path, "slots_host_check")


def test_the_buffer_template_is_host_code_and_reads_no_environment():
    src = open(os.path.join(CSRC, "device_mem.hpp")).read()
    assert "getenv" not in src and not re.search(r"\bhip[A-Z]\w*\s*\(", src)
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["cstddef"]


def test_the_handle_releases_nothing_by_hand():
    """every block a handle owns is a MemBuf: no release call and no capacity field of its own is left in solver_impl.hpp, and the run loop exists once"""
    impl = open(os.path.join(CSRC, "solver_impl.hpp")).read()
    assert not re.search(r"\bhip(Host)?Free\s*\(", impl) and not re.search(r"\bhip(Host)?Malloc\s*\(", impl)
    for gone in ("h_stage_bytes", "d_slot_stage_cap", "scratch_cap", "d_simb_cap", "d_simb_plan_cap", "h_simb_cap"):
        assert gone not in impl, gone
    loop = "while (j < count && " + "idx[j] == idx[j - 1] + 1)"      # (in two pieces: this file is not an occurrence)
    found = []
    for top in ("parallel-ddp_amd", "tests", "include", "tools"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".hpp", ".h", ".hip", ".cpp", ".cuh", ".inc", ".c")):
                    found += [os.path.join(d, f)] * open(os.path.join(d, f), errors="replace").read().count(loop)
    assert found == [os.path.join(CSRC, "slots.hpp")], found
