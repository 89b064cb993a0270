#!/usr/bin/env python3
"""Compares two compiler resource reports (hipcc -Rpass-analysis=kernel-resource-usage, the text `make resource-usage` greps or the whole stderr) per kernel symbol.
usage: tools/resource_compare.py OLD.txt NEW.txt [regex on the demangled name for the list of new kernels]
Prints how many symbols both reports hold and how many of them differ (with old and new figures), then the kernels only NEW has that match the regex."""
import re
import subprocess
import sys

KEYS = (("vgpr", " VGPRs: "), ("agpr", "AGPRs: "), ("sgpr", "TotalSGPRs: "), ("scratch", "ScratchSize [bytes/lane]: "), ("occ", "Occupancy [waves/SIMD]: "), ("lds", "LDS Size [bytes/block]: "))


def parse(path):
    out, cur = {}, None
    for ln in open(path, errors="replace"):
        if "Function Name:" in ln:
            cur = out.setdefault(ln.split("Function Name: ")[1].split()[0], {})
        elif cur is not None:
            for key, tag in KEYS:
                if tag in ln:
                    cur[key] = ln.split(tag)[1].split()[0]
    return out


def demangle(names):
    if not names:
        return {}
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r"\(pddp::Buffers.*", "", d).replace("void pddp::", "").replace("void ", "") for n, d in zip(names, res)}


def fmt(r):
    return " ".join(f"{k} {r.get(k, '?')}" for k, _ in KEYS)


def main():
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else ".")
    both = sorted(set(old) & set(new))
    diff = [n for n in both if any(old[n][k] != new[n][k] for k in old[n] if k in new[n])]      # (a report filtered by `make resource-usage` has no AGPR line)
    print(f"{len(old)} kernels in OLD, {len(new)} in NEW, {len(both)} in both, {len(diff)} of those differ, {len(set(old) - set(new))} only in OLD")
    names = demangle(diff)
    for n in diff:
        print(f"DIFF {names[n][:110]}\n     old {fmt(old[n])}\n     new {fmt(new[n])}")
    only = sorted(set(new) - set(old))
    names = demangle(only)
    shown = [n for n in only if pat.search(names[n])]
    print(f"{len(only)} kernels only in NEW, {len(shown)} match:")
    for n in sorted(shown, key=lambda n: names[n]):
        print(f"  {names[n][:118]:118s} {fmt(new[n])}")
    spills = [n for n in new if new[n].get("scratch", "0") != "0" and n not in old]
    print(f"new kernels with scratch: {len(spills)}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
