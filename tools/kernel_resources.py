"""Table of the compiler-reported resources of every kernel in a build log.

Build with the remarks on and keep the log:

    make -C compton2d_amd/csrc BUILD=/tmp/b OUT=/tmp/b/lib.so \
        EXTRA=-Rpass-analysis=kernel-resource-usage 2> build.log
    python tools/kernel_resources.py build.log [other.log]

One log: a table (kernel, SGPRs, VGPRs, AGPRs, scratch, occupancy, SGPR
spills, VGPR spills, LDS).  Two logs: the kernels of the first whose figures
differ in the second or that the second lacks (a kernel template that has
gained parameters is matched with its instance that has zeros there); exit
status 1 if there are any.
"""
from __future__ import annotations

import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def parse(path: str) -> dict:
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = m.group(2)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(d: str) -> str:
    d = re.sub(r"\([^()]*(\([^()]*\)[^()]*)*\)$", "", d)      # the trailing argument list only
    return d.replace("void ", "").replace("c2d::", "")


def table(res: dict) -> str:
    names = demangle(sorted(res))
    rows = ["kernel | " + " | ".join(FIELDS)]
    for sym in sorted(res, key=lambda s: short(names[s])):
        rows.append(short(names[sym]) + " | " + " | ".join(res[sym].get(f, "?") for f in FIELDS))
    return "\n".join(rows)


def main(argv) -> int:
    if len(argv) == 2:
        print(table(parse(argv[1])))
        return 0
    a, b = parse(argv[1]), parse(argv[2])
    names = demangle(sorted(a))
    nb = demangle(sorted(b))
    by_name = {short(nb[s]).replace(" ", ""): b[s] for s in b}

    def partner(sym):
        """The second log's figures of the same kernel; a kernel that has gained
        template parameters since is its instance with the new ones 0."""
        if sym in b:
            return b[sym]
        n = short(names[sym]).replace(" ", "")
        for extra in (",0>", ",0,0>"):
            if n.endswith(">") and n[:-1] + extra in by_name:
                return by_name[n[:-1] + extra]
        return None

    diff = [short(names[s]) for s in sorted(a) if a[s] != partner(s)]
    print("%d kernels in %s, %d in %s, %d of the first differ or are missing in the second"
          % (len(a), argv[1], len(b), argv[2], len(diff)))
    for d in diff:
        print("  " + d)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
