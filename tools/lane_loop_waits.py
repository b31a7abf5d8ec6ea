#!/usr/bin/env python3
"""Wait audit of the transport kernels' compiled code: where a wave waits for
its vector-memory counter, and where it uses flat memory instructions.

Builds csrc/transport.hip to gfx950 assembly with the Makefile's own flags for
one variant (the compile line is taken from `make -n`, with -c replaced by
--cuda-device-only -S) into a temporary directory, and lists for a chosen
kernel, in program order,

  * every s_waitcnt that carries a vmcnt field, and
  * every flat_* instruction (a flat access counts in vmcnt and lgkmcnt, so
    waiting for it drains both),

each with the instruction that follows it and the vector-memory instructions
issued since the previous listed line.  Lines inside the lane loop (the
kernel's largest outermost loop) are marked with L.  Nothing else is looked at.

    python tools/lane_loop_waits.py --variant fast --kernel 'bundle_kernel_fast<0,1>'
    python tools/lane_loop_waits.py --variant exact --summary
"""
from __future__ import annotations

import argparse
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "compton2d_amd" / "csrc"
VMEM = ("global_", "flat_", "buffer_", "scratch_")

_KERNEL = re.compile(r"^([A-Za-z_][\w$.]*):\s+; @")
_BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+)|; %bb\.\d+):")
_IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
_HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")


class Insn:
    __slots__ = ("line", "text", "loop")

    def __init__(self, line, text, loop):
        self.line = line      # line number within the kernel's listing
        self.text = text
        self.loop = loop      # label of the outermost loop around it, or None

    @property
    def op(self):
        return self.text.split(None, 1)[0]

    @property
    def is_vmem(self):
        return self.op.startswith(VMEM)

    @property
    def is_flat(self):
        return self.op.startswith("flat_")

    @property
    def is_vm_wait(self):
        return self.op == "s_waitcnt" and "vmcnt(" in self.text


class Kernel:
    def __init__(self, symbol, name, insns):
        self.symbol = symbol
        self.name = name
        self.insns = insns
        sizes = {}
        for i in insns:
            if i.loop:
                sizes[i.loop] = sizes.get(i.loop, 0) + 1
        # the lane loop: the largest outermost loop of the kernel
        self.lane_loop = max(sizes, key=sizes.get) if sizes else None

    def in_lane_loop(self, insn):
        return self.lane_loop is not None and insn.loop == self.lane_loop

    def events(self):
        """(insn, next insn or None, [vmem since the previous event]) per vmcnt wait / flat_*."""
        out, since = [], []
        for n, i in enumerate(self.insns):
            if i.is_vm_wait or i.is_flat:
                nxt = self.insns[n + 1] if n + 1 < len(self.insns) else None
                out.append((i, nxt, since))
                since = []
            if i.is_vmem:
                since.append(i)
        return out

    def counts(self):
        ll = [i for i in self.insns if self.in_lane_loop(i)]
        return {
            "vm_waits": sum(i.is_vm_wait for i in self.insns),
            "vm_waits_0": sum(i.is_vm_wait and "vmcnt(0)" in i.text for i in self.insns),
            "flat": sum(i.is_flat for i in self.insns),
            "loop_vm_waits": sum(i.is_vm_wait for i in ll),
            "loop_vm_waits_0": sum(i.is_vm_wait and "vmcnt(0)" in i.text for i in ll),
            "loop_flat": sum(i.is_flat for i in ll),
        }


def hipcc_path():
    return shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))


def compile_line(variant: str, csrc: Path, out: Path) -> list:
    """The Makefile's compile line of transport_<variant>.o, turned into an assembly build."""
    build = out.parent / "obj"
    target = "%s/transport_%s.o" % (build, variant)
    txt = subprocess.run(["make", "-n", "-B", "-C", str(csrc), "BUILD=%s" % build, target],
                         check=True, capture_output=True, text=True).stdout
    line = next(ln for ln in txt.splitlines() if " -c " in ln and "transport.hip" in ln)
    args = shlex.split(line)
    o = args.index("-o")
    del args[o:o + 2]
    args[args.index("-c")] = "-S"
    return args + ["--cuda-device-only", "-o", str(out)]


def build_asm(variant: str, csrc: Path = CSRC) -> str:
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / ("transport_%s.s" % variant)
        subprocess.run(compile_line(variant, csrc, out), check=True, cwd=str(csrc), capture_output=True)
        return out.read_text()


def demangle(symbols):
    """name<args> of the c2d:: kernels' Itanium symbols (integer template arguments only)."""
    out = []
    for s in symbols:
        m = re.match(r"_ZN3c2d(?:12_GLOBAL__N_1)?(\d+)", s)
        if not m:
            out.append(s)
            continue
        n = int(m.group(1))
        name, rest = s[m.end():m.end() + n], s[m.end() + n:]
        t = re.match(r"I((?:Li\d+E)+)E", rest)
        if t:
            name += "<%s>" % ",".join(re.findall(r"Li(\d+)E", t.group(1)))
        out.append(name)
    return out


def parse(asm: str) -> list:
    """The kernels (and device functions) of an assembly listing."""
    raw, cur = [], None
    for ln in asm.splitlines():
        m = _KERNEL.match(ln)
        if m:
            cur = (m.group(1), [])
            raw.append(cur)
        elif ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            cur[1].append(ln)
    names = demangle([s for s, _ in raw])
    return [Kernel(s, n, _insns(lines)) for (s, lines), n in zip(raw, names)]


def _insns(lines):
    # pass 1: the blocks with their loop comments; the outermost loop of every loop header
    blocks, root, in_comment = [], {}, False
    for n, ln in enumerate(lines):
        m = _BLOCK.match(ln)
        if m:
            blocks.append([n, m.group(1), ln])
        elif in_comment and re.match(r"^\s+;", ln):
            blocks[-1][2] += "\n" + ln       # the label's loop comment continues
        in_comment = bool(m) or (in_comment and bool(re.match(r"^\s+;", ln)))
    for _, label, com in blocks:
        h = _HEADER.search(com)
        if h and label:
            top = [p for p, d in _PARENT.findall(com) if d == "1"]
            root[label] = label if h.group(1) == "1" else (top[0] if top else None)
    # pass 2: every instruction with the outermost loop of its block
    starts = {}
    for n, label, com in blocks:
        if _HEADER.search(com) and label:
            starts[n] = root.get(label)
        else:
            m = _IN_LOOP.search(com)
            starts[n] = root.get(m.group(1)) if m else None
    out, loop = [], None
    for n, ln in enumerate(lines):
        if n in starts:
            loop = starts[n]
        if ln.startswith("\t") and not ln.startswith(("\t.", "\t;")):
            out.append(Insn(n + 1, ln.split(";")[0].strip(), loop))
    return out


def find(kernels, pattern):
    hit = [k for k in kernels if pattern in k.name or pattern in k.symbol]
    if len(hit) != 1:
        raise SystemExit("--kernel %r matches %s" % (pattern, [k.name for k in hit] or "nothing"))
    return hit[0]


def report(k: Kernel) -> str:
    out = ["%s  (lane loop: %s, %d instructions)" % (k.name, k.lane_loop, len(k.insns))]
    for i, nxt, since in k.events():
        out.append("%s %6d  %s" % ("L" if k.in_lane_loop(i) else " ", i.line, i.text))
        out.append("            next:  %s" % (nxt.text if nxt else "-"))
        if since:
            out.append("            since: %s" % "; ".join(s.text for s in since))
    return "\n".join(out)


def summary(kernels) -> str:
    out = ["%-44s %9s %9s %5s | %9s %9s %5s" % ("kernel", "vm waits", "vmcnt(0)", "flat",
                                                "loop: vm", "vmcnt(0)", "flat")]
    for k in kernels:
        c = k.counts()
        if c["vm_waits"] or c["flat"]:
            out.append("%-44s %9d %9d %5d | %9d %9d %5d" % (
                k.name[:44], c["vm_waits"], c["vm_waits_0"], c["flat"],
                c["loop_vm_waits"], c["loop_vm_waits_0"], c["loop_flat"]))
    return "\n".join(out)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--variant", choices=("exact", "fast"), default="fast")
    ap.add_argument("--csrc", default=str(CSRC),
                    help="the csrc directory to build (default: this tree's; another checkout's for a before/after)")
    ap.add_argument("--kernel", default="bundle_kernel_fast<0,1>",
                    help="substring of the kernel's demangled name or symbol")
    ap.add_argument("--summary", action="store_true", help="counts per kernel")
    a = ap.parse_args(argv)
    kernels = parse(build_asm(a.variant, Path(a.csrc)))
    print(summary(kernels) if a.summary else report(find(kernels, a.kernel)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
