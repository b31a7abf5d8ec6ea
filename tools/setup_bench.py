#!/usr/bin/env python3
"""Run-setup timings on one MI355X and one host core of the same box.

IC_loss on the standard grids (200 x 400: 50 854 Klein-Nishina entries, 101 708
f_Li series of 1 to 77 970 terms), after one warm-up run, `--reps` timed runs:

  kernel   c2d_icloss_kernel alone, by the library's HIP events around it
  call     the whole c2d_ic_loss call: wave list and factor table on the host,
           allocation, copies, both kernels, the table copied back
  host     c2d_ic_loss_host (libm = 0, the same arithmetic) on one core, once

and c2d_setup_electrons of the C3 deck's 270 zones against its host twin.  The
device table is checked against the host's bit for bit.

    python tools/setup_bench.py [--reps 5] [--out profiles/<run>/setup_bench.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from compton2d_amd import abi, engine, synth

    gnt, E_field, _ = abi.setup_grids()
    engine.ic_loss(gnt, E_field, device=args.device)                 # warm-up
    kernel, call = [], []
    for _ in range(args.reps):
        ms = []
        t0 = time.perf_counter()
        F = engine.ic_loss(gnt, E_field, device=args.device, kernel_ms=ms)
        call.append(1e3 * (time.perf_counter() - t0))
        kernel.append(ms[0])
    t0 = time.perf_counter()
    H = abi.ic_loss_host(gnt, E_field, libm=False)
    host_s = time.perf_counter() - t0

    d = synth.C3_DECK
    n = d["nz"] * d["nr"]
    ins = [np.full(n, float(d[k])) for k in ("tea", "amxwl", "gmin", "gmax", "p_nth")]
    engine.setup_electrons(*ins, device=args.device)
    el = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        engine.setup_electrons(*ins, device=args.device)
        el.append(1e3 * (time.perf_counter() - t0))
    t0 = time.perf_counter()
    abi.setup_electrons_host(*ins, libm=False)
    el_host_ms = 1e3 * (time.perf_counter() - t0)

    res = dict(
        workload="IC_loss 200x400 (standard grids); electrons: the C3 deck's 270 zones",
        reps=args.reps,
        icloss_kernel_ms=dict(median=statistics.median(kernel), min=min(kernel), max=max(kernel), runs=kernel),
        icloss_call_ms=dict(median=statistics.median(call), min=min(call), max=max(call), runs=call),
        icloss_host_one_core_s=host_s,
        icloss_host_over_kernel=host_s * 1e3 / statistics.median(kernel),
        icloss_device_equals_host_bitwise=bool(np.array_equal(F.view(np.uint64), H.view(np.uint64))),
        electrons_call_ms=dict(median=statistics.median(el), min=min(el), max=max(el)),
        electrons_host_ms=el_host_ms,
    )
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
