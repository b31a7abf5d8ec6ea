#!/usr/bin/env python3
"""Escape-event file throughput (c2d_events_write_from) on one MI355X.

Workload: N escape events resident in HBM (jittered copies of the reference's
own events, tests/golden/obs.npz; default 1.1e7 = one C3 step), written as
p###_evb.dat text (105 bytes a record).  After one warm-up round the targets
are timed alternately, round by round; medians over the rounds:

  kernel     the formatting kernel alone (the library's HIP events around it),
             events/s and the fraction of the HBM roofline at 161 B/event (56
             read + 105 written).  Timed in calls of their own with the chunk
             set to N (C2D_EVTEXT_CHUNK): one launch with no copy queued in
             front of it -- between chunks the kernel's events also span its
             wait for the previous chunk's copy (reported as kernel_in_pipeline_ms)
  devnull    the whole call into /dev/null: kernel + copy to pinned memory
  tmpfs      the whole call to a file on tmpfs (--tmpfs-dir, default /dev/shm)
  disk       the whole call to a file in --disk-dir (default: the working directory)

Baseline, the route without the device formatter: the events copied to the
host, then formatted on one core by the same header's host function and by
glibc snprintf("%.6e") (tests/c/fmt_wrap.c, gcc -O2) on --cpu-events events,
scaled to N, and observer.write_events (the Python loop) on --py-events.

    python tools/evtext_bench.py [--events 11000000] [--reps 7]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

HBM_PEAK_GBS = 8000.0
BYTES_PER_EVENT = 161.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=11_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-events", type=int, default=1_000_000)
    ap.add_argument("--py-events", type=int, default=100_000)
    ap.add_argument("--tmpfs-dir", default="/dev/shm")
    ap.add_argument("--disk-dir", default=".")
    args = ap.parse_args()
    import torch
    import fmt_cases as FC
    from compton2d_amd import observer
    from compton2d_amd.engine import obs_engine
    from obs_bench import device_events

    n = args.events
    dev = device_events(n)
    eng = obs_engine(0)
    tmp = {"tmpfs": tempfile.mkdtemp(prefix="evtext", dir=args.tmpfs_dir),
           "disk": tempfile.mkdtemp(prefix="evtext", dir=args.disk_dir)}
    paths = {"devnull": "/dev/null", "tmpfs": os.path.join(tmp["tmpfs"], "p001_evb.dat"),
             "disk": os.path.join(tmp["disk"], "p001_evb.dat")}
    wall = {k: [] for k in paths}
    parts = {k: [] for k in paths}
    try:
        for rep in range(args.reps + 1):                    # round 0 warms up (staging buffers, page cache)
            for k, p in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.events_write_from(dev, p)
                dt = (time.perf_counter() - t0) * 1e3
                if rep:
                    wall[k].append(dt)
                    parts[k].append(eng.last_events_write())
        # the kernel alone: one chunk, one launch, on a context of its own (N x 105 B of staging)
        os.environ["C2D_EVTEXT_CHUNK"] = str(n)
        solo = []
        with obs_engine(0) as e1:
            for rep in range(args.reps + 1):
                e1.events_write_from(dev, "/dev/null")
                if rep:
                    solo.append(e1.last_events_write()["kernel_ms"])
        del os.environ["C2D_EVTEXT_CHUNK"]
        size = os.path.getsize(paths["tmpfs"])
        assert size == 105 * n, size

        out = {"events": n, "reps": args.reps, "text_bytes": size, "bytes_per_event": BYTES_PER_EVENT,
               "chunk_events": int(os.environ.get("C2D_EVTEXT_CHUNK", 1 << 20)),
               "chunks": parts["devnull"][0]["chunks"]}
        kms = float(np.median(solo))
        ach = BYTES_PER_EVENT * n / (kms * 1e-3) / 1e9
        out["kernel"] = {"ms": kms, "ms_min_max": [min(solo), max(solo)],
                         "kernel_in_pipeline_ms": float(np.median([p["kernel_ms"] for p in parts["devnull"]])),
                         "events_per_s": n / (kms * 1e-3),
                         "scan_ms": float(np.median([p["scan_ms"] for p in parts["devnull"]])),
                         "ambiguous_values": parts["devnull"][0]["ambiguous"],
                         "multilimb_values": parts["devnull"][0]["multilimb"],
                         "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                      "frac": ach / HBM_PEAK_GBS}}
        for k in paths:
            ms = float(np.median(wall[k]))
            out[k] = {"ms": ms, "ms_min_max": [min(wall[k]), max(wall[k])], "events_per_s": n / (ms * 1e-3),
                      "text_GBps": size / (ms * 1e-3) / 1e9,
                      "host_wait_ms": float(np.median([p["wait_ms"] for p in parts[k]])),
                      "host_fwrite_ms": float(np.median([p["io_ms"] for p in parts[k]]))}

        # the route without the device formatter: events to the host, one core formats
        t0 = time.perf_counter()
        host_ev = dev.cpu().numpy()
        d2h = (time.perf_counter() - t0) * 1e3
        m = min(args.cpu_events, n)
        sample = np.ascontiguousarray(host_ev[:m])
        with tempfile.TemporaryDirectory() as d:
            hf = FC.HostFmt(d)
            buf = C.create_string_buffer(14 * 7 * m)
            px = sample.ctypes.data_as(C.POINTER(C.c_double))
            base = {}
            for name, call in (("header", lambda: hf.lib.fw_format(px, 7 * m, buf, None, None)),
                               ("glibc_snprintf", lambda: hf.lib.fw_format_glibc(px, 7 * m, buf))):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    call()
                    ts.append((time.perf_counter() - t0) * 1e3)
                f_ms = float(np.median(ts)) * n / m
                base[name] = {"format_ms_scaled": f_ms, "total_ms": d2h + f_ms + out["tmpfs"]["host_fwrite_ms"],
                              "ns_per_value": float(np.median(ts)) * 1e6 / (7 * m)}
        mp = min(args.py_events, n)
        t0 = time.perf_counter()
        observer.write_events(os.path.join(tmp["tmpfs"], "py.dat"), host_ev[:mp])
        py_ms = (time.perf_counter() - t0) * 1e3 * n / mp
        out["baseline"] = {"events_d2h_ms": d2h, "sample_events": m, "cores": 1,
                           "note": "total = events_d2h + format (scaled from the sample) + the tmpfs fwrite time "
                                   "of the device route; the separators are not written by the host formatters",
                           **base, "python_write_events_ms_scaled": py_ms, "python_sample_events": mp}
        out["speedup_tmpfs_vs_header_baseline"] = base["header"]["total_ms"] / out["tmpfs"]["ms"]
        out["speedup_tmpfs_vs_glibc_baseline"] = base["glibc_snprintf"]["total_ms"] / out["tmpfs"]["ms"]
        print(json.dumps(out))
    finally:
        for k in ("tmpfs", "disk"):
            for f in os.listdir(tmp[k]):
                os.unlink(os.path.join(tmp[k], f))
            os.rmdir(tmp[k])
        eng.close()


if __name__ == "__main__":
    main()
