#!/usr/bin/env python3
"""Escape-event file read-back (c2d_events_read, c2d_obs_set_accumulate_file)
on one MI355X.

Workload: N escape events (jittered copies of the reference's own events,
tests/golden/obs.npz; default 1.1e7 = one C3 step) written once to a file on
tmpfs by Engine.events_write_from (105 bytes a record).  After one warm-up
round the targets are timed alternately, round by round; medians:

  read_host    Engine.events_read(path): parse on the device, events to a numpy array
  read_device  Engine.events_read(path, device=True): events stay in HBM
  set_file     Engine.obs_set_accumulate_file(path) into a SED + light-curve set
               (sed_mrk421, lc_mrk421): parse and bin chunk by chunk

each with c2d_last_events_read_ms of the call (host time in read(), host time
waiting for a chunk, parse-kernel device time, records by parser).  The parse
kernel is also timed alone: one chunk of N records, one launch
(C2D_EVTEXT_CHUNK = N), as events/s and as a fraction of the HBM roofline at
161 B/event (105 read + 56 written).

Baseline, the route before the device parser: observer.read_events(path)
(f.read().split() and numpy's float64 conversion) followed by
Engine.obs_set_accumulate(events), once, on the same file (--parent-events
limits it to a prefix of the file; the time is then scaled to N).

    python tools/evread_bench.py [--events 11000000] [--reps 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

HBM_PEAK_GBS = 8000.0
BYTES_PER_EVENT = 161.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=11_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-events", type=int, default=0, help="0: the whole file")
    ap.add_argument("--tmpfs-dir", default="/dev/shm")
    args = ap.parse_args()
    import torch
    from compton2d_amd import observer
    from compton2d_amd.engine import obs_engine
    from obs_bench import device_events
    from test_gpu_observe import _binning

    n = args.events
    dev = device_events(n)
    eng = obs_engine(0)
    bins = [_binning(nm)[1] for nm in ("sed_mrk421", "lc_mrk421")]
    tmp = tempfile.mkdtemp(prefix="evread", dir=args.tmpfs_dir)
    path = os.path.join(tmp, "p001_evb.dat")
    try:
        eng.events_write_from(dev, path)
        size = os.path.getsize(path)
        assert size == 105 * n, size
        del dev
        torch.cuda.empty_cache()

        def set_file():
            eng.obs_set_clear()
            ids = [eng.obs_set_add(b) for b in bins]
            assert eng.obs_set_accumulate_file(path) == n
            return ids

        targets = {"read_host": lambda: eng.events_read(path),
                   "read_device": lambda: eng.events_read(path, device=True),
                   "set_file": set_file}
        wall = {k: [] for k in targets}
        parts = {k: [] for k in targets}
        for rep in range(args.reps + 1):                    # round 0 warms up (staging buffers, page cache)
            for k, call in targets.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = call()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                del r
                if rep:
                    wall[k].append(dt)
                    parts[k].append(eng.last_events_read())
        counts = [eng.obs_set_result(i)[2].sum() for i in range(len(bins))]

        out = {"events": n, "reps": args.reps, "text_bytes": size, "bytes_per_event": BYTES_PER_EVENT,
               "chunk_events": int(os.environ.get("C2D_EVTEXT_CHUNK", 1 << 20))}
        for k in targets:
            ms = float(np.median(wall[k]))
            out[k] = {"ms": ms, "ms_min_max": [min(wall[k]), max(wall[k])], "events_per_s": n / (ms * 1e-3),
                      "text_GBps": size / (ms * 1e-3) / 1e9,
                      **{f: float(np.median([p[f] for p in parts[k]]))
                         for f in ("io_ms", "wait_ms", "kernel_ms", "host_parse_ms")},
                      **{f: parts[k][0][f] for f in ("canonical", "host_parsed", "exact_fields", "chunks")}}
            print(k, json.dumps(parts[k][-1]), file=sys.stderr)          # c2d_last_events_read_ms of the last round

        # the kernel alone: one chunk, one launch, on a context of its own
        os.environ["C2D_EVTEXT_CHUNK"] = str(n)
        solo = []
        with obs_engine(0) as e1:
            for rep in range(3):
                assert e1.events_read_into(path, np.zeros((0, 7))) == n
                if rep:
                    solo.append(e1.last_events_read()["kernel_ms"])
        del os.environ["C2D_EVTEXT_CHUNK"]
        kms = float(np.median(solo))
        ach = BYTES_PER_EVENT * n / (kms * 1e-3) / 1e9
        out["kernel"] = {"ms": kms, "ms_min_max": [min(solo), max(solo)], "events_per_s": n / (kms * 1e-3),
                         "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                      "frac": ach / HBM_PEAK_GBS}}

        # the parent route: Python parses, then the set bins host events
        m = args.parent_events or n
        ppath = path
        if m < n:
            ppath = os.path.join(tmp, "prefix.dat")
            with open(path, "rb") as f, open(ppath, "wb") as g:
                g.write(f.read(105 * m))
        t0 = time.perf_counter()
        ev = observer.read_events(ppath)
        t1 = time.perf_counter()
        eng.obs_set_clear()
        ids = [eng.obs_set_add(b) for b in bins]
        eng.obs_set_accumulate(ev)
        t2 = time.perf_counter()
        assert len(ev) == m
        same = m < n or all(eng.obs_set_result(i)[2].sum() == c for i, c in zip(ids, counts))
        out["parent"] = {"events": m, "read_events_ms": (t1 - t0) * 1e3 * n / m,
                         "obs_set_accumulate_ms": (t2 - t1) * 1e3 * n / m, "total_ms": (t2 - t0) * 1e3 * n / m,
                         "scaled": m < n, "same_counts_as_set_file": bool(same)}
        out["speedup_set_file_vs_parent"] = out["parent"]["total_ms"] / out["set_file"]["ms"]
        out["speedup_read_host_vs_read_events"] = out["parent"]["read_events_ms"] / out["read_host"]["ms"]
        print(json.dumps(out))
    finally:
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)
        eng.close()


if __name__ == "__main__":
    main()
