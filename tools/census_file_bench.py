#!/usr/bin/env python3
"""Census record files (c2d_census_write, c2d_census_read) on one MI355X.

Workload: the census of the golden C3 case (c3_mrk421) after its first step,
replicated by c2d_census_pack / c2d_census_append to N records (default 1e6
and 1e7), written to and read from a file on tmpfs (116 bytes a record, and
8 bytes a record of `.keys`).  After one warm-up round the two calls are
timed alternately, round by round; medians:

  write  Engine.write_census_file(path): census -> plain records -> text
  read   Engine.read_census_file(path):  text -> plain records -> census

each with c2d_last_census_file_ms of the call (host time in file I/O, host
time waiting for a chunk, device time of the format / parse kernels and of
the record conversion kernels).  The format and parse kernels are also timed
alone: one chunk of N records, one launch (C2D_CENSTEXT_CHUNK = N), as
records/s and as a fraction of the HBM roofline at 192 B/record (write: 76
read + 116 written; read: 116 + 76).

Parent route, once, at --parent-records (default 1e6; 0 skips it):
Engine.save_census / load_census on the same census in the same process
(census_io.py formats and parses field by field in Python), and whether its
files equal the library's byte for byte.

    python tools/census_file_bench.py [--records 1000000,10000000] [--reps 3]
"""
from __future__ import annotations

import argparse
import filecmp
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
BYTES_PER_RECORD = 192.0


def replicated_engine(n, mode):
    """A C3 context whose census is its first step's, repeated up to n records."""
    import torch
    from compton2d_amd import abi
    from compton2d_amd.engine import Engine
    from golden_io import GoldenCase
    gc = GoldenCase("c3_mrk421")
    eng = Engine(gc.grid(comtot_mode=mode, census_capacity=max(n, 1 << 20)))
    eng.transport_step(gc.step_inputs(0))
    n0 = eng.census_count()
    rec = torch.zeros(n0 * abi.CENSUS_REC_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()      # torch's fill runs on its own stream, the pack on the context's
    eng.census_pack(0, n0, rec.data_ptr())
    if n < n0:
        eng.census_truncate(n)
    while eng.census_count() < n:
        eng.census_append(rec.data_ptr(), min(n0, n - eng.census_count()))
    assert eng.census_count() == n
    return eng


def timed(call):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def bench(n, reps, mode, tmp, parent):
    eng = replicated_engine(n, mode)
    path = os.path.join(tmp, "p001_census.dat")
    targets = {"write": lambda: eng.write_census_file(path), "read": lambda: eng.read_census_file(path)}
    wall = {k: [] for k in targets}
    parts = {k: [] for k in targets}
    for rep in range(reps + 1):                     # round 0 warms up (staging buffers, page cache)
        for k, call in targets.items():
            ms, got = timed(call)
            assert got == n
            if rep:
                wall[k].append(ms)
                parts[k].append(eng.last_census_file())
    size = os.path.getsize(path)
    assert size == 116 * n and os.path.getsize(path + ".keys") == 8 * n
    out = {"records": n, "reps": reps, "text_bytes": size, "bytes_per_record": BYTES_PER_RECORD,
           "chunk_records": int(os.environ.get("C2D_CENSTEXT_CHUNK", 1 << 20))}
    for k in targets:
        ms = float(np.median(wall[k]))
        out[k] = {"ms": ms, "ms_min_max": [min(wall[k]), max(wall[k])], "records_per_s": n / (ms * 1e-3),
                  "text_GBps": size / (ms * 1e-3) / 1e9,
                  **{f: float(np.median([p[f] for p in parts[k]])) for f in ("io_ms", "wait_ms", "kernel_ms", "convert_ms")},
                  **{f: parts[k][0][f] for f in ("device_records", "host_records", "chunks")}}
    # the kernels alone: one chunk, one launch
    os.environ["C2D_CENSTEXT_CHUNK"] = str(n)
    solo = {k: [] for k in targets}
    for rep in range(3):
        for k, call in targets.items():
            assert call() == n
            if rep:
                solo[k].append(eng.last_census_file()["kernel_ms"])
    del os.environ["C2D_CENSTEXT_CHUNK"]
    for k in targets:
        kms = float(np.median(solo[k]))
        ach = BYTES_PER_RECORD * n / (kms * 1e-3) / 1e9
        out[k]["kernel"] = {"ms": kms, "ms_min_max": [min(solo[k]), max(solo[k])], "records_per_s": n / (kms * 1e-3),
                            "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                         "frac": ach / HBM_PEAK_GBS}}
    if parent:
        ppath = os.path.join(tmp, "parent.dat")
        t_save, got = timed(lambda: eng.save_census(ppath))
        assert got == n
        same = filecmp.cmp(path, ppath, shallow=False) and filecmp.cmp(path + ".keys", ppath + ".keys", shallow=False)
        t_load, got = timed(lambda: eng.load_census(ppath))
        assert got == n
        out["parent"] = {"save_census_ms": t_save, "load_census_ms": t_load, "same_bytes_as_write": bool(same)}
        out["speedup_write_vs_save_census"] = t_save / out["write"]["ms"]
        out["speedup_read_vs_load_census"] = t_load / out["read"]["ms"]
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-records", type=int, default=1_000_000, help="0: skip save_census / load_census")
    ap.add_argument("--exact", action="store_true", help="an exact-comtot context (phi stored as it is)")
    ap.add_argument("--tmpfs-dir", default="/dev/shm")
    args = ap.parse_args()
    from compton2d_amd import abi
    mode = abi.COMTOT_EXACT if args.exact else abi.COMTOT_TABLE
    tmp = tempfile.mkdtemp(prefix="censfile", dir=args.tmpfs_dir)
    try:
        for n in (int(s) for s in args.records.split(",")):
            out = bench(n, args.reps, mode, tmp, parent=n == args.parent_records)
            out["comtot_mode"] = "exact" if args.exact else "table"
            print(json.dumps(out), flush=True)
    finally:
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
