#!/usr/bin/env python3
"""Binary checkpoints (c2d_checkpoint_write, c2d_checkpoint_read) on one MI355X.

Workload: the census of the golden C3 case (c3_mrk421) after its first step,
replicated by c2d_census_pack / c2d_census_append to N records (default 1e7).
After one warm-up round the legs are timed alternately, round by round;
medians, each with c2d_last_checkpoint_ms of the call (host time in file I/O,
host time waiting for a chunk, device time of the gather or verify kernels):

  write       Engine.checkpoint_write to a file on tmpfs (64 B a record)
  write_null  the same to /dev/null (a device is written in place)
  read        Engine.checkpoint_read of the tmpfs file (a file is needed to
              read: there is no /dev/null leg)

and beside them, on the same census in the same process, the text route:
Engine.write_census_file / read_census_file (116 B a record and 8 B of key).

--kernels: the gather-and-digest kernel against c2d_census_pack's kernel.
Five rounds, alternating: one checkpoint_write to /dev/null with the whole
census as one chunk (C2D_CKPT_CHUNK = N: kernel_ms is one gather launch) and
one Engine.census_pack of the whole census into a device buffer, timed from
the host around the synchronous call.  Under `rocprofv3 --kernel-trace
--stats -- python tools/ckpt_bench.py --kernels` the trace holds both
kernels' device times.

    python tools/ckpt_bench.py [--records 10000000] [--reps 3] [--kernels]
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
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
sys.path.insert(0, str(ROOT / "tools"))

from census_file_bench import replicated_engine, timed  # noqa: E402


def med(rows, key):
    return float(np.median([r[key] for r in rows]))


def bench(n, reps, mode, tmp):
    eng = replicated_engine(n, mode)
    path = os.path.join(tmp, "run.ckpt")
    text = os.path.join(tmp, "p001_census.dat")
    legs = {
        "write": lambda: eng.checkpoint_write(path),
        "write_null": lambda: eng.checkpoint_write("/dev/null"),
        "read": lambda: eng.checkpoint_read(path)[0],
        "text_write": lambda: eng.write_census_file(text),
        "text_read": lambda: eng.read_census_file(text),
    }
    wall = {k: [] for k in legs}
    parts = {k: [] for k in legs}
    for rep in range(reps + 1):                     # round 0 warms up (staging buffers, page cache)
        for k, call in legs.items():
            ms, got = timed(call)
            assert got == n, (k, got)
            if rep:
                wall[k].append(ms)
                parts[k].append(eng.last_census_file() if k.startswith("text") else eng.last_checkpoint())
    out = {"records": n, "reps": reps, "file_bytes": os.path.getsize(path),
           "text_bytes": os.path.getsize(text) + os.path.getsize(text + ".keys"),
           "chunk_records": int(os.environ.get("C2D_CKPT_CHUNK", 1 << 20))}
    for k in legs:
        ms = float(np.median(wall[k]))
        out[k] = {"ms": ms, "ms_min_max": [min(wall[k]), max(wall[k])], "records_per_s": n / (ms * 1e-3),
                  **{f: med(parts[k], f) for f in ("io_ms", "wait_ms", "kernel_ms")}, "chunks": parts[k][0]["chunks"]}
    eng.close()
    return out


def kernels(n, mode, rounds=5):
    import torch
    from compton2d_amd import abi
    eng = replicated_engine(n, mode)
    buf = torch.empty(n * abi.CENSUS_REC_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    os.environ["C2D_CKPT_CHUNK"] = str(n)
    gather, pack = [], []
    for rep in range(rounds + 1):                   # round 0 warms up
        assert eng.checkpoint_write("/dev/null") == n
        g = eng.last_checkpoint()
        assert g["chunks"] == 1
        t0 = time.perf_counter()
        eng.census_pack(0, n, buf.data_ptr())       # synchronous on the context's stream
        p = (time.perf_counter() - t0) * 1e3
        if rep:
            gather.append(g["kernel_ms"])
            pack.append(p)
    del os.environ["C2D_CKPT_CHUNK"]
    eng.close()
    gm, pm = float(np.median(gather)), float(np.median(pack))
    return {"records": n, "rounds": rounds, "gather_kernel_ms": gm, "gather_ms_all": gather,
            "pack_call_ms_host": pm, "pack_call_ms_all": pack, "gather_over_pack_call": gm / pm,
            "gather_GBps": 128.0 * n / (gm * 1e-3) / 1e9,
            "note": "pack is host time around the synchronous call (launch and sync included); the kernel's "
                    "device time is in the rocprofv3 kernel trace of this run"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", action="store_true", help="gather kernel against the pack kernel only")
    ap.add_argument("--exact", action="store_true", help="an exact-comtot context (phi stored as it is)")
    ap.add_argument("--tmpfs-dir", default="/dev/shm")
    args = ap.parse_args()
    from compton2d_amd import abi
    mode = abi.COMTOT_EXACT if args.exact else abi.COMTOT_TABLE
    if args.kernels:
        print(json.dumps(kernels(args.records, mode)), flush=True)
        return
    tmp = tempfile.mkdtemp(prefix="ckpt", dir=args.tmpfs_dir)
    try:
        print(json.dumps(bench(args.records, args.reps, mode, tmp)), flush=True)
    finally:
        for f in os.listdir(tmp):
            os.unlink(os.path.join(tmp, f))
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
