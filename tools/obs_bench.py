#!/usr/bin/env python3
"""Observer-frame binning throughput (c2d_obs_accumulate) on one MI355X.

Workload: N escape events already resident in HBM (jittered copies of the
reference's own events, tests/golden/obs.npz), binned with the reference's
decks: `sed_wide` (pspt, 12 x 32 bins, LDS-privatised) and `lc_wide` (plcm,
1024 x 3 x 7 bins, global atomics).  Reports events/s from the HIP-event
kernel time, the HBM roofline (56 algorithmic bytes per event: 7 f64 read
once) and the C oracle (the tools' loop, 1 core) on a bounded sample.

    python tools/obs_bench.py [--events 50000000] [--reps 5] [--cpu-events 2000000]

`set` leg: the observer set (c2d_obs_set_*, one fused pass over the events for
several decks) against the same decks binned one after another by the
single-observer kernel, on the same device events; for {sed_mrk421, lc_mrk421}
and for all four decks of obs.npz.  Per round the two are timed alternately
(HIP-event kernel times of the library); the medians over the rounds, the
bytes per event (56 B read once by the fused pass, 56 B per deck by the
sequential passes) and a counts check against the single-observer kernel.

    python tools/obs_bench.py set [--events 20000000] [--reps 7]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

HBM_PEAK_GBS = 8000.0
BYTES_PER_EVENT = 56.0


def device_events(n):
    import torch
    from test_gpu_observe import _many_events
    chunk = 5_000_000
    dev = torch.empty((n, 7), dtype=torch.float64, device="cuda:0")
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        dev[i:i + m] = torch.from_numpy(_many_events(m, seed=11 + i // chunk))
    torch.cuda.synchronize()
    return dev


def set_leg(argv):
    ap = argparse.ArgumentParser(prog="obs_bench.py set")
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args(argv)
    from compton2d_amd.engine import obs_engine
    from test_gpu_observe import _binning

    n = args.events
    dev = device_events(n)           # torch's HIP runtime comes up before the library opens its context
    eng = obs_engine(0)
    ptr = dev.data_ptr()
    out = {"events": n, "reps": args.reps, "bytes_per_event_fused": BYTES_PER_EVENT}
    for label, names in (("sed+lc_mrk421", ("sed_mrk421", "lc_mrk421")),
                         ("four_decks", ("sed_mrk421", "sed_wide", "lc_mrk421", "lc_wide"))):
        bins = [_binning(nm)[1] for nm in names]
        fused, seq = [], []
        for rep in range(args.reps + 1):                 # round 0 warms both up
            eng.obs_set_clear()
            ids = [eng.obs_set_add(b) for b in bins]
            eng.obs_set_accumulate_device(ptr, n)
            ms, launches = eng.obs_set_kernel_ms()
            per = []
            for b in bins:
                eng.obs_begin(b)
                eng.obs_accumulate_device(ptr, n)
                per.append(eng.obs_result()[3])
            if rep:
                fused.append(ms)
                seq.append(per)
        same = True
        for i, b in zip(ids, bins):                      # the last round's histograms
            eng.obs_begin(b)
            eng.obs_accumulate_device(ptr, n)
            same = same and bool(np.array_equal(eng.obs_result()[2], eng.obs_set_result(i)[2]))
        f = float(np.median(fused))
        per = np.median(np.array(seq), axis=0)
        ach = BYTES_PER_EVENT * n / (f * 1e-3) / 1e9
        out[label] = {"decks": list(names), "fused_ms": f, "fused_ms_min_max": [min(fused), max(fused)],
                      "fused_launches": launches,
                      "lds_rows": [eng.obs_set_shape(i)[3] for i in ids],
                      "sequential_ms": float(per.sum()), "sequential_ms_each": [float(x) for x in per],
                      "sequential_ms_min_max": [float(np.sum(seq, axis=1).min()), float(np.sum(seq, axis=1).max())],
                      "bytes_per_event_sequential": BYTES_PER_EVENT * len(names),
                      "speedup": float(per.sum()) / f,
                      "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                   "frac": ach / HBM_PEAK_GBS},
                      "counts_equal_single_observer": same}
    eng.close()
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "set":
        return set_leg(sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-events", type=int, default=2_000_000)
    args = ap.parse_args()
    import torch
    from compton2d_amd import observer
    from compton2d_amd.engine import obs_engine
    from test_gpu_observe import G, _binning, _many_events
    import oracle_lib as OL

    eng = obs_engine(0)
    n = args.events
    chunk = 5_000_000
    dev = torch.empty((n, 7), dtype=torch.float64, device="cuda:0")
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        dev[i:i + m] = torch.from_numpy(_many_events(m, seed=11 + i // chunk))
    torch.cuda.synchronize()
    out = {"events": n, "bytes_per_event": BYTES_PER_EVENT}
    for name in ("sed_wide", "lc_wide"):
        _, b = _binning(name)
        eng.obs_begin(b)
        eng.obs_accumulate_device(dev.data_ptr(), min(n, 1_000_000))      # warm-up
        eng.obs_begin(b)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            eng.obs_accumulate_device(dev.data_ptr(), n)
        wall = time.perf_counter() - t0
        F, F2, cnt, ms = eng.obs_result()
        per = ms / args.reps
        ach = BYTES_PER_EVENT * n / (per * 1e-3) / 1e9
        out[name] = {"kernel_ms": per, "events_per_s": n / (per * 1e-3),
                     "wall_events_per_s": n * args.reps / wall,
                     "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS,
                                  "unit": "GB/s", "frac": ach / HBM_PEAK_GBS},
                     "binned": float(cnt.sum()) / args.reps,
                     "hist_bins": b.n_t * b.n_mu * b.n_e}
        # CPU: the tools' loop (oracle, glibc cos, 1 core) on a bounded sample
        m = min(args.cpu_events, n)
        sample = dev[:m].cpu().numpy()
        t0 = time.perf_counter()
        ref = OL.obs_bin(b, sample, "ref")
        cpu = time.perf_counter() - t0
        out[name]["cpu_baseline"] = {"value": m / cpu, "unit": "events/s", "cores": 1, "kind": "port",
                                     "sample": "%d events" % m}
        # parity on the sample
        eng.obs_begin(b)
        eng.obs_accumulate_device(dev.data_ptr(), m)
        F, F2, cnt, _ = eng.obs_result()
        out[name]["sample_counts_exact"] = bool(np.array_equal(cnt, OL.obs_bin(b, sample, "det")[2]))
        out[name]["sample_F_maxrel_vs_tools"] = float(np.max(np.abs(F - ref[0]) / np.maximum(np.abs(ref[0]), 1e-300)))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
