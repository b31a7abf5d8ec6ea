#!/usr/bin/env python3
"""The exact observer set (c2d_obs_set_exact, integer sums) against the f64
set kernel on one MI355X: the same device-resident events (tools/obs_bench.py
`set`: jittered copies of the reference's, tests/golden/obs.npz) and the same
two sets, {sed_mrk421, lc_mrk421} and all four decks.  Per round both kernels
are timed alternately in one process (HIP-event kernel times of the
library); reported: the medians, the ratio exact / f64, the lds_rows each
plan reached, the bytes per event (56 B read once by either kernel) and
whether the exact counts equal the f64 kernel's.

    python tools/obs_exact_bench.py [--events 20000000] [--reps 7]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

HBM_PEAK_GBS = 8000.0
BYTES_PER_EVENT = 56.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    from obs_bench import device_events
    from compton2d_amd.engine import obs_engine
    from test_gpu_observe import G, _binning

    n = args.events
    dev = device_events(n)           # torch's HIP runtime comes up before the library opens its context
    w_max = float(G["events"][:, 2].max())          # the jitter leaves the weights as they are
    eng = obs_engine(0)
    ptr = dev.data_ptr()
    out = {"events": n, "reps": args.reps, "bytes_per_event": BYTES_PER_EVENT, "w_max": w_max}
    for label, names in (("sed+lc_mrk421", ("sed_mrk421", "lc_mrk421")),
                         ("four_decks", ("sed_mrk421", "sed_wide", "lc_mrk421", "lc_wide"))):
        bins = [_binning(nm)[1] for nm in names]
        ms = {"f64": [], "exact": []}
        rows, counts, rejected = {}, {}, []
        for rep in range(args.reps + 1):                 # round 0 warms both up
            for kind in ("f64", "exact"):
                eng.obs_set_clear()
                if kind == "exact":
                    eng.obs_set_exact(w_max)
                ids = [eng.obs_set_add(b) for b in bins]
                eng.obs_set_accumulate_device(ptr, n)
                t, _ = eng.obs_set_kernel_ms()
                if rep:
                    ms[kind].append(t)
                rows[kind] = [eng.obs_set_shape(i)[3] for i in ids]
                if rep == args.reps:
                    if kind == "exact":
                        rejected = [eng.obs_set_exact_info(i)[1] for i in ids]
                    counts[kind] = [eng.obs_set_result(i)[2] for i in ids]
        f, x = float(np.median(ms["f64"])), float(np.median(ms["exact"]))
        ach = BYTES_PER_EVENT * n / (x * 1e-3) / 1e9
        out[label] = {"decks": list(names), "f64_ms": f, "f64_ms_min_max": [min(ms["f64"]), max(ms["f64"])],
                      "exact_ms": x, "exact_ms_min_max": [min(ms["exact"]), max(ms["exact"])],
                      "ratio_exact_over_f64": x / f, "lds_rows_f64": rows["f64"], "lds_rows_exact": rows["exact"],
                      "n_t": [b.n_t for b in bins], "n_rejected": rejected,
                      "roofline_exact": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                         "frac": ach / HBM_PEAK_GBS},
                      "counts_equal_f64": all(bool(np.array_equal(a, b))
                                              for a, b in zip(counts["f64"], counts["exact"]))}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
