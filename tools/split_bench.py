#!/usr/bin/env python3
"""Census splitting (c2d_census_split) on one MI355X.

Workload: the census of the golden C3 case (c3_mrk421) after its first step,
replicated to N records with distinct keys (replica k's keys are the
census's xor a SplitMix64 output of k; torch does the xor on the packed
records).  After one warm-up round, `--reps` rounds of

  pack      Engine.census_pack of the whole census into a device buffer, the
            same-traffic yardstick (64 B read and 64 B written a record):
            host time around the synchronous call
  count     Engine.census_split(dry_run=True) at the ceilings below: device
            time of the count kernel and the tile scan
  split     the committed pass at ceilings that split about a quarter of the
            records: the C3 census carries one weight a source, so no ratio
            above 1 of weight_ceiling splits any of it; instead the fullest
            (cell, group) bins that together hold a quarter of the records
            get two thirds of their mean weight as ceiling (m = 2 for a
            record of mean weight) and the others none: device time of
            count, scan and expansion
  multiply  popcontrol.multiply(eng, 2): every record doubled
  roulette  Engine.census_roulette with weight_floor at target = N / 4 on the
            same census (the pass is untouched by the split: the figure is
            the parent commit's)

with the census put back from the packed buffer after every pass that
changed it, and for each leg its share of the 8 TB/s HBM peak priced on the
bytes it must move: 32 B read a record (ex and tg), 32 B more read and 16 B
written a split record (rz and wp read for the copies, ex rewritten), 64 B
written a copy.

    python tools/split_bench.py [--records 10000000] [--reps 3]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
sys.path.insert(0, str(ROOT / "tools"))

from census_file_bench import timed  # noqa: E402

HBM_PEAK = 8.0e12


def distinct_engine(n, mode, capacity):
    """A C3 context whose census is its first step's, repeated up to n records, every replica
    with keys of its own; returns (engine, the packed census in a device buffer)."""
    import torch
    from compton2d_amd import abi, popcontrol as PC
    from compton2d_amd.engine import Engine
    from golden_io import GoldenCase
    gc = GoldenCase("c3_mrk421")
    eng = Engine(gc.grid(comtot_mode=mode, census_capacity=capacity))
    eng.transport_step(gc.step_inputs(0))
    n0 = eng.census_count()
    rec = torch.zeros(n0 * abi.CENSUS_REC_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()      # torch's fill runs on its own stream, the pack on the context's
    eng.census_pack(0, n0, rec.data_ptr())
    eng.census_truncate(0)
    k = 0
    while eng.census_count() < n:
        mix = PC.mix64_int(k + 1) if k else 0
        rep = rec.clone().view(-1, abi.CENSUS_REC_WORDS)
        rep[:, 7] ^= mix - (1 << 64) if mix >> 63 else mix            # the key word, as a signed 64-bit integer
        torch.cuda.synchronize()
        eng.census_append(rep.data_ptr(), min(n0, n - eng.census_count()))
        k += 1
    assert eng.census_count() == n
    buf = torch.empty(n * abi.CENSUS_REC_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    eng.census_pack(0, n, buf.data_ptr())
    return eng, buf


def bench(n, reps, mode, ratios):
    from compton2d_amd import popcontrol as PC
    eng, buf = distinct_engine(n, mode, max(2 * n + (1 << 20), 1 << 21))
    g, ng = PC.groups_by_decade(eng.grid.hu)
    count, energy = eng.census_stats(g, ng)
    assert int(count.sum()) == n

    def restore():
        eng.census_truncate(0)
        eng.census_append(buf.data_ptr(), n)

    tried = {}
    for ratio in ratios:                            # what weight_ceiling's own ceilings would split
        w = PC.weight_ceiling(count, energy, ratio)
        tried[ratio] = eng.census_split(g, ng, w, 8, 0, dry_run=True)["n_split"]
    order = np.argsort(-count, axis=None)
    take = order[:int(np.searchsorted(np.cumsum(count.reshape(-1)[order]), n / 4)) + 1]
    w_max = np.zeros(count.size)
    w_max[take] = energy.reshape(-1)[take] / count.reshape(-1)[take] / 1.5
    w_max = w_max.reshape(count.shape)
    w_min = PC.weight_floor(count, energy, n // 4)
    rows = []
    for rep in range(reps + 1):                     # round 0 warms up
        pack_ms, _ = timed(lambda: eng.census_pack(0, n, buf.data_ptr()))
        dry = eng.census_split(g, ng, w_max, 8, rep, dry_run=True)
        out = eng.census_split(g, ng, w_max, 8, rep)
        assert (out["n_before"], out["n_after"], out["n_split"]) == (n, dry["n_after"], dry["n_split"])
        restore()
        dbl = PC.multiply(eng, 2, rep)
        assert dbl["n_after"] == n + dbl["n_split"]
        restore()
        rl = eng.census_roulette(g, ng, w_min, rep)
        restore()
        if rep:
            rows.append(dict(pack_ms=pack_ms, count_ms=dry["kernel_ms"], split_ms=out["kernel_ms"],
                             n_split=out["n_split"], copies=out["n_after"] - n, multiply_ms=dbl["kernel_ms"],
                             multiply_copies=dbl["n_after"] - n, roulette_ms=rl["kernel_ms"],
                             roulette_after=rl["n_after"]))
    eng.close()
    med = lambda k: float(np.median([r[k] for r in rows]))
    must = lambda split, copies: 32.0 * n + 48.0 * split + 64.0 * copies
    roof = lambda b, ms: b / HBM_PEAK / (ms * 1e-3)
    n_split, copies, mcopies = int(med("n_split")), int(med("copies")), int(med("multiply_copies"))
    return {
        "records": n, "reps": reps, "groups": ng, "bins_with_ceiling": int(len(take)), "weight_ceiling_n_split_by_ratio": {str(k): int(v) for k, v in tried.items()},
        "n_split": n_split, "copies": copies, "multiply_copies": mcopies,
        "count_kernel_ms": med("count_ms"), "count_share_of_hbm_peak": roof(32.0 * n, med("count_ms")),
        "split_kernel_ms": med("split_ms"), "split_must_move_bytes": must(n_split, copies),
        "split_share_of_hbm_peak": roof(must(n_split, copies), med("split_ms")),
        "multiply2_kernel_ms": med("multiply_ms"), "multiply2_must_move_bytes": must(mcopies, mcopies),
        "multiply2_share_of_hbm_peak": roof(must(mcopies, mcopies), med("multiply_ms")),
        "roulette_kernel_ms": med("roulette_ms"), "roulette_n_after": int(med("roulette_after")),
        "pack_call_ms_host": med("pack_ms"), "pack_GBps": 128.0 * n / (med("pack_ms") * 1e-3) / 1e9,
        "count_over_pack": med("count_ms") / med("pack_ms"), "split_over_pack": med("split_ms") / med("pack_ms"),
        "multiply2_over_pack": med("multiply_ms") / med("pack_ms"),
        "split_over_roulette": med("split_ms") / med("roulette_ms"),
        "multiply2_over_roulette": med("multiply_ms") / med("roulette_ms"),
        "all": rows, "hbm_peak_TBps": HBM_PEAK / 1e12,
        "note": "count, split, multiply, roulette: device time between events; pack: host time around the synchronous call"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--exact", action="store_true", help="an exact-comtot context")
    ap.add_argument("--ratios", type=float, nargs="+", default=[1.25, 1.5, 2.0, 3.0, 4.0, 8.0])
    args = ap.parse_args()
    from compton2d_amd import abi
    mode = abi.COMTOT_EXACT if args.exact else abi.COMTOT_TABLE
    print(json.dumps(bench(args.records, args.reps, mode, args.ratios)), flush=True)


if __name__ == "__main__":
    main()
