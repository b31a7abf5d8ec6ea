#!/usr/bin/env python3
"""The census comb (c2d_census_comb_hist, popcontrol.comb_floor) on one MI355X.

Workload: the census of the golden C3 case (c3_mrk421) after its first step,
replicated to N records as in roulette_bench.py, but every replica with keys
of its own (the key word of the packed records XORed with a constant a
replica): equal keys would give equal critical values, and the search's
buckets would never shrink.  After one warm-up round, `--reps` rounds of

  stats      Engine.census_stats with groups_by_decade, the kernel the comb's
             pass shares its traffic with (the ex and tg columns, 32 B a
             record): device time of the kernel
  hist       one c2d_census_comb_hist pass at prefix_bits 0, 11 and 22 under
             the prefix of the bucket that holds the sought rank: device time
             (the first pass's digit is sign and exponent: the LDS atomics
             of a wave meet on a few addresses, the later ones' do not)
  comb       popcontrol.comb_floor at target = N / 4, all passes, downloads
             and numpy's partition: host time around the call, and its device
             time (info: passes, collected values)
  comb+rl    comb_floor and Engine.census_roulette with its floors: host time
  floor+rl   popcontrol.weight_floor and Engine.census_roulette, the policy
             the comb replaces, at the same target: host time; n_after of both
  refill     the census put back from a device copy (not reported)

Medians over the rounds.  Roofline: 8.0 TB/s on the 32 B a record a pass must
read.

    python tools/comb_bench.py [--records 10000000] [--reps 3]
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
KEY_WORD = 7                                   # of a packed record's 8 words (capi.cpp rec_pack)
GOLDEN = 0x9E3779B97F4A7C15


def replicated_distinct(n, mode):
    """A C3 context whose census is its first step's, repeated up to n records, replica k's keys
    XORed with k * GOLDEN."""
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
    keys0 = rec.view(n0, abi.CENSUS_REC_WORDS)[:, KEY_WORD].clone()
    eng.census_truncate(0)
    k = 0
    while eng.census_count() < n:
        x = (k * GOLDEN) & 0xFFFFFFFFFFFFFFFF
        rec.view(n0, abi.CENSUS_REC_WORDS)[:, KEY_WORD] = keys0 ^ (x - (1 << 64) if x >> 63 else x)
        torch.cuda.synchronize()
        eng.census_append(rec.data_ptr(), min(n0, n - eng.census_count()))
        k += 1
    assert eng.census_count() == n
    return eng, n0


def sought_bucket(hist, k):
    """(digit, rank within it, size) of the bucket that holds the k-th largest value."""
    above = np.cumsum(hist[::-1])
    i = int(np.searchsorted(above, k, side="left"))
    d = len(hist) - 1 - i
    return d, k - int(above[i] - hist[d]), int(hist[d])


def bench(n, reps, mode):
    import torch
    from compton2d_amd import abi, popcontrol as PC
    eng, n0 = replicated_distinct(n, mode)
    buf = torch.empty(n * abi.CENSUS_REC_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    eng.census_pack(0, n, buf.data_ptr())
    g, ng = PC.groups_by_decade(eng.grid.hu)
    target = n // 4
    rows = []

    def refill():
        eng.census_truncate(0)
        eng.census_append(buf.data_ptr(), n)

    def hist_ms(prefix, pb):
        return eng.census_comb_hist(g, ng, norm, rep, prefix, pb)

    for rep in range(reps + 1):                     # round 0 warms up
        count, energy = eng.census_stats(g, ng)
        row = dict(stats_ms=eng.last_census_stats_ms())
        norm = PC.comb_norm(count, energy)
        # the passes of the search, one by one
        h0, o0 = hist_ms(0, 0)
        k = target - o0["n_fixed"] + 1
        d0, k1, b0 = sought_bucket(h0, k)
        h1, o1 = hist_ms(d0, 11)
        d1, k2, b1 = sought_bucket(h1, k1)
        h2, o2 = hist_ms((d0 << 11) | d1, 22)
        row.update(hist0_ms=o0["kernel_ms"], hist11_ms=o1["kernel_ms"], hist22_ms=o2["kernel_ms"],
                   bucket0=b0, bucket11=b1, bucket22=sought_bucket(h2, k2)[2], n_fixed=o0["n_fixed"],
                   distinct_digits0=int((h0 > 0).sum()))
        # the whole policy
        ms, (w, info) = timed(lambda: PC.comb_floor(eng, (g, ng), count, energy, target, rep))
        row.update(comb_host_ms=ms, comb_device_ms=info["comb_ms"], comb_passes=info["passes"],
                   comb_collected=info["collected"])
        ms, out = timed(lambda: eng.census_roulette(g, ng, PC.comb_floor(eng, (g, ng), count, energy, target, rep)[0],
                                                    rep))
        row.update(comb_rl_host_ms=ms, comb_n_after=out["n_after"], comb_rl_kernel_ms=out["kernel_ms"])
        refill()
        ms, out = timed(lambda: eng.census_roulette(g, ng, PC.weight_floor(count, energy, target), rep))
        row.update(floor_rl_host_ms=ms, floor_n_after=out["n_after"], floor_rl_kernel_ms=out["kernel_ms"])
        refill()
        if rep:
            rows.append(row)
    eng.close()
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    roof = lambda ms: 32.0 * n / HBM_PEAK / (ms * 1e-3)
    return {"records": n, "reps": reps, "replica_records": n0, "target": target, "groups": ng, **med,
            "hist0_over_stats": med["hist0_ms"] / med["stats_ms"],
            "hist22_over_stats": med["hist22_ms"] / med["stats_ms"],
            "stats_share_of_hbm_peak": roof(med["stats_ms"]), "hist0_share_of_hbm_peak": roof(med["hist0_ms"]),
            "hist22_share_of_hbm_peak": roof(med["hist22_ms"]), "hbm_peak_TBps": HBM_PEAK / 1e12, "all": rows,
            "note": "kernel times: device time between events; *_host_ms: host time around the synchronous calls"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--exact", action="store_true", help="an exact-comtot context")
    args = ap.parse_args()
    from compton2d_amd import abi
    mode = abi.COMTOT_EXACT if args.exact else abi.COMTOT_TABLE
    print(json.dumps(bench(args.records, args.reps, mode)), flush=True)


if __name__ == "__main__":
    main()
