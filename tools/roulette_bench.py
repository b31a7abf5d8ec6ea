#!/usr/bin/env python3
"""Census population control (c2d_census_stats, c2d_census_roulette) on one MI355X.

Kernels (default).  Workload: the census of the golden C3 case (c3_mrk421)
after its first step, replicated by c2d_census_pack / c2d_census_append to N
records (census_file_bench.replicated_engine; repeated records share their
keys and so their fates, which costs the kernels nothing).  After one warm-up
round, `--reps` rounds of

  stats     Engine.census_stats with groups_by_decade: device time of the
            kernel (c2d_last_census_stats_ms)
  roulette  Engine.census_roulette with weight_floor at target = N / 4:
            device time of the whole pass (kernel_ms: decide-and-pack,
            unpack and cursor kernels of every slice)
  pack      Engine.census_pack of the whole census into a device buffer, the
            same-traffic yardstick (64 B read and 64 B written a record):
            host time around the synchronous call
  refill    the census put back from that buffer (not reported)

and for each kernel its share of the HBM roofline priced on the bytes it
must move: stats reads the ex and tg columns, 32 B a record; the roulette
must read those 32 B of every record, and read the other 32 B and write 64 B
of every record that stays (an in-place pass could not do with less); what
the pass as built moves (a survivor goes through the scratch: 4 x 64 B) is
printed beside it.  Roofline: 8.0 TB/s (the HBM3E peak; a float4 copy reaches
6.3 TB/s).

--c3: the C3 workload at reduced size (--sources volume packets a step,
--steps steps, FP on), 16 seeds without a CensusControl, with one at
target = 1/4 of the uncontrolled run's last census, and with the same one
made exact (the comb's floors, popcontrol.comb_floor): mean step time of the
last half of the steps, the census there, and the relative scatter over the
seeds (standard deviation / mean, per bin) of the SED summed over those steps
(the fout tally), as its energy-weighted mean over the bins.

    python tools/roulette_bench.py [--records 10000000] [--reps 3] [--c3]
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
sys.path.insert(0, str(ROOT / "tools"))

from census_file_bench import replicated_engine, timed  # noqa: E402

HBM_PEAK = 8.0e12


def kernels(n, reps, mode):
    import torch
    from compton2d_amd import abi, popcontrol as PC
    eng = replicated_engine(n, mode)
    buf = torch.empty(n * abi.CENSUS_REC_WORDS, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    g, ng = PC.groups_by_decade(eng.grid.hu)
    rows = []
    for rep in range(reps + 1):                     # round 0 warms up
        pack_ms, _ = timed(lambda: eng.census_pack(0, n, buf.data_ptr()))
        count, energy = eng.census_stats(g, ng)
        stats_ms = eng.last_census_stats_ms()
        assert int(count.sum()) == n
        w = PC.weight_floor(count, energy, n // 4)
        out = eng.census_roulette(g, ng, w, rep)
        assert out["n_before"] == n
        eng.census_truncate(0)
        eng.census_append(buf.data_ptr(), n)        # the census as it was
        if rep:
            rows.append(dict(pack_ms=pack_ms, stats_ms=stats_ms, roulette_ms=out["kernel_ms"], n_after=out["n_after"],
                             n_tested=out["n_tested"]))
    eng.close()
    med = lambda k: float(np.median([r[k] for r in rows]))
    n_after = int(med("n_after"))
    must_stats, must_rl = 32.0 * n, 32.0 * n + 96.0 * n_after
    does_rl = 32.0 * n + (32.0 + 64.0 + 64.0 + 64.0) * n_after
    roof = lambda b, ms: b / HBM_PEAK / (ms * 1e-3)
    return {
        "records": n, "reps": reps, "groups": ng, "bins": int(count.size), "n_after": n_after,
        "n_tested": int(med("n_tested")), "floors_set": int((w > 0).sum()),
        "stats_kernel_ms": med("stats_ms"), "stats_GBps": must_stats / (med("stats_ms") * 1e-3) / 1e9,
        "stats_share_of_hbm_peak": roof(must_stats, med("stats_ms")),
        "roulette_kernel_ms": med("roulette_ms"), "roulette_must_move_bytes": must_rl,
        "roulette_moves_bytes": does_rl, "roulette_share_of_hbm_peak": roof(must_rl, med("roulette_ms")),
        "roulette_GBps_moved": does_rl / (med("roulette_ms") * 1e-3) / 1e9,
        "pack_call_ms_host": med("pack_ms"), "pack_GBps": 128.0 * n / (med("pack_ms") * 1e-3) / 1e9,
        "roulette_over_pack": med("roulette_ms") / med("pack_ms"), "stats_over_pack": med("stats_ms") / med("pack_ms"),
        "all": rows, "hbm_peak_TBps": HBM_PEAK / 1e12,
        "note": "stats and roulette: device time between events; pack: host time around the synchronous call"}


def c3_run(sources, steps, seed, ctl):
    from compton2d_amd import abi, synth
    from compton2d_amd.coupled import CoupledRun
    from compton2d_amd.engine import Engine
    wl = synth.c3_workload(sources=sources, seed=seed, census_capacity=max(1 << 20, 40 * sources))
    L = abi.tally_layout(wl.grid.nz, wl.grid.nr, 1)["fout"]
    import dataclasses
    with Engine(dataclasses.replace(wl.grid, census_inplace=1)) as eng:
        run = CoupledRun(eng, wl, census_control=ctl)
        sed, ms, cens, rl = np.zeros(L[1]), [], [], []
        for n in range(steps):
            t0 = time.perf_counter()
            row = run.step()
            dt = (time.perf_counter() - t0) * 1e3
            if n >= steps // 2:
                sed += eng.tally_range(L[0], L[1])
                ms.append(dt)
                cens.append(eng.census_count())
                rl.append(row.get("roulette_ms", 0.0))
    return sed, float(np.mean(ms)), float(np.mean(cens)), float(np.mean(rl))


def scatter(seds):
    s = np.array(seds)
    mean, std = s.mean(0), s.std(0, ddof=1)
    ok = mean > 0
    rel = std[ok] / mean[ok]
    return {"bins": int(ok.sum()), "energy_weighted": float((rel * mean[ok]).sum() / mean[ok].sum()),
            "median": float(np.median(rel))}


def c3(sources, steps, seeds):
    from compton2d_amd import popcontrol as PC
    free = [c3_run(sources, steps, 1000 + s, None) for s in range(seeds)]
    target = int(np.mean([f[2] for f in free]) / 4)
    ctl = PC.CensusControl(target=target)
    held = [c3_run(sources, steps, 1000 + s, ctl) for s in range(seeds)]
    combed = [c3_run(sources, steps, 1000 + s, PC.CensusControl(target=target, exact=True)) for s in range(seeds)]
    leg = lambda rs: {"step_ms": float(np.mean([r[1] for r in rs])), "census": float(np.mean([r[2] for r in rs])),
                      "roulette_kernel_ms": float(np.mean([r[3] for r in rs])), "sed_rel_scatter": scatter([r[0] for r in rs])}
    return {"sources": sources, "steps": steps, "seeds": seeds, "target": target, "slack": ctl.slack,
            "uncontrolled": leg(free), "controlled": leg(held), "controlled_exact": leg(combed),
            "note": "means over the last half of the steps; step_ms is host time around CoupledRun.step"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--exact", action="store_true", help="an exact-comtot context")
    ap.add_argument("--c3", action="store_true", help="the C3 legs instead of the kernels")
    ap.add_argument("--sources", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--seeds", type=int, default=16)
    args = ap.parse_args()
    from compton2d_amd import abi
    if args.c3:
        print(json.dumps(c3(args.sources, args.steps, args.seeds)), flush=True)
        return
    mode = abi.COMTOT_EXACT if args.exact else abi.COMTOT_TABLE
    print(json.dumps(kernels(args.records, args.reps, mode)), flush=True)


if __name__ == "__main__":
    main()
