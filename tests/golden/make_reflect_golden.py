"""Fixtures of the Compton-reflection decks from the reference itself
(oracle/_ref/c2d_refdrv through tests/refcase.py) — TEST INFRASTRUCTURE.

    python tests/golden/make_reflect_golden.py [--seeds N] [--jobs 8] [deck ...]
    python tests/golden/make_reflect_golden.py tables     (reflect_tables.npz)

Three decks on ssc_tau's 2x2 grid (n_e = 4e6, nst = 2000, 3 steps,
rand_switch = 1), each run with reflect_case.REF_SEEDS distinct rseeds:

    reflect_spec   cr_sent = 4           specular lower boundary
    reflect_both   cr_sent = 3, tbbl > 0 matrix branch below, the disk outside
    reflect_disk   cr_sent = 2           the disk alone

tests/golden/reflect_<deck>.npz keeps the deck, the seeds, the first seed's
step inputs (they do not depend on rseed: checked here), and per run and step
the summed tallies and the histograms of the disk-reflected events
(zpre == 0 and wmu > 0) -- not the event lists.  It also keeps the compared
spectral bins (groups of adjacent hu bins, each populated in every run:
reflect_case.select_groups) with the share of the summed fout energy they carry, and the verdict of a split-half comparison of the runs
against each other under tests/test_gpu_reflect.py's thresholds; the
generator fails if the share is below 90 % or the split-half does not pass.
"""
from __future__ import annotations

import argparse
import json
import shutil
import sys
import tempfile
from multiprocessing import Pool
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parents[1]))

import refcase as RC  # noqa: E402
import reflect_case as RF  # noqa: E402

NSTEPS = 3


def one_run(args):
    deck, seed = args
    case = dict(RF.DECKS[deck], rseed=int(seed))
    d = Path(tempfile.mkdtemp(prefix="c2d_refl_"))
    try:
        RC.write_input_deck(d, case)
        RC.run_reference(d, NSTEPS)
        cfg = RC.read_config(d)
        ins = [RC.read_step_in(d, n, cfg) for n in range(NSTEPS)]
        outs = [RC.read_step_out(d, n, cfg) for n in range(NSTEPS)]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    row = {}
    for n, o in enumerate(outs):
        ev = o["events"]
        if not np.isfinite(ev).all():
            raise RuntimeError("%s seed %d step %d: non-finite event" % (deck, seed, n))
        # the reference's fout runs on from step to step (tests/test_oracle_golden.py): this step's part
        fout = o["fout"] - (outs[n - 1]["fout"] if n > 0 else 0.0)
        row[n] = RF.step_summary(fout, o["edout"], {k: o[k] for k in ("erlki", "erlko", "erlku", "erlkl")},
                                 o["Ed_in"], float(o["edep"].sum()), float(o["ecens"].sum()), ev,
                                 int(o["census_d"].shape[0]), cfg["hu"])
    return cfg, ins, outs[0], row


def make(deck: str, seeds, jobs: int) -> Path:
    with Pool(jobs) as pool:
        res = pool.map(one_run, [(deck, s) for s in seeds], chunksize=1)
    cfg, ins, out0, _ = res[0]
    # the step inputs are the deck's, whatever the seed
    for c2, i2, _, _ in res[1:]:
        for n in range(NSTEPS):
            for k in RF.IN_KEYS:
                np.testing.assert_array_equal(np.asarray(ins[n][k]), np.asarray(i2[n][k]), err_msg="%s in%d_%s" % (deck, n, k))
    arrays = {"seeds": np.asarray(seeds, np.int64)}
    for k in ("z", "r", "E_field", "gnt", "hu", "Elcmin", "Elcmax", "mu"):
        arrays["cfg_" + k] = np.asarray(cfg[k])
    arrays["E_ph"] = np.asarray(ins[0]["E_ph"])
    for n in range(NSTEPS):
        for k in RF.IN_KEYS:
            arrays["in%d_%s" % (n, k)] = np.asarray(ins[n][k])
    for name in RF.SUMMARY_KEYS:
        arrays["run_" + name] = np.stack([np.stack([np.asarray(r[3][n][name]) for n in range(NSTEPS)]) for r in res])
    meta = {k: (int(v) if isinstance(v, (int, np.integer)) else float(v)) for k, v in cfg.items()
            if np.isscalar(v)}
    meta["nsteps"] = NSTEPS
    meta["deck"] = {k: v for k, v in RF.DECKS[deck].items()}
    for n in range(NSTEPS):
        meta["step%d" % n] = {k: (int(ins[n][k]) if k == "ncycle" else float(ins[n][k])) for k in ("ncycle", "time", "dt")}
    # compared bins and the split-half self-check
    sel, share = RF.select_groups(RF.run_energy(arrays["run_fout"]))
    half = len(seeds) // 2
    verdict = RF.compare(arrays, slice(0, half), arrays, slice(half, 2 * half), sel)
    meta["groups"] = sel
    meta["fout_share"] = share
    meta["split_half"] = verdict
    nev = arrays["run_n_events"].sum(axis=1)
    nrf = arrays["run_refl_xnu"].sum(axis=(1, 2))
    meta["events_per_run"] = float(nev.mean())
    meta["disk_reflected_per_run"] = float(nrf.mean())
    print(deck, "bins", len(sel), "fout share %.4f" % share, "events/run %.1f" % nev.mean(),
          "disk-reflected/run %.1f" % nrf.mean(), "split-half", json.dumps(verdict))
    arrays["meta_json"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    out = HERE / ("reflect_%s.npz" % deck.split("_", 1)[1])
    np.savez_compressed(out, **arrays)
    ok = share >= 0.9 and verdict["ok"]
    print(out, "%.1f KB" % (out.stat().st_size / 1024), "OK" if ok else "FAILS ITS OWN CHECKS")
    return out if ok else None


TABLES_DRIVER = """      program c2d_refl_dump
      implicit none
      include 'general.pa'
      include 'commonblock.f'
      integer i, j
      call Pref_calc()
      call Wref_calc()
      open(11, file='tab.bin', form='unformatted', access='stream')
      write(11) (E_ref(i), i=1,n_ref)
      write(11) ((P_ref(j,i), j=1,n_ref), i=1,n_ref)
      write(11) ((W_abs(j,i), j=1,n_ref), i=1,n_ref)
      close(11)
      end
"""


def sample_tables(E, P, W) -> dict:
    """What reflect_tables.npz keeps of the three tables ([n_in][n_out]):
    E_ref whole, every TABLE_STRIDE-th column and row of P_ref and W_abs, the
    diagonals, and each column's plain sum over n_out."""
    s = RF.TABLE_STRIDE
    d = np.arange(len(E))
    return dict(E_ref=E, P_cols=P[::s], W_cols=W[::s], P_rows=P[:, ::s], W_rows=W[:, ::s], P_diag=P[d, d],
                W_diag=W[d, d], P_sum=P.sum(axis=1), W_sum=W.sum(axis=1))


def make_tables() -> Path:
    """E_ref, P_ref, W_abs of the reference's own Pref_calc / Wref_calc
    (src/ref_matrix.f, the object oracle/ref/build_ref.sh compiled), dumped by a
    ten-line driver and sampled into tests/golden/reflect_tables.npz."""
    import os
    import subprocess
    src = Path(os.environ.get("C2D_REFERENCE_SRC", str(RC.REFERENCE / "src")))
    fc = os.environ.get("FC", "/opt/rocm/lib/llvm/bin/flang")
    d = Path(tempfile.mkdtemp(prefix="c2d_refl_tab_"))
    try:
        (d / "dump.f").write_text(TABLES_DRIVER)
        subprocess.run([fc, "-O2", "-I" + os.environ.get("MPI_INC", "/opt/conda/include"), "-I" + str(src), "dump.f",
                        str(RC.ROOT / "oracle" / "_ref" / "obj" / "ref_matrix.o"), "-o", "dump"], cwd=d, check=True)
        subprocess.run([str(d / "dump")], cwd=d, check=True)
        t = np.fromfile(d / "tab.bin")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    n = 500
    assert t.size == n + 2 * n * n
    out = HERE / "reflect_tables.npz"
    np.savez_compressed(out, **sample_tables(t[:n], t[n:n + n * n].reshape(n, n), t[n + n * n:].reshape(n, n)))
    print(out, "%.1f KB" % (out.stat().st_size / 1024))
    return out


if __name__ == "__main__":
    if sys.argv[1:] == ["tables"]:
        make_tables()
        sys.exit(0)
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=None, help="rseeds per deck (default: reflect_case.REF_SEEDS)")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("decks", nargs="*", default=list(RF.DECKS))
    a = ap.parse_args()
    bad = [d for d in a.decks
           if make(d, [RF.ref_seed(k) for k in range(a.seeds or RF.REF_SEEDS[d])], a.jobs) is None]
    sys.exit(1 if bad else 0)
