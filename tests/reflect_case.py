"""The Compton-reflection decks and how their runs are summarised and
compared — TEST INFRASTRUCTURE shared by tests/golden/make_reflect_golden.py
(the reference's runs) and tests/test_gpu_reflect.py (the engine's).

Both sides are sets of independent runs of one deck (distinct seeds), three
steps each; a run is reduced to summed tallies and to histograms of its
disk-reflected events.  `compare` holds two such sets against each other with
the thresholds of tests/test_gpu_compton.py (compton_case.compare_runs over
the compared bins (select_groups): chi^2 p-value > 1e-3, rms z <= 1.2, no bin beyond 4.5
sigma, each light-curve band within 4 sigma), the same thresholds on the
histograms, and the mean event and census counts within 4 sigma of the two
sides' run-to-run scatter.
"""
from __future__ import annotations

import numpy as np

import compton_case as CC
import spectrum_case as S

# tbbl of the matrix deck's lower rings [keV]: > 0 turns both rings into
# matrix reflectors (and blackbody surface sources of that temperature)
TBBL = 1.0e-3
_BASE = dict(nz=2, nr=2, n_e=4.0e6, nst=2000, rand_switch=1)
DECKS = {
    "reflect_spec": dict(_BASE, cr_sent=4),
    "reflect_both": dict(_BASE, cr_sent=3, tbbl=TBBL),
    "reflect_disk": dict(_BASE, cr_sent=2, spec_switch=0),
}
# reference runs (distinct rseeds) per deck.  The spectral bins of one run are
# correlated (a collision hands its split2/split3 copies to neighbouring bins),
# so rms z over the bins scatters more than independent bins would: the
# reference's own halves give 0.88-1.19.  The specular deck's first 64 rseeds
# sat in that upper tail against any engine sample (rms z 1.32; 1.07 against
# rseeds 128..255 alone), so it keeps 256 reference runs
REF_SEEDS = {"reflect_spec": 256, "reflect_both": 64, "reflect_disk": 64}
IN_KEYS = ("kappa_tot", "eps_tot", "eps_th", "f_nt", "Pnt", "n_e", "Eloss_th", "Eloss_tot",
           "zsurf", "ewsv", "nsv", "nsurfi", "nsurfo", "ewsurfi", "ewsurfo", "nsurfu", "nsurfl",
           "ewsurfu", "ewsurfl", "tbbi", "tbbo", "tbbu", "tbbl")
SUMMARY_KEYS = ("fout", "edout", "erlki", "erlko", "erlku", "erlkl", "Ed_in", "edep", "ecens",
                "n_events", "n_census", "refl_xnu", "refl_wmu")
WMU_BINS = 8
TABLE_STRIDE = 7        # reflect_tables.npz: every 7th column and row of P_ref / W_abs

P_MIN, RMS_Z_MAX, MAX_Z, BAND_Z, COUNT_Z = 1.0e-3, 1.2, 4.5, 4.0, 4.0


def ref_seed(k: int) -> int:
    """rseed of the k-th reference run."""
    return 10007 + 7919 * k


def lin_seed(k: int) -> int:
    """Lineage seed of the k-th engine run."""
    return CC.LINEAGE_SEED + 104729 * (k + 1)


def step_summary(fout, edout, erlk: dict, Ed_in, edep: float, ecens: float, events, n_census: int, hu) -> dict:
    """One step of one run: the tallies the comparison reads and the
    histograms of the disk-reflected events (zpre == 0 and wmu > 0): xnu on
    the hu grid, wmu in WMU_BINS equal bins of (0, 1)."""
    ev = np.asarray(events, float).reshape(-1, 7)
    disk = ev[(ev[:, 4] == 0.0) & (ev[:, 5] > 0.0)]
    hx = np.histogram(disk[:, 1], bins=np.asarray(hu))[0].astype(np.float64)
    hw = np.histogram(disk[:, 5], bins=np.linspace(0.0, 1.0, WMU_BINS + 1))[0].astype(np.float64)
    d = dict(fout=np.asarray(fout, float), edout=np.asarray(edout, float), Ed_in=np.asarray(Ed_in, float),
             edep=np.float64(edep), ecens=np.float64(ecens), n_events=np.float64(len(ev)),
             n_census=np.float64(n_census), refl_xnu=hx, refl_wmu=hw)
    for k in ("erlki", "erlko", "erlku", "erlkl"):
        d[k] = np.asarray(erlk[k], float)
    return d


def run_F(run_fout) -> np.ndarray:
    """Per-run F(E) [runs, bins] summed over the steps."""
    f = np.asarray(run_fout, float).sum(axis=1)          # [runs, nmu, NPHOMAX]
    return np.stack([S.f_of_e(x) for x in f])


def run_energy(run_fout) -> np.ndarray:
    """Per-run escaping energy per hu bin [runs, bins], summed over the steps and mu."""
    return run_F(run_fout) * np.diff(S.synth.photon_grid())


def select_groups(E_ref):
    """The compared spectral bins: groups of adjacent hu bins, each populated
    in every reference run.  From compare_runs' lowest bin (1e-3 keV) upwards a
    group takes hu bins until every run has energy in it; what is left over at
    the top joins the last group.  At nst = 2000 single hu bins populated in
    every run carry 35-52 % of the escaping energy, which sits in the rarely
    populated top bins; the groups carry all of it above 1e-3 keV.  Returns
    ([[first, last], ...], the share of the reference's summed fout energy in
    the groups)."""
    E_ref = np.asarray(E_ref, float)
    groups, cur = [], []
    for b in CC.compton_bins():
        cur.append(int(b))
        if (E_ref[:, cur].sum(axis=1) > 0).all():
            groups.append([cur[0], cur[-1]])
            cur = []
    if cur:
        groups[-1][1] = cur[-1]
    inside = sum(E_ref[:, a:b + 1].sum() for a, b in groups)
    return groups, float(inside / E_ref.sum())


def regroup(E, groups) -> np.ndarray:
    """[runs, bins] with each group's sum at its first bin and 0 elsewhere
    (compare_runs takes the bins with a positive reference mean)."""
    E = np.asarray(E, float)
    out = np.zeros_like(E)
    for a, b in groups:
        out[:, a] = E[:, a:b + 1].sum(axis=1)
    return out


def _z_stats(XA, XB):
    """Per-bin z of two sets of runs [runs, bins] over the bins populated in
    every run of B, with run-to-run variances."""
    from scipy import stats
    XA, XB = np.asarray(XA, float), np.asarray(XB, float)
    live = np.nonzero((XB > 0).all(axis=0))[0]
    s = np.sqrt(XA.var(axis=0, ddof=1) / len(XA) + XB.var(axis=0, ddof=1) / len(XB))
    live = live[s[live] > 0]
    if len(live) == 0:
        return dict(bins=0, p_value=1.0, rms_z=0.0, max_abs_z=0.0)
    z = (XA.mean(axis=0)[live] - XB.mean(axis=0)[live]) / s[live]
    chi2 = float(np.sum(z ** 2))
    return dict(bins=int(len(live)), p_value=float(stats.chi2.sf(chi2, len(live))),
                rms_z=float(np.sqrt(np.mean(z ** 2))), max_abs_z=float(np.abs(z).max()))


def _mean_z(a, b) -> float:
    a, b = np.asarray(a, float), np.asarray(b, float)
    s = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    d = a.mean() - b.mean()
    return float(d / s) if s > 0 else (0.0 if d == 0 else float("inf"))


def compare(A, ia, B, ib, groups) -> dict:
    """Runs ia of A (the side under test) against runs ib of B (the
    reference): dicts of 'run_*' arrays [runs, steps, ...].  `groups`: the
    compared spectral bins (select_groups of the reference)."""
    FA, FB = regroup(run_energy(A["run_fout"][ia]), groups), regroup(run_energy(B["run_fout"][ib]), groups)
    EA = np.asarray(A["run_edout"][ia], float).sum(axis=1).reshape(FA.shape[0], -1)[:, :5]
    EB = np.asarray(B["run_edout"][ib], float).sum(axis=1).reshape(FB.shape[0], -1)[:, :5]
    sp = CC.compare_runs(FA, EA, FB, EB)
    out = {"spectrum": {k: sp[k] for k in ("bins", "p_value", "rms_z", "max_abs_z", "band_z")}}
    out["refl_xnu"] = _z_stats(A["run_refl_xnu"][ia].sum(axis=1), B["run_refl_xnu"][ib].sum(axis=1))
    out["refl_wmu"] = _z_stats(A["run_refl_wmu"][ia].sum(axis=1), B["run_refl_wmu"][ib].sum(axis=1))
    out["events_z"] = _mean_z(A["run_n_events"][ia].sum(axis=1), B["run_n_events"][ib].sum(axis=1))
    # the census a run ends with
    out["census_z"] = _mean_z(A["run_n_census"][ia][:, -1], B["run_n_census"][ib][:, -1])
    ok = abs(out["events_z"]) <= COUNT_Z and abs(out["census_z"]) <= COUNT_Z
    for k in ("spectrum", "refl_xnu", "refl_wmu"):
        d = out[k]
        ok = ok and d["p_value"] > P_MIN and d["rms_z"] <= RMS_Z_MAX and d["max_abs_z"] <= MAX_Z
    ok = ok and all(abs(z) <= BAND_Z for z in out["spectrum"]["band_z"])
    out["ok"] = bool(ok)
    return out


class ReflectFixture:
    """tests/golden/reflect_<name>.npz: the deck, the reference's per-run
    summaries, and the step inputs the engine is driven with."""

    def __init__(self, name: str):
        import json
        from pathlib import Path
        z = np.load(Path(__file__).resolve().parent / "golden" / ("reflect_%s.npz" % name), allow_pickle=False)
        self.a = {k: z[k] for k in z.files}
        self.meta = json.loads(bytes(self.a.pop("meta_json")).decode())
        self.nsteps = self.meta["nsteps"]
        self.groups = [list(g) for g in self.meta["groups"]]

    def grid(self, **over):
        from compton2d_amd import abi
        m, a = self.meta, self.a
        g = abi.GridConfig(
            nz=m["nz"], nr=m["nr"], rmin=m["rmin"], zmin=m["zmin"], z=a["cfg_z"], r=a["cfg_r"],
            E_ph=a["E_ph"], E_field=a["cfg_E_field"], gnt=a["cfg_gnt"], hu=a["cfg_hu"],
            Elcmin=a["cfg_Elcmin"], Elcmax=a["cfg_Elcmax"], mu=a["cfg_mu"], split1=m["split1"],
            split2=m["split2"], split3=m["split3"], spl3_trg=m["spl3_trg"],
            spec_switch=m["spec_switch"], cr_sent=m["cr_sent"], pair_switch=m["pair_switch"],
            census_capacity=1 << 17, event_capacity=1 << 18, queue_capacity=1 << 16)
        for k, v in over.items():
            setattr(g, k, v)
        return g

    def step_inputs(self, n: int):
        from compton2d_amd import abi
        st = self.meta["step%d" % n]
        return abi.StepInputs(ncycle=st["ncycle"], time=st["time"], dt=st["dt"], spectra=[],
                              **{k: self.a["in%d_%s" % (n, k)] for k in IN_KEYS})


def engine_run(fx: ReflectFixture, eng) -> list:
    """The fixture's steps through an Engine: per step the step_summary plus
    the reflection results and the counters."""
    from compton2d_amd import abi
    rows = []
    for n in range(fx.nsteps):
        eng.transport_step(fx.step_inputs(n))
        t = eng.tallies()
        ev = eng.events()
        row = step_summary(t["fout"], t["edout"], t, t["Ed_in"], float(np.sum(t["edep"])), float(np.sum(t["ecens"])),
                           ev, eng.census_count(), fx.a["cfg_hu"])
        row["Ed_ref"], row["counts"] = eng.reflect_result()
        row["counters"] = np.asarray(t["counters"])
        row["events"] = ev
        rows.append(row)
    return rows


def stack_runs(runs: list) -> dict:
    """'run_*' arrays [runs, steps, ...] of engine_run results."""
    return {"run_" + k: np.stack([np.stack([np.asarray(r[n][k]) for n in range(len(r))]) for r in runs])
            for k in SUMMARY_KEYS}
