"""The coupled Monte-Carlo step of a T_const = 0 run on one GPU context.

Mirrors the reference's per-step sequence (src/xec2d.f:41-110 master,
:141-193 worker) for the hot path:

    imcgen2d   tables + budgets       Engine.volume_em (c2d_volume_em) +
                                      surface.volume_budget (src/imcgen2d.f:209-456);
                                      for a deck with external-Compton rings
                                      (CoupledWorkload.boundary) the window's ring
                                      budgets and seed tables, surface.step_surfaces
                                      + surface.apply_bias (src/imcgen2d.f:111-183,
                                      :436-437, :476-528)
    imcfield2d / imcvol2d / imcsurf2d Engine.transport_step (c2d_set_step + c2d_run_step)
    xec_add / cens_add_up             `allreduce` hook (RCCL all-reduce of the fused tallies)
    update                            Engine.fp_step (c2d_fp_step), n_field/ecens read
                                      from the device tallies (src/update2d.f:7-327)
    (no counterpart: the reference    optional census population control after the
     stops at ucens records)          update (popcontrol.CensusControl): census
                                      statistics, the default weight floors and the
                                      weight-window roulette on the device

With `device_resident` (the default) the 400-bin emission/absorption tables
and the 200-bin electron spectra never leave the GPU: c2d_volume_em keeps its
tables for c2d_set_step (C2D_DEV_EMISSION) and c2d_fp_step updates the
context's electron state in place (C2D_DEV_ELECTRONS).  Only zone scalars
(270 of each at C3) and the tally buffer's ecens cross the host per step.
"""
from __future__ import annotations

import time as _time
from typing import Callable, Optional

import numpy as np

from . import abi, popcontrol, surface
from .engine import Engine
from .synth import CoupledWorkload


class CoupledRun:
    """Advance a CoupledWorkload one MC step at a time on `eng`."""

    def __init__(self, eng: Engine, wl: CoupledWorkload, device_resident: bool = True,
                 allreduce: Optional[Callable[[], None]] = None, fp_mode: int = abi.FP_AUTO,
                 after_transport: Optional[Callable[[], None]] = None,
                 census_control: Optional[popcontrol.CensusControl] = None):
        """fp_mode: the FP update's arithmetic (Engine.fp_set_mode); the
        default abi.FP_AUTO picks exact or fast per update, and each step's
        row logs what ran (`fp_mode`).  after_transport: called as soon as a
        step's transport has returned, before the tally exchange and the FP
        update (e.g. the on-device SED binning of the step's escapes, which
        then runs on its own stream beside them).  census_control: bound the
        census with the weight-window roulette (popcontrol.CensusControl):
        after a step's transport, tally exchange and FP update, when the
        census (summed over ranks through its stats_allreduce) exceeds
        target * (1 + slack), the floors of popcontrol.weight_floor are
        applied with salt = ncycle, and the step's row gains census_before,
        census_after and roulette_ms; with CensusControl(exact=True) the
        floors are popcontrol.comb_floor's, which leave exactly `target`
        records, and the row also gains comb_ms and comb_passes; with
        CensusControl(ceiling_ratio=...) records far heavier than their
        (cell, group)'s mean are split afterwards, the census permitting
        (popcontrol.apply_control), and the row also gains split_copies,
        split_ms and split_skipped.  None (the default) changes nothing."""
        self.eng, self.wl = eng, wl
        self.census_control = census_control
        self._groups = None
        if census_control is not None:
            self._groups = census_control.groups or popcontrol.groups_by_decade(wl.grid.hu)
        self.after_transport = after_transport
        self.device_resident = device_resident
        self.allreduce = allreduce
        self.state = {k: np.array(v, copy=True) for k, v in wl.state0.items()}
        nz, nr = wl.grid.nz, wl.grid.nr
        self.ecens_prev = np.zeros((nz, nr))
        self.n = 0
        self.last = {}
        self.fp_on = int(wl.deck.get("T_const", 0)) == 0
        eng.fp_set_config(wl.fp_const)
        eng.fp_set_mode(fp_mode)
        self.fp_mode = fp_mode
        L = abi.tally_layout(nz, nr, int(np.asarray(wl.grid.mu).size))
        self._ecens = L["ecens"]
        self._cnt = L["counters"][0]

    def _electrons_on_device(self) -> bool:
        return self.device_resident and self.n > 0

    def step(self) -> dict:
        """One MC step; returns per-phase wall times (s) and counters, and of
        the boundary sources `window` (0-based; ntime once every window has
        ended; None without a boundary), `ec_on` (the t0 gate),
        `surface_packets` and `fbias` (the 10 nst cap's factor, 1 if unused)."""
        eng, wl, st = self.eng, self.wl, self.state
        ncycle, t = wl.clock(self.n)
        dt = wl.dt
        t0 = _time.perf_counter()
        # imcgen2d (src/imcgen2d.f:86-99): ec_old = last step's reduced ecens
        ec_old = self.ecens_prev if ncycle > 0 else np.zeros_like(self.ecens_prev)
        dev_el = self._electrons_on_device()
        vin = dict(wl.fixed, tea=st["tea"], n_e=st["n_e"], f_nt=None if dev_el else st["f_nt"])
        vem = eng.volume_em(dt, vin, tables_to_host=not self.device_resident)
        nsv, ewsv = surface.volume_budget(wl.nst, vem["Eloss_tot"])
        self._last_vem = vem
        t1 = _time.perf_counter()
        nz, nr = wl.grid.nz, wl.grid.nr
        surf, window, ec_on = self._surfaces(ncycle, t)
        tab = (None, None, None) if self.device_resident else (vem["kappa_tot"], vem["eps_tot"],
                                                               vem["eps_th"])
        si = abi.StepInputs(
            ncycle=ncycle, time=t, dt=dt, kappa_tot=tab[0], eps_tot=tab[1], eps_th=tab[2],
            f_nt=None if dev_el else st["f_nt"], Pnt=None if dev_el else st["Pnt"],
            n_e=st["n_e"], Eloss_th=vem["Eloss_th"], Eloss_tot=vem["Eloss_tot"],
            zsurf=wl.fixed["zsurf"], ewsv=ewsv, nsv=nsv, **surf)
        fbias = surface.apply_bias(wl.nst, si) if wl.boundary is not None else 1.0
        eng.transport_step(si)
        if self.after_transport is not None:
            self.after_transport()
        t2 = _time.perf_counter()
        if self.allreduce is not None:
            self.allreduce()
        t3 = _time.perf_counter()
        # what the step reads back: this step's ecens (the next step's ec_old)
        # and the counters, not the whole tally buffer
        o = self._ecens
        ecens_now = eng.tally_range(o[0], o[1])
        c = eng.tally_range(self._cnt, abi.NCOUNTERS)
        fp_ms = 0.0
        fp_mode = None
        if self.fp_on and ncycle > 0:
            inputs = dict(wl.fixed, tea=st["tea"], n_e=st["n_e"], B_field=vem["B_field"],
                          Eloss_sy=vem["Eloss_sy"], ec_old=ec_old, ecens=None, n_field=None)
            state_in = dict(st)
            if self.device_resident:
                state_in.pop("f_nt", None)
                state_in.pop("Pnt", None)
            new = eng.fp_step(ncycle, t, dt, inputs, state_in)
            for k in ("tea", "n_e", "gmin", "gmax", "amxwl", "p_nth", "Te_new"):
                st[k] = new[k]
            if not self.device_resident:
                st["f_nt"], st["Pnt"] = new["f_nt"], new["Pnt"]
            self.last_fp = new
            fp_ms = eng.last_fp_ms()
            fp_mode = abi.FP_MODE_NAMES.get(eng.last_fp_mode())
        t4 = _time.perf_counter()
        self.ecens_prev = ecens_now.reshape(nz, nr)
        g0_ms, all_ms, _ = eng.last_kernel_ms()
        g0_paths, all_paths = eng.last_path_steps()
        self.last = dict(
            ncycle=ncycle, tables_s=t1 - t0, transport_s=t2 - t1, allreduce_s=t3 - t2, fp_s=t4 - t3,
            step_s=t4 - t0, vem_kernel_ms=eng.last_vem_ms(), transport_gen0_ms=g0_ms,
            transport_all_ms=all_ms, fp_kernel_ms=fp_ms, fp_mode=fp_mode,
            packet_steps=float(c[abi.CNT_STEPS]),
            gen0_steps=float(eng.last_gen0_steps()), gen0_paths=float(g0_paths),
            all_paths=float(all_paths), sources=float(c[abi.CNT_SOURCES]),
            census=float(c[abi.CNT_CENSUS]), escapes=float(c[abi.CNT_ESCAPES]),
            aborted=float(c[abi.CNT_ABORTED]), mean_Te=float(np.mean(st.get("Te_new", st["tea"]))),
            volume_packets=int(np.sum(si.nsv)), window=window, ec_on=ec_on,
            surface_packets=int(np.sum(si.nsurfi) + np.sum(si.nsurfo) + np.sum(si.nsurfu)
                                + np.sum(si.nsurfl)), fbias=fbias)
        if self.census_control is not None:
            self.last.update(popcontrol.apply_control(eng, self.census_control, self._groups, ncycle))
        self.n += 1
        return self.last

    def next_step_inputs(self) -> abi.StepInputs:
        """Host-array StepInputs of the NEXT step (tables computed on the GPU
        from the current electron state), e.g. to replay it on the CPU."""
        wl, st = self.wl, self.state
        ncycle, t = wl.clock(self.n)
        f, p = self.electrons()
        vin = dict(wl.fixed, tea=st["tea"], n_e=st["n_e"], f_nt=f)
        vem = self.eng.volume_em(wl.dt, vin, tables_to_host=True)
        nsv, ewsv = surface.volume_budget(wl.nst, vem["Eloss_tot"])
        surf, _, _ = self._surfaces(ncycle, t)
        si = abi.StepInputs(
            ncycle=ncycle, time=t, dt=wl.dt, kappa_tot=vem["kappa_tot"], eps_tot=vem["eps_tot"],
            eps_th=vem["eps_th"], f_nt=f, Pnt=p, n_e=st["n_e"], Eloss_th=vem["Eloss_th"],
            Eloss_tot=vem["Eloss_tot"], zsurf=wl.fixed["zsurf"], ewsv=ewsv, nsv=nsv, **surf)
        if wl.boundary is not None:
            surface.apply_bias(wl.nst, si)
        return si

    def _surfaces(self, ncycle: int, t: float):
        """(surface fields of the step's StepInputs, window, ec_on): the
        deck's boundary rings in the window of this step
        (surface.step_surfaces), or no surface sources at all for a workload
        without a boundary."""
        wl = self.wl
        b = wl.boundary
        if b is not None:
            return surface.step_surfaces(b, b.r, b.rmin, wl.nst, ncycle, t, wl.dt)
        nz, nr = wl.grid.nz, wl.grid.nr
        zz, zr = np.zeros(nz), np.zeros(nr)
        izz, izr = np.zeros(nz, np.int32), np.zeros(nr, np.int32)
        return dict(nsurfi=izz, nsurfo=izz, ewsurfi=zz, ewsurfo=zz, nsurfu=izr, nsurfl=izr,
                    ewsurfu=zr, ewsurfl=zr, tbbi=zz, tbbo=zz, tbbu=zr, tbbl=zr), None, False

    @staticmethod
    def sample_step(si: abi.StepInputs, frac: float) -> abi.StepInputs:
        """The same step with every zone's volume packet count scaled by frac."""
        import dataclasses
        nsv = np.floor(np.asarray(si.nsv, np.float64) * frac).astype(np.int32)
        return dataclasses.replace(si, nsv=nsv)

    def fp_call_host(self):
        """(ncycle, time, dt, inputs, state) of an FP update from the current
        state and the last step's tallies, as host arrays (CPU replay)."""
        wl, st = self.wl, self.state
        nz, nr = wl.grid.nz, wl.grid.nr
        t = self.eng.tallies()
        f, p = self.electrons()
        ncycle, tm = wl.clock(max(self.n - 1, 1))
        inputs = dict(wl.fixed, tea=st["tea"], n_e=st["n_e"], Eloss_sy=np.zeros((nz, nr)),
                      ec_old=self.ecens_prev, ecens=np.asarray(t["ecens"]).reshape(nz, nr),
                      n_field=np.asarray(t["n_field"]).reshape(nz, nr, abi.NPHFIELD))
        if hasattr(self, "last_fp") and "B_field" in getattr(self, "_last_vem", {}):
            inputs["B_field"] = self._last_vem["B_field"]
            inputs["Eloss_sy"] = self._last_vem["Eloss_sy"]
        state = dict(st, f_nt=f, Pnt=p)
        return ncycle, tm, wl.dt, inputs, state

    def electrons(self):
        """Current f_nt, Pnt [nz, nr, NUM_NT] (downloaded in device-resident mode)."""
        if self._electrons_on_device():
            return self.eng.electron_state()
        return self.state["f_nt"], self.state["Pnt"]

    # -- checkpoints ---------------------------------------------------------
    def _observer_members(self) -> int:
        """Members of the engine's observer set."""
        from .engine import C2DError
        n = 0
        while n < abi.OBS_SET_MAX:
            try:
                self.eng.obs_set_shape(n)
            except C2DError:
                break
            n += 1
        return n

    def save(self, path, observer_set: bool = False) -> int:
        """Save the run between two steps (Engine.checkpoint_write): the
        context's census, kappa_prev, device electrons and FP flags, and as
        the user blob an .npz (no pickling) of the step number, ecens_prev,
        the zone scalars of `state` (f_nt / Pnt too while they live on the
        host) and the workload's nst, dt and seed.  Returns the census
        records written.  observer_set: the engine's exact observer set
        (Engine.obs_set_exact) travels too, every member's state as a further
        member of the blob (obs_state_<id>), for restore(observer_set=True);
        without it the blob is what it always was, and observer accumulations
        are not part of the checkpoint."""
        import io
        import zipfile
        on_dev = self._electrons_on_device()
        blob = {"n": np.int64(self.n), "ecens_prev": self.ecens_prev,
                "wl_nst": np.asarray(self.wl.nst), "wl_dt": np.float64(self.wl.dt),
                "wl_seed": np.uint64(self.wl.grid.seed), "device_resident": np.int64(self.device_resident)}
        for k, v in self.state.items():
            if on_dev and k in ("f_nt", "Pnt"):
                continue
            blob["state_" + k] = np.asarray(v)
        if observer_set:
            m = self._observer_members()
            blob["obs_members"] = np.int64(m)
            for i in range(m):
                blob["obs_state_%d" % i] = self.eng.obs_set_state(i)
        # an .npz with fixed member dates: the same state gives the same bytes
        buf = io.BytesIO()
        with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
            for k, v in blob.items():
                member = io.BytesIO()
                np.lib.format.write_array(member, np.asanyarray(v), allow_pickle=False)
                z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())
        return self.eng.checkpoint_write(path, buf.getvalue())

    @classmethod
    def restore(cls, eng: Engine, wl: CoupledWorkload, path, observer_set: bool = False, **kw) -> "CoupledRun":
        """A run on `eng` (a fresh context of the workload's grid) that
        carries on where save() stopped: step() runs step n.  kw: the
        constructor's arguments; device_resident must be the saved run's.
        observer_set: the states saved by save(observer_set=True) are merged
        into the exact observer set the caller has re-created on `eng` (the
        same members in the same order, the same w_max): the set then holds
        the saved integers, bit for bit.  ValueError if the checkpoint has no
        states, another number of them, or one of another binning or bound."""
        import io
        from .engine import C2DError
        run = cls(eng, wl, **kw)
        states = []
        if observer_set:                               # checked before the engine reads anything
            from . import checkpoint, observer
            with np.load(io.BytesIO(checkpoint.read_user(path)), allow_pickle=False) as z:
                if "obs_members" not in z.files:
                    raise ValueError("checkpoint '%s' was saved without the observer set" % path)
                states = [np.array(z["obs_state_%d" % i], np.uint64) for i in range(int(z["obs_members"]))]
            if len(states) != run._observer_members():
                raise ValueError("checkpoint '%s' holds %d observer states, the engine's set has %d members"
                                 % (path, len(states), run._observer_members()))
            for i, st in enumerate(states):
                try:
                    observer.state_merge(eng.obs_set_state(i), st)
                except C2DError as err:
                    raise ValueError("checkpoint '%s': observer state %d does not fit member %d: %s"
                                     % (path, i, i, err)) from None
        _, user = eng.checkpoint_read(path)
        with np.load(io.BytesIO(user), allow_pickle=False) as z:
            if (not np.array_equal(z["wl_nst"], np.asarray(wl.nst)) or float(z["wl_dt"]) != float(wl.dt)
                    or int(z["wl_seed"]) != int(wl.grid.seed)):
                raise ValueError("checkpoint '%s' was saved by another workload (nst, dt or seed differ)" % path)
            if bool(z["device_resident"]) != bool(run.device_resident):
                raise ValueError("checkpoint '%s' was saved with device_resident=%s" % (path, bool(z["device_resident"])))
            run.n = int(z["n"])
            run.ecens_prev = np.array(z["ecens_prev"], copy=True)
            for k in z.files:
                if k.startswith("state_"):
                    run.state[k[len("state_"):]] = np.array(z[k], copy=True)
        for i, st in enumerate(states):
            eng.obs_set_merge(i, st)
        return run
