"""The drop-in shim (examples/c2d_shim.f) linked into the REFERENCE's own
Fortran host: its main program (src/compton2d.f), reader, setup, xec
(src/xec2d.f:41-193), imcgen2d, graphics, write_record and MPI plumbing,
with the five per-step entry points imcfield2d, imcvol2d, imcsurf2d,
imcredist and update replaced by the shim's (the reference's own
definitions weakened at link time, oracle/ref/build_shim.sh).

This container only (the reference sources and its MPI build stay here): the
reference reads a prepared input.dat (the C3 deck), sets up, enters its
time loop, and the first worker's imcfield2d -> c2d_init fails loudly with
C2D_E_HIP (no GPU here) and aborts the MPI job instead of hanging or
falling back."""
import os
import resource
import subprocess
from pathlib import Path

import pytest

import refcase
from compton2d_amd import synth

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "oracle" / "_ref" / "shim" / "compton2d_gpu"
MPIEXEC = Path("/opt/conda/bin/mpiexec")
REPLACED = ("imcfield2d_", "imcvol2d_", "imcsurf2d_", "imcredist_", "update_")


def _reference_available() -> bool:
    return (refcase.REFERENCE / "src" / "xec2d.f").exists() and MPIEXEC.exists()


@pytest.fixture(scope="module")
def shim_exe():
    if not _reference_available():
        pytest.skip("reference sources / MPI not in this container")
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: this test checks the failure path")
    subprocess.run(["bash", str(ROOT / "oracle" / "ref" / "build_shim.sh")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    assert EXE.exists()
    return EXE


def test_shim_replaces_the_five_entry_points(shim_exe):
    out = subprocess.run(["nm", str(shim_exe)], capture_output=True, text=True, check=True).stdout
    defs = {}
    for line in out.splitlines():
        p = line.split()
        if len(p) == 3:
            defs.setdefault(p[2], []).append(p[1])
    for sym in REPLACED:
        assert defs.get(sym) == ["T"], (sym, defs.get(sym))   # the shim's strong definition
    # the reference's own routines around them are linked unchanged
    for sym in ("xec_", "imcgen2d_", "cens_add_up_", "e_add_up_", "fp_end_bcast_", "file_sp_",
                "write_record_", "reader_", "setup_"):
        assert defs.get(sym) == ["T"], (sym, defs.get(sym))
    weak = ROOT / "oracle" / "_ref" / "shim" / "imcfield2d.weak.o"
    wout = subprocess.run(["nm", str(weak)], capture_output=True, text=True, check=True).stdout
    assert any(l.split()[-2:] == ["W", "imcfield2d_"] for l in wout.splitlines() if l.strip())


def test_reference_host_with_shim_fails_loudly_without_gpu(shim_exe, tmp_path):
    case = tmp_path / "c3"
    refcase.write_input_deck(case, synth.c3_refcase(nst=20000))

    def big_stack():   # the reference needs `ulimit -s unlimited`
        resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))
    env = dict(os.environ)
    # every rank writes its own stdout/stderr file: what a rank wrote just
    # before MPI_Abort the launcher forwards only when it wins a race against
    # its own teardown (lost on a busy or one-CPU host), and this test is about
    # what the shim writes, not about the launcher's forwarding
    r = subprocess.run([str(MPIEXEC), "-n", "2", "/bin/sh", "-c",
                        'exec "$0" > rank_$PMI_RANK.log 2>&1', str(shim_exe)], cwd=case,
                       capture_output=True, text=True, timeout=300, preexec_fn=big_stack, env=env)
    text = r.stdout + r.stderr + "".join(f.read_text() for f in sorted(case.glob("rank_*.log")))
    # the reference ran its own reader + setup and the time loop up to the
    # first transport call (its master log and the worker's rank line)
    assert (case / "log.txt").exists() and "Number of Processors" in (case / "log.txt").read_text()
    assert "c2d_shim: c2d_init failed: -2" in text, text[-2000:]
    assert "MPI_Abort" in text or r.returncode != 0


# ---- the shim's success path, end to end (this container: no GPU needed) ----
# oracle/ref/build_shim.sh also links the same reference host + shim against
# oracle/c2d_standin.c (the C-ABI symbols the shim calls, over the C oracle in
# its reference mode) and builds the unmodified reference.  Both run under
# mpiexec on the same deck (master + worker(s), T_const = 0: FP on).
STANDIN = ROOT / "oracle" / "_ref" / "shim" / "compton2d_standin"
REFEXE = ROOT / "oracle" / "_ref" / "shim" / "compton2d_ref"
SHIM_DECK = dict(T_const=0, tstop=2.0e5, nst=1500)
# files whose every byte the reference writes from state the shim delivers
# (the spectra and light curves since hazard H12 is reproduced by the stand-in)
SAME_FILES = ("p001_evb.dat", "output/nfield.dat", "output/temp_b.dat", "output/eic.dat",
              "output/seb.dat", "esp.dat", "output/spb.dat", "output/phb.dat", "output/lcb_01.dat")
PSPT = ROOT / "oracle" / "_ref" / "pspt"
# pspt's dialogue for this small run: no bulk boost, every direction, the
# run's whole time range, 100 log channels (postprocessing/pspt.c:105-205)
SED_DECK = "p001_evb.dat\n1\n1e16\nsed_shim.dat\n30\n0\n2.5e5\n-1\n1\n1\n1e-7\n1e10\n100\n0\nn\n"


# the census mirror's test hooks: write_record's mark lowered to 0 s of
# etotal (the mirror starts at once and stays on), and every mirror written
# by the reference's own write_cens as write_record would
MIRROR_HOOK = {"C2D_SHIM_MIRROR_MARK": "0", "C2D_SHIM_WRITE_CENS": "1"}


def _mpirun(exe, case, nproc, env_extra):
    def big_stack():
        resource.setrlimit(resource.RLIMIT_STACK, (resource.RLIM_INFINITY, resource.RLIM_INFINITY))
    env = dict(os.environ, **env_extra)
    r = subprocess.run([str(MPIEXEC), "-n", str(nproc), str(exe)], cwd=case, capture_output=True,
                       text=True, timeout=600, preexec_fn=big_stack, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    (case / "run.log").write_text(r.stdout + r.stderr)
    return r


@pytest.fixture(scope="module")
def shim_runs(tmp_path_factory):
    """The reference (1 worker), the shim over the stand-in in fib mode (1
    worker) with and without hazard H12 reproduced, and the shim over the
    stand-in in lineage mode with 1 and 2 workers, run concurrently."""
    if not _reference_available():
        pytest.skip("reference sources / MPI not in this container")
    subprocess.run(["bash", str(ROOT / "oracle" / "ref" / "build_shim.sh")], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    from concurrent.futures import ThreadPoolExecutor
    base = tmp_path_factory.mktemp("shim")
    ev = {"C2D_SHIM_EVENTS": "1"}          # the text events too (the SED is the default)
    runs = {"ref": (REFEXE, 2, {}),
            "shim": (STANDIN, 2, dict(ev, C2D_STANDIN_RSEED=str(refcase.BASE_CASE["rseed"]))),
            "nolag": (STANDIN, 2, dict(ev, C2D_STANDIN_RSEED=str(refcase.BASE_CASE["rseed"]),
                                       C2D_STANDIN_GRID_LAG="0")),
            "lin1": (STANDIN, 2, dict(ev, C2D_STANDIN_RNG="lineage", **MIRROR_HOOK)),
            "lin2": (STANDIN, 3, dict(ev, C2D_STANDIN_RNG="lineage", **MIRROR_HOOK))}
    dirs = {}
    for k in runs:
        dirs[k] = base / k
        refcase.write_input_deck(dirs[k], SHIM_DECK)
        (dirs[k] / "sed.input").write_text(SED_DECK)
        runs[k][2]["C2D_SHIM_SED_DECK"] = str(dirs[k] / "sed.input")
    with ThreadPoolExecutor(len(runs)) as ex:
        futs = {k: ex.submit(_mpirun, exe, dirs[k], n, dict(env, C2D_STANDIN_COMM_DIR=str(dirs[k])))
                for k, (exe, n, env) in runs.items()}
        for f in futs.values():
            f.result()
    return dirs


def _events(d, pattern="p00*_evb.dat"):
    return [line for f in sorted(d.glob(pattern)) for line in f.read_text().splitlines()]


def _spectrum_from_events(d):
    """spb.dat's F(E) (src/graphics2d.f:143-160: fout / (dE (time + dt))) of the
    run's own escape events, binned on the spb.dat energy grid."""
    import numpy as np
    a = np.loadtxt(d / "output" / "spb.dat")
    lo, hi = a[0::2], a[1::2]
    edges = np.append(lo[:, 0], hi[-1, 0])
    ev = np.array([[float(x) for x in l.split()] for l in _events(d)])
    f = np.zeros(len(lo))
    idx = np.searchsorted(edges, ev[:, 1], side="right") - 1
    ok = (idx >= 0) & (idx < len(lo))
    np.add.at(f, idx[ok], ev[ok, 2])
    return lo[:, 1], f / np.diff(edges)


def test_shim_over_standin_reproduces_the_reference_mpi_run(shim_runs):
    """The reference's OWN host (main program, reader, setup, xec, imcgen2d,
    graphics, FP_end_bcast ...) with the shim's five entry points over the
    C-ABI (here the stand-in: the oracle in its reference mode, bit for bit
    the reference's worker routines), against the unmodified reference on
    the same deck, both 1 master + 1 worker under MPI: the worker's escape
    event file and the files the master writes from the shim-delivered
    tallies and electron state are identical byte for byte -- census
    transport, volume sources, the tally download into COMMON, the census
    mirror, and update's c2d_fp_step through FP_end_bcast (temp_b.dat).
    Two reference quirks are reproduced by the stand-in, not the shim: the
    workers' stale t_bound (H4) and their stale dt (H11: dt reaches the
    workers only in z_surf_bcast, src/surf_mpi.f:68, so their census and
    volume packets fly with the previous step's dt, 0 at ncycle 0)."""
    ref, shim = shim_runs["ref"], shim_runs["shim"]
    for f in SAME_FILES:
        assert (shim / f).read_bytes() == (ref / f).read_bytes(), f
    assert len(_events(shim)) > 1000


def test_shim_spectrum_is_its_event_spectrum(shim_runs):
    """Hazard H12 isolated.  With the workers' first-step grids supplied
    (C2D_STANDIN_GRID_LAG=0: what the GPU engine does), spb.dat is F(E) of
    the run's escape events (to the file's 6 digits).  The reference's own
    spb.dat, from the byte-identical event file, is not: the packets its
    worker creates in step 0, before its first z_surf_bcast delivers
    nphtotal / hu / nph_lc / Elcmin / Elcmax (src/surf_mpi.f:24-27,76-81),
    carry spectral and light-curve bins 0 (src/imcvol2d_para.f:334-374)
    through the census until they scatter, so their escapes are written to
    the event file but never reach fout / edout (src/imcleak2d.f:172-175,
    206-209, 307-310).  Only energy is removed (every bin <= the event
    spectrum), and the stand-in with the lag on (the "shim" run) reproduces
    the reference's spb.dat byte for byte (SAME_FILES)."""
    import numpy as np
    F, f_ev = _spectrum_from_events(shim_runs["nolag"])
    # the last step's time + dt (graphics2d.f:146), from the spectrum's own normalisation
    live = F > 1e-20
    scale = np.median(f_ev[live] / F[live])
    np.testing.assert_allclose(F[live] * scale, f_ev[live], rtol=5e-5)   # e14.6 text
    Fr, f_evr = _spectrum_from_events(shim_runs["ref"])
    assert np.array_equal(f_evr, f_ev)                       # same events ...
    r = Fr[live] / F[live]
    assert np.all(r <= 1 + 1e-5) and np.median(r) < 0.9      # ... energy missing from spb.dat
    lc0 = np.loadtxt(shim_runs["nolag"] / "output" / "lcb_01.dat")
    lc1 = np.loadtxt(shim_runs["ref"] / "output" / "lcb_01.dat")
    assert np.all(lc1[:, 1:] <= lc0[:, 1:] * (1 + 1e-5)) and np.any(lc1[:, 1:] < 0.9 * lc0[:, 1:])


def test_shim_two_workers_allreduce_equals_one_worker(shim_runs):
    """The shim's N-worker mode: the workers' step tallies summed by
    c2d_allreduce_tallies inside the C-ABI (the stand-in's file-based
    exchange here; RCCL in the product), deposited into COMMON by worker 1
    only.  Lineage streams make the histories independent of the worker
    count, so 2 workers reproduce 1: spb.dat, lcb_01.dat, temp_b.dat,
    eic.dat, esp.dat byte for byte, nfield.dat to summation order, and the
    escape events as a set -- but for the stale t_bound of lower-surface
    escapes (H4), which is per-worker state in the reference."""
    import numpy as np
    a, b = shim_runs["lin1"], shim_runs["lin2"]
    assert len(list(b.glob("p00*_evb.dat"))) == 2
    for f in ("output/spb.dat", "output/lcb_01.dat", "output/temp_b.dat", "output/eic.dat", "esp.dat"):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    na, nb = np.loadtxt(a / "output" / "nfield.dat"), np.loadtxt(b / "output" / "nfield.dat")
    np.testing.assert_allclose(nb, na, rtol=1e-13, atol=0)
    ea, eb = _events(a), _events(b)
    assert sorted(l.split(None, 1)[1] for l in ea) == sorted(l.split(None, 1)[1] for l in eb)
    lower = lambda ev: sorted(l for l in ev if l.split()[4] != "0.0000000E+00")
    assert lower(ea) == lower(eb)


def _sed(path):
    """(header lines, E, F [n_e, n_t], counts of the last time bin) of a pspt file."""
    import numpy as np
    lines = Path(path).read_text().splitlines()
    rows = [l.split() for l in lines[4:]]
    a = np.array([[float(x) for x in r[:-1]] for r in rows])
    return lines[:4], a[:, 0], a[:, 1:], np.array([int(r[-1]) for r in rows])


@pytest.mark.parametrize("run", ["shim", "lin2"])
def test_shim_sed_on_device_equals_pspt_on_its_event_files(shim_runs, run):
    """The shim's default event output: every step's escapes binned with
    pspt's own binning from its deck (c2d_obs_begin_pspt; N workers summed
    inside the C-ABI, c2d_obs_write_pspt) and pspt's file written, instead
    of event text.  Against the reference's pspt (postprocessing/pspt.c,
    built from the reference) run on the same run's event files (written
    here too, C2D_SHIM_EVENTS=1): the same header, energies and last-bin
    counts but for events within text rounding of a bin edge (pspt bins the
    7-digit event text, the engine the doubles), fluxes to that rounding."""
    import numpy as np
    if not PSPT.exists():
        pytest.skip("reference pspt not built (oracle/ref/build_ref.sh)")
    d = shim_runs[run]
    ours = d / "sed_shim.dat"
    assert ours.exists()
    ref_dir = d / "pspt_ref"
    ref_dir.mkdir(exist_ok=True)
    for f in d.glob("p00*_evb.dat"):
        (ref_dir / f.name).write_bytes(f.read_bytes())
    subprocess.run([str(PSPT)], input=SED_DECK, text=True, cwd=ref_dir, check=True, capture_output=True)
    h0, E0, F0, c0 = _sed(ref_dir / "sed_shim.dat")
    h1, E1, F1, c1 = _sed(ours)
    assert h0 == h1
    np.testing.assert_array_equal(E1, E0)
    assert np.sum(np.abs(c1 - c0)) <= 2 and c0.sum() > 0
    live = F0 > 1e-19
    assert live.sum() > 20
    assert np.all((F1 > 1e-19) == live)
    rel = np.abs(F1[live] - F0[live]) / F0[live]
    assert np.median(rel) < 1e-6 and np.mean(rel < 1e-5) > 0.98, (np.max(rel), np.median(rel))


def _census_records(path):
    """(6 f64 text, 6 i32 text) record pairs of a write_cens file (census2d.f:23-25)."""
    lines = Path(path).read_text().splitlines()
    assert len(lines) % 2 == 0
    return [(lines[i], lines[i + 1]) for i in range(0, len(lines), 2)]


def test_shim_census_mirror_reaches_write_cens(shim_runs):
    """the census mirror that write_record reads.  With the mark
    lowered (C2D_SHIM_MIRROR_MARK=0) it starts at ncycle 0 and stays on,
    and the reference's own write_cens (census2d.f:1-33, called as
    write_record.f:433-437 calls it) writes the census of the run's last
    step from COMMON dbufout/ibufout: 2 workers write, between them, the
    same records as 1 worker (lineage streams: the census does not depend
    on the worker count).  With the default mark no mirror runs."""
    a, b = shim_runs["lin1"], shim_runs["lin2"]
    for d, nw in ((a, 1), (b, 2)):
        log = (d / "run.log").read_text()
        import re
        assert len(re.findall(r"census mirror on from ncycle\s+0\b", log)) == nw, log[-2000:]
        assert "records dropped" not in log
    ra = _census_records(a / "p001_census_mirror.dat")
    rb = _census_records(b / "p001_census_mirror.dat") + _census_records(b / "p002_census_mirror.dat")
    assert len(ra) > 100
    assert sorted(ra) == sorted(rb)
    for d6, i6 in ra:
        v = [float(d6[14 * i:14 * i + 14]) for i in range(6)]                               # 6e14.7
        jgpsp, jgplc, jgpmu, jph, kph, seed = (int(i6[5 * i:5 * i + 5]) for i in range(6))   # 6i5
        assert v[4] > 0 and v[5] > 0 and 1 <= jph <= 2 and 1 <= kph <= 2 and 0 <= seed < 100000
    shim_log = (shim_runs["shim"] / "run.log").read_text()
    assert "census mirror on" not in shim_log
    assert not list(shim_runs["shim"].glob("p00*_census_mirror.dat"))
