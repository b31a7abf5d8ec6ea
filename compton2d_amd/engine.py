"""Host-side mirror of the reference's per-step transport interface.

The reference runs, each Monte-Carlo time step (src/xec2d.f:67-87):

    imcgen2d   -> budgets + tables          (host side here: StepInputs)
    imcfield2d -> census transport          \\
    imcvol2d   -> volume-source transport    > Engine.transport_step()
    imcsurf2d  -> surface-source transport  /   (one C-ABI call, c2d_transport_step)
    imcredist  -> census rebalance          (not needed: census stays on its GPU)
    xec_add / graphics_collect / cens_add_up -> Engine.allreduce_tallies()

`Engine` owns one c2d context (one GPU).  Errors raise `C2DError` carrying
the library's message (the reference `stop`s instead).  The HIP library is
required: there is no CPU fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional

import numpy as np

from . import abi

import os

# C2D_LIBRARY selects an alternative build of the same library (tuning sweeps)
LIB_PATH = Path(os.environ.get("C2D_LIBRARY") or
                Path(__file__).resolve().parent / "libcompton2d.so")
_lib = None


class C2DError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("%s (%d): %s" % (abi.ERRORS.get(code, "C2D_E_?"), code, msg))
        self.code = code


def load_library(path: Optional[Path] = None) -> C.CDLL:
    """Load libcompton2d.so (built by `make -C compton2d_amd/csrc`); raise if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise RuntimeError(
            "compton2d_amd: HIP library %s is missing; build it with "
            "`make -C compton2d_amd/csrc` (hipcc --offload-arch=gfx950)" % p)
    lib = C.CDLL(str(p))
    vp = C.c_void_p
    lib.c2d_version.restype = C.c_char_p
    lib.c2d_init.restype = C.c_int
    lib.c2d_init.argtypes = [C.POINTER(abi.Config), C.POINTER(vp)]
    lib.c2d_finalize.argtypes = [vp]
    lib.c2d_last_error.restype = C.c_char_p
    lib.c2d_last_error.argtypes = [vp]
    for fn in ("c2d_transport_step", "c2d_set_step"):
        getattr(lib, fn).restype = C.c_int
        getattr(lib, fn).argtypes = [vp, C.POINTER(abi.StepIn)]
    lib.c2d_set_clock.restype = C.c_int
    lib.c2d_set_clock.argtypes = [vp, C.c_int32, C.c_double, C.c_double]
    lib.c2d_run_step.restype = C.c_int
    lib.c2d_run_step.argtypes = [vp]
    lib.c2d_set_tally_buffer.restype = C.c_int
    lib.c2d_set_tally_buffer.argtypes = [vp, C.c_void_p]
    lib.c2d_tally_layout_get.restype = C.c_int
    lib.c2d_tally_layout_get.argtypes = [vp, C.POINTER(abi.TallyLayout)]
    lib.c2d_tally_device_ptr.restype = C.c_void_p
    lib.c2d_tally_device_ptr.argtypes = [vp]
    lib.c2d_tally_download.restype = C.c_int
    lib.c2d_tally_download.argtypes = [vp, C.POINTER(C.c_double), C.c_int64]
    lib.c2d_tally_download_range.restype = C.c_int
    lib.c2d_tally_download_range.argtypes = [vp, C.POINTER(C.c_double), C.c_int64, C.c_int64]
    lib.c2d_events.restype = C.c_int
    lib.c2d_events.argtypes = [vp, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int64)]
    lib.c2d_events_write.restype = C.c_int
    lib.c2d_events_write.argtypes = [vp, C.c_char_p, C.c_int32, C.POINTER(C.c_int64)]
    lib.c2d_events_write_from.restype = C.c_int
    lib.c2d_events_write_from.argtypes = [vp, C.c_void_p, C.c_int64, C.c_int32, C.c_char_p, C.c_int32]
    lib.c2d_last_events_write_ms.restype = C.c_int
    lib.c2d_last_events_write_ms.argtypes = [vp] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_int64)] * 2 + [
        C.POINTER(C.c_int32)]
    lib.c2d_events_read.restype = C.c_int
    lib.c2d_events_read.argtypes = [vp, C.c_char_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
    lib.c2d_obs_accumulate_file.restype = C.c_int
    lib.c2d_obs_accumulate_file.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    lib.c2d_obs_set_accumulate_file.restype = C.c_int
    lib.c2d_obs_set_accumulate_file.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    lib.c2d_last_events_read_ms.restype = C.c_int
    lib.c2d_last_events_read_ms.argtypes = [vp] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_int64)] * 3 + [
        C.POINTER(C.c_int32)]
    lib.c2d_selftest_scan.restype = C.c_int
    lib.c2d_selftest_scan.argtypes = [C.c_int, C.c_char_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    lib.c2d_selftest_fmt.restype = C.c_int
    lib.c2d_selftest_fmt.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_char_p]
    lib.c2d_census_write.restype = C.c_int
    lib.c2d_census_write.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    lib.c2d_census_write_from.restype = C.c_int
    lib.c2d_census_write_from.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p]
    lib.c2d_census_read.restype = C.c_int
    lib.c2d_census_read.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    lib.c2d_census_read_records.restype = C.c_int
    lib.c2d_census_read_records.argtypes = [vp, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.POINTER(C.c_int64)]
    lib.c2d_last_census_file_ms.restype = C.c_int
    lib.c2d_last_census_file_ms.argtypes = [vp] + [C.POINTER(C.c_double)] * 4 + [C.POINTER(C.c_int64)] * 2 + [
        C.POINTER(C.c_int32)]
    lib.c2d_checkpoint_write.restype = C.c_int
    lib.c2d_checkpoint_write.argtypes = [vp, C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    lib.c2d_checkpoint_read.restype = C.c_int
    lib.c2d_checkpoint_read.argtypes = [vp, C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.c2d_checkpoint_info.restype = C.c_int
    lib.c2d_checkpoint_info.argtypes = [C.c_char_p, C.POINTER(abi.CkptInfo)]
    lib.c2d_last_checkpoint_ms.restype = C.c_int
    lib.c2d_last_checkpoint_ms.argtypes = [vp] + [C.POINTER(C.c_double)] * 3 + [C.POINTER(C.c_int64),
                                                                                C.POINTER(C.c_int32)]
    lib.c2d_census_count.restype = C.c_int
    lib.c2d_census_count.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.c2d_census_export.restype = C.c_int
    lib.c2d_census_export.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_uint64), C.c_int64, C.POINTER(C.c_int64)]
    lib.c2d_census_export_range.restype = C.c_int
    lib.c2d_census_export_range.argtypes = [vp, C.c_int64, C.c_int64, C.POINTER(C.c_double),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.c_int64,
                                            C.POINTER(C.c_int64)]
    lib.c2d_census_pack.restype = C.c_int
    lib.c2d_census_pack.argtypes = [vp, C.c_int64, C.c_int64, C.c_void_p]
    lib.c2d_census_append.restype = C.c_int
    lib.c2d_census_append.argtypes = [vp, C.c_void_p, C.c_int64]
    lib.c2d_census_truncate.restype = C.c_int
    lib.c2d_census_truncate.argtypes = [vp, C.c_int64]
    lib.c2d_census_stats.restype = C.c_int
    lib.c2d_census_stats.argtypes = [vp, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.c2d_last_census_stats_ms.restype = C.c_int
    lib.c2d_last_census_stats_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.c2d_census_roulette.restype = C.c_int
    lib.c2d_census_roulette.argtypes = [vp, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64,
                                        C.POINTER(abi.RouletteOut)]
    lib.c2d_census_roulette_host.restype = C.c_int
    lib.c2d_census_roulette_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.c2d_census_split.restype = C.c_int
    lib.c2d_census_split.argtypes = [vp, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.c_int32,
                                     C.POINTER(abi.SplitOut)]
    lib.c2d_census_split_host.restype = C.c_int
    lib.c2d_census_split_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p,
                                          C.c_void_p]
    lib.c2d_census_split_keys_host.restype = C.c_int
    lib.c2d_census_split_keys_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p]
    lib.c2d_census_comb_hist.restype = C.c_int
    lib.c2d_census_comb_hist.argtypes = [vp, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32,
                                         C.c_void_p, C.POINTER(abi.CombOut)]
    lib.c2d_census_comb_collect.restype = C.c_int
    lib.c2d_census_comb_collect.argtypes = [vp, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32,
                                            C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    lib.c2d_census_comb_host.restype = C.c_int
    lib.c2d_census_comb_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.c2d_census_import.restype = C.c_int
    lib.c2d_census_import.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_uint64), C.c_int64]
    lib.c2d_fp_tridag.restype = C.c_int
    lib.c2d_fp_tridag.argtypes = [vp, C.POINTER(abi.FpIn), C.POINTER(C.c_double)]
    lib.c2d_selftest_math.restype = C.c_int
    lib.c2d_selftest_math.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.c_int64]
    lib.c2d_selftest_geom.restype = C.c_int
    lib.c2d_selftest_geom.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.c_int64]
    lib.c2d_last_gen0_steps.restype = C.c_int
    lib.c2d_last_gen0_steps.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.c2d_last_path_steps.restype = C.c_int
    lib.c2d_last_path_steps.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.c2d_last_compaction.restype = C.c_int
    lib.c2d_last_compaction.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int64)]
    lib.c2d_last_census_chunks.restype = C.c_int
    lib.c2d_last_census_chunks.argtypes = [vp] + [C.POINTER(C.c_int64)] * 4
    lib.c2d_last_kernel_ms.restype = C.c_int
    lib.c2d_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_int32)]
    lib.c2d_transport_prof.restype = C.c_int
    lib.c2d_transport_prof.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int32]
    lib.c2d_fp_set_config.restype = C.c_int
    lib.c2d_fp_set_config.argtypes = [vp, C.POINTER(abi.FpConfig)]
    lib.c2d_fp_step.restype = C.c_int
    lib.c2d_fp_step.argtypes = [vp, C.POINTER(abi.FpStepIn), C.POINTER(abi.FpStepOut)]
    lib.c2d_fp_set_mode.restype = C.c_int
    lib.c2d_fp_set_mode.argtypes = [vp, C.c_int32]
    lib.c2d_last_fp_mode.restype = C.c_int
    lib.c2d_last_fp_mode.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.c2d_last_fp_ms.restype = C.c_int
    lib.c2d_last_fp_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.c2d_volume_em.restype = C.c_int
    lib.c2d_volume_em.argtypes = [vp, C.POINTER(abi.VemIn), C.POINTER(abi.VemOut)]
    lib.c2d_last_vem_ms.restype = C.c_int
    lib.c2d_last_vem_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.c2d_obs_begin.restype = C.c_int
    lib.c2d_obs_begin.argtypes = [vp, C.POINTER(abi.ObsBins)]
    lib.c2d_obs_accumulate.restype = C.c_int
    lib.c2d_obs_accumulate.argtypes = [vp, C.POINTER(C.c_double), C.c_int64]
    lib.c2d_obs_accumulate_device.restype = C.c_int
    lib.c2d_obs_accumulate_device.argtypes = [vp, C.c_void_p, C.c_int64]
    lib.c2d_obs_result.restype = C.c_int
    lib.c2d_obs_result.argtypes = [vp] + [C.POINTER(C.c_double)] * 4
    lib.c2d_obs_begin_pspt.restype = C.c_int
    lib.c2d_obs_begin_pspt.argtypes = [vp, C.c_char_p]
    lib.c2d_obs_write_pspt.restype = C.c_int
    lib.c2d_obs_write_pspt.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32]
    pi32 = C.POINTER(C.c_int32)
    lib.c2d_obs_set_clear.restype = C.c_int
    lib.c2d_obs_set_clear.argtypes = [vp]
    lib.c2d_obs_set_add.restype = C.c_int
    lib.c2d_obs_set_add.argtypes = [vp, C.POINTER(abi.ObsBins), pi32]
    for fn in ("c2d_obs_set_add_pspt", "c2d_obs_set_add_plcm"):
        getattr(lib, fn).restype = C.c_int
        getattr(lib, fn).argtypes = [vp, C.c_char_p, pi32]
    lib.c2d_obs_set_accumulate.restype = C.c_int
    lib.c2d_obs_set_accumulate.argtypes = [vp, C.POINTER(C.c_double), C.c_int64]
    lib.c2d_obs_set_accumulate_device.restype = C.c_int
    lib.c2d_obs_set_accumulate_device.argtypes = [vp, C.c_void_p, C.c_int64]
    lib.c2d_obs_set_shape.restype = C.c_int
    lib.c2d_obs_set_shape.argtypes = [vp, C.c_int32] + [pi32] * 4
    lib.c2d_obs_set_result.restype = C.c_int
    lib.c2d_obs_set_result.argtypes = [vp, C.c_int32] + [C.POINTER(C.c_double)] * 3
    lib.c2d_obs_set_kernel_ms.restype = C.c_int
    lib.c2d_obs_set_kernel_ms.argtypes = [vp, C.POINTER(C.c_double), pi32]
    lib.c2d_obs_set_write.restype = C.c_int
    lib.c2d_obs_set_write.argtypes = [vp, C.c_int32, C.c_char_p, C.c_int32, C.c_int32]
    pu64 = C.POINTER(C.c_uint64)
    lib.c2d_obs_set_exact.restype = C.c_int
    lib.c2d_obs_set_exact.argtypes = [vp, C.c_double]
    lib.c2d_obs_set_exact_info.restype = C.c_int
    lib.c2d_obs_set_exact_info.argtypes = [vp, C.c_int32, pi32, C.POINTER(C.c_int64)]
    lib.c2d_obs_set_state_words.restype = C.c_int
    lib.c2d_obs_set_state_words.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
    lib.c2d_obs_set_state.restype = C.c_int
    lib.c2d_obs_set_state.argtypes = [vp, C.c_int32, pu64, C.c_int64]
    lib.c2d_obs_set_merge.restype = C.c_int
    lib.c2d_obs_set_merge.argtypes = [vp, C.c_int32, pu64, C.c_int64]
    lib.c2d_obs_exact_host.restype = C.c_int
    lib.c2d_obs_exact_host.argtypes = [C.POINTER(abi.ObsBins), C.c_double, C.POINTER(C.c_double), C.c_int64, pu64,
                                       C.c_int64]
    lib.c2d_obs_state_merge.restype = C.c_int
    lib.c2d_obs_state_merge.argtypes = [pu64, C.c_int64, pu64, C.c_int64]
    lib.c2d_obs_state_result.restype = C.c_int
    lib.c2d_obs_state_result.argtypes = [pu64, C.c_int64] + [C.POINTER(C.c_double)] * 3
    lib.c2d_electron_state.restype = C.c_int
    lib.c2d_electron_state.argtypes = [vp, abi.MArray3, abi.MArray3]
    lib.c2d_comm_unique_id.restype = C.c_int
    lib.c2d_comm_unique_id.argtypes = [C.c_void_p, C.c_int64]
    lib.c2d_comm_init.restype = C.c_int
    lib.c2d_comm_init.argtypes = [vp, C.c_void_p, C.c_int32, C.c_int32]
    lib.c2d_allreduce_tallies.restype = C.c_int
    lib.c2d_allreduce_tallies.argtypes = [vp]
    lib.c2d_reflect_tables_host.restype = C.c_int
    lib.c2d_reflect_tables_host.argtypes = [C.POINTER(C.c_double)] * 3
    lib.c2d_reflect_tables.restype = C.c_int
    lib.c2d_reflect_tables.argtypes = [vp] + [C.POINTER(C.c_double)] * 3
    lib.c2d_reflect_result.restype = C.c_int
    lib.c2d_reflect_result.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]
    lib.c2d_selftest_reflect.restype = C.c_int
    lib.c2d_selftest_reflect.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int64,
                                                         C.POINTER(C.c_double), C.POINTER(C.c_double)]
    pd = C.POINTER(C.c_double)
    lib.c2d_setup_grids.restype = C.c_int
    lib.c2d_setup_grids.argtypes = [pd] * 3
    ic = [pd, C.c_int, pd, C.c_int, pd, C.c_int64, C.c_int64]
    lib.c2d_ic_loss.restype = C.c_int
    lib.c2d_ic_loss.argtypes = [C.c_int] + ic
    lib.c2d_ic_loss_timed.restype = C.c_int
    lib.c2d_ic_loss_timed.argtypes = [C.c_int] + ic + [pd]
    lib.c2d_ic_loss_host.restype = C.c_int
    lib.c2d_ic_loss_host.argtypes = ic + [C.c_int]
    lib.c2d_setup_electrons.restype = C.c_int
    lib.c2d_setup_electrons.argtypes = [C.c_int, C.c_int64] + [pd] * 10
    lib.c2d_setup_electrons_host.restype = C.c_int
    lib.c2d_setup_electrons_host.argtypes = [C.c_int64] + [pd] * 10 + [C.c_int]
    if path is None:
        _lib = lib
    return lib


def checkpoint_info(path) -> dict:
    """The header of the checkpoint `path` (c2d_checkpoint_info): checked
    against its digest, the file's size and the trailer; needs no GPU.
    Raises C2DError (C2D_E_IO) for a file that fails."""
    lib = load_library()
    info = abi.CkptInfo()
    rc = lib.c2d_checkpoint_info(os.fsencode(path), C.byref(info))
    if rc != 0:
        raise C2DError(rc, "checkpoint '%s' cannot be read or is damaged" % path)
    d = {k: getattr(info, k) for k, _ in abi.CkptInfo._fields_ if k != "reserved"}
    d["has_kappa"] = bool(info.sections & abi.CKPT_HAS_KAPPA)
    d["has_electrons"] = bool(info.sections & abi.CKPT_HAS_ELECTRONS)
    return d


class Engine:
    """One GPU's transport context (c2d_ctx)."""

    def __init__(self, grid: abi.GridConfig, lib_path: Optional[Path] = None):
        self.lib = load_library(lib_path)
        self.grid = grid
        self._cfg = grid.to_ctypes()
        ctx = C.c_void_p()
        rc = self.lib.c2d_init(C.byref(self._cfg), C.byref(ctx))
        self.ctx = ctx
        if rc != 0:
            msg = self.lib.c2d_last_error(ctx).decode() if ctx.value else "c2d_init rejected config"
            if ctx.value:
                self.lib.c2d_finalize(ctx)
            self.ctx = None
            raise C2DError(rc, msg)
        L = abi.TallyLayout()
        self._check(self.lib.c2d_tally_layout_get(self.ctx, C.byref(L)))
        self.layout = L
        self.nz, self.nr, self.nmu = grid.nz, grid.nr, int(np.asarray(grid.mu).size)
        self._tally_tensor = None

    # -- lifecycle -------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "ctx", None):
            self.lib.c2d_finalize(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int) -> None:
        if rc != 0:
            raise C2DError(rc, self.lib.c2d_last_error(self.ctx).decode())

    # -- the step ------------------------------------------------------------
    def set_step(self, si: abi.StepInputs) -> None:
        self._si = si.to_ctypes()
        self._check(self.lib.c2d_set_step(self.ctx, C.byref(self._si)))

    def set_clock(self, ncycle: int, time: float, dt: float) -> None:
        self._check(self.lib.c2d_set_clock(self.ctx, int(ncycle), float(time), float(dt)))

    def run_step(self) -> None:
        self._check(self.lib.c2d_run_step(self.ctx))

    def transport_step(self, si: abi.StepInputs) -> None:
        """imcfield2d + imcvol2d + imcsurf2d of one time step."""
        self.set_step(si)
        self.run_step()

    # -- tallies -------------------------------------------------------------
    def use_tally_tensor(self, tensor) -> None:
        """Write tallies into a caller-owned device tensor (float64, >= layout.total)."""
        assert tensor.dtype.itemsize == 8 and tensor.numel() >= self.layout.total
        self._tally_tensor = tensor
        self._check(self.lib.c2d_set_tally_buffer(self.ctx, C.c_void_p(tensor.data_ptr())))

    def tallies_raw(self) -> np.ndarray:
        out = np.zeros(self.layout.total, np.float64)
        self._check(self.lib.c2d_tally_download(
            self.ctx, out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out

    def tally_range(self, offset: int, n: int) -> np.ndarray:
        """Tally words [offset, offset + n) of the fused buffer (c2d_tally_download_range)."""
        out = np.zeros(n, np.float64)
        self._check(self.lib.c2d_tally_download_range(
            self.ctx, out.ctypes.data_as(C.POINTER(C.c_double)), int(offset), int(n)))
        return out

    def tallies(self) -> dict:
        return abi.split_tallies(self.tallies_raw(), self.nz, self.nr, self.nmu)

    # -- Compton reflection (cr_sent != 0) ------------------------------------
    def reflect_tables(self):
        """The context's reflection tables from the device (c2d_reflect_tables):
        E_ref [500], P_ref [n_in, n_out], W_abs [n_in, n_out]; cr_sent 1..3 only."""
        n = abi.N_REF
        E, P, W = np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
        self._check(self.lib.c2d_reflect_tables(self.ctx, E.ctypes.data_as(abi.PD), P.ctypes.data_as(abi.PD),
                                                W.ctypes.data_as(abi.PD)))
        return E, P, W

    def reflect_result(self, world_sum: bool = False):
        """The last step's Ed_ref [nr] and the (specular, matrix, disk) reflection
        counts (c2d_reflect_result); world_sum sums over the communicator first."""
        ed = np.zeros(self.nr)
        cnt = np.zeros(3, np.int64)
        self._check(self.lib.c2d_reflect_result(self.ctx, ed.ctypes.data_as(abi.PD),
                                                cnt.ctypes.data_as(C.POINTER(C.c_int64)), int(bool(world_sum))))
        return ed, cnt

    def last_event_count(self) -> int:
        """Escape events the last transport step wrote (c2d_events with no buffer)."""
        n = C.c_int64()
        self._check(self.lib.c2d_events(self.ctx, None, 0, C.byref(n)))
        return n.value

    def events(self) -> np.ndarray:
        n = C.c_int64()
        self._check(self.lib.c2d_events(self.ctx, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), abi.EVENT_WORDS))
        self._check(self.lib.c2d_events(self.ctx, out.ctypes.data_as(C.POINTER(C.c_double)),
                                        n.value, C.byref(n)))
        return out[:n.value]

    def census_count(self) -> int:
        n = C.c_int64()
        self._check(self.lib.c2d_census_count(self.ctx, C.byref(n)))
        return n.value

    def census(self):
        n = self.census_count()
        d6 = np.zeros((max(n, 1), 6))
        i5 = np.zeros((max(n, 1), 5), np.int32)
        keys = np.zeros(max(n, 1), np.uint64)
        m = C.c_int64()
        self._check(self.lib.c2d_census_export(
            self.ctx, d6.ctypes.data_as(C.POINTER(C.c_double)),
            i5.ctypes.data_as(C.POINTER(C.c_int32)), keys.ctypes.data_as(C.POINTER(C.c_uint64)),
            n, C.byref(m)))
        return d6[:n], i5[:n], keys[:n]

    def census_sample(self, first: int, stride: int, cap: int):
        """Census records first, first+stride, ... (at most cap)."""
        n = C.c_int64()
        self._check(self.lib.c2d_census_export_range(self.ctx, first, stride, None, None, None, 0,
                                                     C.byref(n)))
        m = min(cap, n.value)
        d6 = np.zeros((max(m, 1), 6))
        i5 = np.zeros((max(m, 1), 5), np.int32)
        keys = np.zeros(max(m, 1), np.uint64)
        self._check(self.lib.c2d_census_export_range(
            self.ctx, first, stride, d6.ctypes.data_as(C.POINTER(C.c_double)),
            i5.ctypes.data_as(C.POINTER(C.c_int32)), keys.ctypes.data_as(C.POINTER(C.c_uint64)),
            m, C.byref(n)))
        return d6[:m], i5[:m], keys[:m]

    # -- device-resident census records (C2D_CENSUS_REC_WORDS u64 each) ------
    def census_pack(self, first: int, n: int, d_ptr: int) -> None:
        """Pack records [first, first+n) into device memory at d_ptr."""
        self._check(self.lib.c2d_census_pack(self.ctx, int(first), int(n), C.c_void_p(d_ptr)))

    def census_append(self, d_ptr: int, n: int) -> None:
        """Append n packed records from device memory at d_ptr."""
        self._check(self.lib.c2d_census_append(self.ctx, C.c_void_p(d_ptr), int(n)))

    def census_truncate(self, n: int) -> None:
        self._check(self.lib.c2d_census_truncate(self.ctx, int(n)))

    # -- census population control (compton2d_amd/popcontrol.py) -------------
    @staticmethod
    def _group_table(group_of_sp) -> np.ndarray:
        g = np.ascontiguousarray(group_of_sp, np.int32).reshape(-1)
        if g.size != abi.ROULETTE_NSP:
            raise ValueError("group_of_sp holds %d entries, %d expected" % (g.size, abi.ROULETTE_NSP))
        return g

    def _bin_table(self, table, ngroup: int, name: str, what: str) -> np.ndarray:
        """`table` as contiguous f64 of nz * nr * ngroup entries, or ValueError naming it."""
        t = np.ascontiguousarray(table, np.float64)
        if t.size != self.nz * self.nr * int(ngroup) and 1 <= int(ngroup) <= abi.ROULETTE_GROUPS_MAX:
            raise ValueError("%s holds %d %s, %d expected" % (name, t.size, what, self.nz * self.nr * int(ngroup)))
        return t

    def census_stats(self, group_of_sp, ngroup: int):
        """(count int64, energy f64), each [nz, nr, ngroup]: the census's
        records and their summed ew per cell and spectral group
        (c2d_census_stats); the census is unchanged."""
        g = self._group_table(group_of_sp)
        shape = (self.nz, self.nr, max(int(ngroup), 1))
        count, energy = np.zeros(shape, np.int64), np.zeros(shape, np.float64)
        self._check(self.lib.c2d_census_stats(self.ctx, g.ctypes.data, int(ngroup), count.ctypes.data,
                                              energy.ctypes.data))
        return count, energy

    def last_census_stats_ms(self) -> float:
        """Device time of the last census_stats kernel (c2d_last_census_stats_ms)."""
        ms = C.c_double()
        self._check(self.lib.c2d_last_census_stats_ms(self.ctx, C.byref(ms)))
        return ms.value

    def census_roulette(self, group_of_sp, ngroup: int, w_min, salt: int) -> dict:
        """Weight-window roulette of the census against the floors w_min
        [nz, nr, ngroup] (c2d_census_roulette; the rule: popcontrol.roulette_numpy).
        Returns n_before, n_after, n_tested, e_before, e_after, kernel_ms."""
        g = self._group_table(group_of_sp)
        w = None if w_min is None else self._bin_table(w_min, ngroup, "w_min", "floors")
        out = abi.RouletteOut()
        self._check(self.lib.c2d_census_roulette(self.ctx, g.ctypes.data, int(ngroup),
                                                 w.ctypes.data if w is not None else None,
                                                 int(salt) & 0xFFFFFFFFFFFFFFFF, C.byref(out)))
        return {k: getattr(out, k) for k, _ in abi.RouletteOut._fields_}

    def census_split(self, group_of_sp, ngroup: int, w_max, max_copies: int, salt: int,
                     dry_run: bool = False) -> dict:
        """Split the census records heavier than the ceilings w_max [nz, nr,
        ngroup] into at most max_copies records each (c2d_census_split; the
        rule: popcontrol.split_numpy).  dry_run: only count, the census stays
        as it is.  Returns n_before, n_after, n_split, e_before, e_after,
        kernel_ms."""
        g = self._group_table(group_of_sp)
        w = None if w_max is None else self._bin_table(w_max, ngroup, "w_max", "ceilings")
        out = abi.SplitOut()
        self._check(self.lib.c2d_census_split(self.ctx, g.ctypes.data, int(ngroup),
                                              w.ctypes.data if w is not None else None, int(max_copies),
                                              int(salt) & 0xFFFFFFFFFFFFFFFF, abi.SPLIT_DRY if dry_run else 0,
                                              C.byref(out)))
        return {k: getattr(out, k) for k, _ in abi.SplitOut._fields_}

    def _comb_tables(self, group_of_sp, ngroup: int, norm):
        return self._group_table(group_of_sp), self._bin_table(norm, ngroup, "norm", "entries")

    def census_comb_hist(self, group_of_sp, ngroup: int, norm, salt: int, prefix: int = 0, prefix_bits: int = 0):
        """(hist int64 [2048], out dict): the digit histogram of the pool
        records' normalised critical values under the prefix
        (c2d_census_comb_hist; the rule: popcontrol.comb_critical), and
        n_records, n_fixed, n_pool, n_match, kernel_ms.  The census is unchanged."""
        g, nm = self._comb_tables(group_of_sp, ngroup, norm)
        hist, out = np.zeros(abi.COMB_BINS, np.uint64), abi.CombOut()
        self._check(self.lib.c2d_census_comb_hist(self.ctx, g.ctypes.data, int(ngroup), nm.ctypes.data,
                                                  int(salt) & 0xFFFFFFFFFFFFFFFF, int(prefix), int(prefix_bits),
                                                  hist.ctypes.data, C.byref(out)))
        return hist.astype(np.int64), {k: getattr(out, k) for k, _ in abi.CombOut._fields_}

    def census_comb_collect(self, group_of_sp, ngroup: int, norm, salt: int, prefix: int, prefix_bits: int,
                            cap: int):
        """(values f64 [min(n, cap)], n): the normalised critical values under
        the prefix, in any order, and their full number (c2d_census_comb_collect)."""
        g, nm = self._comb_tables(group_of_sp, ngroup, norm)
        vals, n = np.zeros(max(int(cap), 1)), C.c_int64()
        self._check(self.lib.c2d_census_comb_collect(self.ctx, g.ctypes.data, int(ngroup), nm.ctypes.data,
                                                     int(salt) & 0xFFFFFFFFFFFFFFFF, int(prefix), int(prefix_bits),
                                                     vals.ctypes.data, int(cap), C.byref(n)))
        return vals[:min(n.value, int(cap))], n.value

    def import_census(self, d6, i5, keys) -> None:
        d6 = np.ascontiguousarray(d6, np.float64)
        i5 = np.ascontiguousarray(i5, np.int32)
        keys = np.ascontiguousarray(keys, np.uint64)
        self._check(self.lib.c2d_census_import(
            self.ctx, d6.ctypes.data_as(C.POINTER(C.c_double)),
            i5.ctypes.data_as(C.POINTER(C.c_int32)), keys.ctypes.data_as(C.POINTER(C.c_uint64)),
            len(keys)))

    def save_census(self, path) -> int:
        """Checkpoint the device census as a reference record file
        (write_cens, src/census2d.f:1-36) + `<path>.keys`; returns the count."""
        from . import census_io
        d6, i5, keys = self.census()
        census_io.write_census(path, d6, i5, keys)
        return len(keys)

    def load_census(self, path) -> int:
        """Restart from a census record file (read_cens, src/census2d.f:40-76)."""
        from . import census_io
        d6, i5, keys = census_io.read_census(path)
        self.import_census(d6, i5, keys)
        return len(keys)

    # -- the census record file, written and read by the library -------------
    def write_census_file(self, path) -> int:
        """Write the device census to `path` and `<path>.keys`, formatted on
        the device (c2d_census_write): the bytes save_census writes.  Returns
        the records written; the census is unchanged."""
        n = C.c_int64()
        self._check(self.lib.c2d_census_write(self.ctx, os.fsencode(path), C.byref(n)))
        return n.value

    def write_census_records(self, d6, i5, keys, path) -> None:
        """The same for records [n, 6], [n, 5], [n] of the caller, in the
        layout of census() (c2d_census_write_from); nothing is checked against
        the grid."""
        d6 = np.ascontiguousarray(d6, np.float64).reshape(-1, 6)
        i5 = np.ascontiguousarray(i5, np.int32).reshape(-1, 5)
        keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
        n = len(keys)
        assert len(d6) == n and len(i5) == n
        self._check(self.lib.c2d_census_write_from(
            self.ctx, C.c_void_p(d6.ctypes.data if n else None), C.c_void_p(i5.ctypes.data if n else None),
            C.c_void_p(keys.ctypes.data if n else None), n, os.fsencode(path)))

    def read_census_file(self, path) -> int:
        """Replace the device census by the records of `path`, parsed and
        converted on the device (c2d_census_read): what load_census does.
        Returns the record count.  If the call fails after it has begun
        storing, the census is lost as after a failed in-place step."""
        n = C.c_int64()
        self._check(self.lib.c2d_census_read(self.ctx, os.fsencode(path), C.byref(n)))
        return n.value

    def parse_census_file(self, path):
        """(d6 [n, 6], i5 [n, 5], keys [n]) of the census record file `path`
        (c2d_census_read_records): parsed only, the census is untouched."""
        n = C.c_int64()
        try:
            cap = os.path.getsize(path) // 116 + 1      # a canonical file's records: one pass
        except OSError:
            cap = 1                                     # the library reports what is wrong with the file
        while True:
            d6, i5, keys = np.empty((cap, 6)), np.empty((cap, 5), np.int32), np.empty(cap, np.uint64)
            self._check_records(self.lib.c2d_census_read_records(
                self.ctx, os.fsencode(path), C.c_void_p(d6.ctypes.data), C.c_void_p(i5.ctypes.data),
                C.c_void_p(keys.ctypes.data), cap, C.byref(n)), n)
            if n.value <= cap:
                return d6[:n.value], i5[:n.value], keys[:n.value]
            cap = n.value                                # short lines: more records than 116-byte slots

    def last_census_file(self) -> dict:
        """Timings and counts of the last census file call (c2d_last_census_file_ms)."""
        d = [C.c_double() for _ in range(4)]
        k = [C.c_int64() for _ in range(2)]
        chunks = C.c_int32()
        self._check(self.lib.c2d_last_census_file_ms(self.ctx, *[C.byref(v) for v in d], *[C.byref(v) for v in k],
                                                     C.byref(chunks)))
        return {"io_ms": d[0].value, "wait_ms": d[1].value, "kernel_ms": d[2].value, "convert_ms": d[3].value,
                "device_records": k[0].value, "host_records": k[1].value, "chunks": chunks.value}

    # -- checkpoints: the state a step hands to the next, bit for bit -----------
    def checkpoint_write(self, path, user: bytes = b"") -> int:
        """Write the census (raw packed words), kappa_prev, the device
        electron state, the FP flags and the caller's blob `user` to `path`
        (c2d_checkpoint_write).  Returns the census records written; the
        context is unchanged."""
        user = bytes(user)
        n = C.c_int64()
        buf = C.create_string_buffer(user, len(user)) if user else None
        self._check(self.lib.c2d_checkpoint_write(self.ctx, os.fsencode(path), buf, len(user), C.byref(n)))
        return n.value

    def checkpoint_read(self, path, first: int = 0, count: int = -1, append: bool = False,
                        census_only: bool = False):
        """Restore records [first, first + count) of the checkpoint's census
        (count = -1: to the end) and, unless census_only, its tables and FP
        flags (c2d_checkpoint_read).  append: behind the present census.
        Returns (records stored, the user blob)."""
        flags = (abi.CKPT_APPEND if append else 0) | (abi.CKPT_CENSUS_ONLY if census_only else 0)
        info = abi.CkptInfo()
        ub = 0
        if self.lib.c2d_checkpoint_info(os.fsencode(path), C.byref(info)) == 0:
            ub = info.user_bytes
        buf = C.create_string_buffer(max(ub, 1))
        n, got = C.c_int64(), C.c_int64()
        self._check(self.lib.c2d_checkpoint_read(self.ctx, os.fsencode(path), int(first), int(count), flags, buf, ub,
                                                 C.byref(got), C.byref(n)))
        return n.value, buf.raw[:min(ub, got.value)]

    def last_checkpoint(self) -> dict:
        """Timings and counts of the last checkpoint call (c2d_last_checkpoint_ms)."""
        d = [C.c_double() for _ in range(3)]
        nb, ch = C.c_int64(), C.c_int32()
        self._check(self.lib.c2d_last_checkpoint_ms(self.ctx, *[C.byref(v) for v in d], C.byref(nb), C.byref(ch)))
        return {"io_ms": d[0].value, "wait_ms": d[1].value, "kernel_ms": d[2].value, "bytes": nb.value,
                "chunks": ch.value}

    def last_kernel_ms(self):
        """(generation-0 kernel ms, all launches ms, launches) of the last step (HIP events)."""
        g0, al, nl = C.c_double(), C.c_double(), C.c_int32()
        self._check(self.lib.c2d_last_kernel_ms(self.ctx, C.byref(g0), C.byref(al), C.byref(nl)))
        return g0.value, al.value, nl.value

    def transport_prof(self) -> np.ndarray:
        """Section counters of the last step's transport launches (zeros unless
        the library was built with -DC2D_TR_PROF; tools/tr_prof.py)."""
        out = (C.c_uint64 * abi.TR_PROF_WORDS)()
        self._check(self.lib.c2d_transport_prof(self.ctx, out, abi.TR_PROF_WORDS))
        return np.array(out[:], dtype=np.uint64)

    def last_gen0_steps(self) -> int:
        n = C.c_int64()
        self._check(self.lib.c2d_last_gen0_steps(self.ctx, C.byref(n)))
        return n.value

    def last_path_steps(self) -> tuple[int, int]:
        """(generation-0, all launches) lane path-steps of the last step: a
        probe bundle's shared step counts once for all its copies."""
        g0, al = C.c_int64(), C.c_int64()
        self._check(self.lib.c2d_last_path_steps(self.ctx, C.byref(g0), C.byref(al)))
        return g0.value, al.value

    def last_compaction(self) -> tuple[int, int, int]:
        """(rounds, records moved, physical slots) of the last step's census
        close: the dead-tail compaction (double-buffered) or the packing of
        the partly filled chunks (chunked) (c2d_last_compaction)."""
        r, m, ph = C.c_int32(), C.c_int64(), C.c_int64()
        self._check(self.lib.c2d_last_compaction(self.ctx, C.byref(r), C.byref(m), C.byref(ph)))
        return r.value, m.value, ph.value

    def last_census_chunks(self) -> tuple[int, int, int, int]:
        """Chunked census: (chunks in the census, chunks recycled within the
        last step, census chunks not counted down, chunks held)
        (c2d_last_census_chunks); zeros when double-buffered."""
        v = [C.c_int64() for _ in range(4)]
        self._check(self.lib.c2d_last_census_chunks(self.ctx, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    # -- Fokker-Planck -------------------------------------------------------
    def fp_set_config(self, const: abi.FpConstants) -> None:
        """FP_calc run constants + F_IC (replaces setup_bcast / FP_bcast)."""
        self._fpc = const.to_ctypes()
        self._check(self.lib.c2d_fp_set_config(self.ctx, C.byref(self._fpc)))

    def fp_set_mode(self, mode: int) -> None:
        """abi.FP_EXACT (bit for bit the reference order, default),
        abi.FP_FAST (block-parallel sums, partitioned tridag, tree-summed McDonald
        series: equal within rounding) or abi.FP_AUTO (per update: exact while
        every zone sits on the tea clamp within a few sub-steps, fast
        otherwise); include/compton2d.h c2d_fp_set_mode."""
        self._check(self.lib.c2d_fp_set_mode(self.ctx, int(mode)))

    def last_fp_mode(self) -> int:
        """abi.FP_EXACT or abi.FP_FAST: what the last fp_step ran (-1: none yet)."""
        m = C.c_int32()
        self._check(self.lib.c2d_last_fp_mode(self.ctx, C.byref(m)))
        return m.value

    def fp_step(self, ncycle: int, time: float, dt: float, inputs: dict, state: dict) -> dict:
        """One `update` (src/update2d.f:7-327) on the GPU; returns the new state.

        inputs['n_field'] / inputs['ecens'] set to None read the context's
        (all-reduced) tally buffer on the device instead of host arrays."""
        call = abi.FpCall(ncycle, time, dt, inputs, state)
        self._check(self.lib.c2d_fp_step(self.ctx, C.byref(call.sin), C.byref(call.sout)))
        return call.result()

    def last_fp_ms(self) -> float:
        ms = C.c_double()
        self._check(self.lib.c2d_last_fp_ms(self.ctx, C.byref(ms)))
        return ms.value

    def electron_state(self):
        """The context's device electron state (f_nt, Pnt), each [nz, nr, NUM_NT]."""
        f = np.zeros((self.nz, self.nr, abi.NUM_NT))
        p = np.zeros_like(f)
        mv = lambda a: abi.MArray3(a.ctypes.data_as(abi.PD), 1, self.nr * abi.NUM_NT, abi.NUM_NT)
        self._check(self.lib.c2d_electron_state(self.ctx, mv(f), mv(p)))
        return f, p

    # -- RCCL tally all-reduce (xec_add / cens_add_up over xGMI) --------------
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = load_library()
        buf = C.create_string_buffer(abi.COMM_ID_BYTES)
        rc = lib.c2d_comm_unique_id(buf, abi.COMM_ID_BYTES)
        if rc != 0:
            raise C2DError(rc, "c2d_comm_unique_id failed")
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, world: int) -> None:
        buf = C.create_string_buffer(bytes(uid), abi.COMM_ID_BYTES)
        self._check(self.lib.c2d_comm_init(self.ctx, buf, int(rank), int(world)))

    def allreduce_tallies(self) -> None:
        """One in-place RCCL all-reduce of the fused tally buffer."""
        self._check(self.lib.c2d_allreduce_tallies(self.ctx))

    # -- emission / absorption tables (imcgen2d.f:209-333, volume_em) ---------
    def volume_em(self, dt: float, state: dict, tables_to_host: bool = True) -> dict:
        """kappa_tot, eps_tot, eps_th [nz, nr, 400], B_field, Eloss_sy/cy/th/tot
        [nz, nr] and E_ph [400] for the cell state (tea, tna, n_e, B_field,
        f_pair, zsurf, vol [nz, nr], f_nt [nz, nr, 200], ep_switch).
        f_nt None: the device electron state; tables_to_host False: the three
        tables stay on the device for set_step(kappa_tot=None, ...)."""
        call = abi.VemCall(dt, state, tables_to_host)
        self._check(self.lib.c2d_volume_em(self.ctx, C.byref(call.sin), C.byref(call.sout)))
        return call.res

    def last_vem_ms(self) -> float:
        ms = C.c_double()
        self._check(self.lib.c2d_last_vem_ms(self.ctx, C.byref(ms)))
        return ms.value

    # -- the escape-event file (imcleak2d.f:181), written by the library -----
    def events_write(self, path, append: bool = False) -> int:
        """Write the last transport step's escape events to `path` as
        p###_evb.dat text, formatted on the device (c2d_events_write); returns
        the records written."""
        n = C.c_int64()
        self._check(self.lib.c2d_events_write(self.ctx, os.fsencode(path), int(bool(append)), C.byref(n)))
        return n.value

    def events_write_from(self, events, path, append: bool = False) -> None:
        """The same for events [n, 7] of the caller: a numpy array, or a
        float64 torch tensor on this context's GPU (no copy)."""
        if hasattr(events, "data_ptr"):
            t = events
            if not t.is_cuda:
                return self.events_write_from(t.numpy(), path, append)
            assert t.dtype.itemsize == 8 and t.is_floating_point() and t.is_contiguous()
            assert t.numel() % abi.EVENT_WORDS == 0
            ptr, n, dev = t.data_ptr(), t.numel() // abi.EVENT_WORDS, 1
            keep = t
        else:
            keep = np.ascontiguousarray(events, np.float64).reshape(-1, abi.EVENT_WORDS)
            ptr, n, dev = keep.ctypes.data, len(keep), 0
        self._check(self.lib.c2d_events_write_from(self.ctx, C.c_void_p(ptr if n else None), n, dev,
                                                   os.fsencode(path), int(bool(append))))
        del keep

    def last_events_write(self) -> dict:
        """Timings of the last events_write* (c2d_last_events_write_ms)."""
        d = [C.c_double() for _ in range(4)]
        amb, ml, chunks = C.c_int64(), C.c_int64(), C.c_int32()
        self._check(self.lib.c2d_last_events_write_ms(self.ctx, *[C.byref(v) for v in d], C.byref(amb),
                                                      C.byref(ml), C.byref(chunks)))
        return {"scan_ms": d[0].value, "kernel_ms": d[1].value, "wait_ms": d[2].value, "io_ms": d[3].value,
                "ambiguous": amb.value, "multilimb": ml.value, "chunks": chunks.value}

    # -- the escape-event file read back, parsed on the device ----------------
    def _check_records(self, rc: int, n) -> int:
        """Like _check; the error carries the records delivered before it."""
        if rc != 0:
            e = C2DError(rc, self.lib.c2d_last_error(self.ctx).decode())
            e.records = n.value
            raise e
        return n.value

    def events_read(self, path, device: bool = False):
        """The events [n, 7] of the event file `path` (c2d_events_read): a
        numpy array, or with device=True a float64 torch tensor on this
        context's GPU.  Canonical records are parsed by a kernel, the rest of
        the file by the library's host parser."""
        def buffer(m):
            if device:
                import torch
                t = torch.empty((m, abi.EVENT_WORDS), dtype=torch.float64, device="cuda:%d" % self.grid.device)
                return t, t.data_ptr()
            a = np.empty((m, abi.EVENT_WORDS))
            return a, a.ctypes.data

        n = C.c_int64()
        try:
            cap = os.path.getsize(path) // 105 + 1      # a canonical file's records: one pass
        except OSError:
            cap = 1                                     # the library reports what is wrong with the file
        while True:
            out, ptr = buffer(cap)
            self._check_records(self.lib.c2d_events_read(self.ctx, os.fsencode(path), C.c_void_p(ptr), cap,
                                                         int(bool(device)), C.byref(n)), n)
            if n.value <= cap:
                return out[:n.value]
            cap = n.value                                # free format: more records than 105-byte slots

    def events_read_into(self, path, out) -> int:
        """Parse `path` into `out` (numpy [cap, 7] float64, or a cuda float64
        tensor): the first min(cap, n) records are stored; returns n."""
        n = C.c_int64()
        if hasattr(out, "data_ptr"):
            assert out.is_cuda and out.dtype.itemsize == 8 and out.is_floating_point() and out.is_contiguous()
            ptr, cap, dev = out.data_ptr(), out.numel() // abi.EVENT_WORDS, 1
        else:
            assert out.dtype == np.float64 and out.flags.c_contiguous
            ptr, cap, dev = out.ctypes.data, out.size // abi.EVENT_WORDS, 0
        return self._check_records(self.lib.c2d_events_read(self.ctx, os.fsencode(path), C.c_void_p(ptr if cap else None),
                                                            cap, dev, C.byref(n)), n)

    def last_events_read(self) -> dict:
        """Timings and counts of the last events_read / obs*_accumulate_file
        (c2d_last_events_read_ms)."""
        d = [C.c_double() for _ in range(4)]
        k = [C.c_int64() for _ in range(3)]
        chunks = C.c_int32()
        self._check(self.lib.c2d_last_events_read_ms(self.ctx, *[C.byref(v) for v in d], *[C.byref(v) for v in k],
                                                     C.byref(chunks)))
        return {"io_ms": d[0].value, "wait_ms": d[1].value, "kernel_ms": d[2].value, "host_parse_ms": d[3].value,
                "canonical": k[0].value, "host_parsed": k[1].value, "exact_fields": k[2].value,
                "chunks": chunks.value}

    last_events_read_ms = last_events_read

    # -- observer-frame binning (postprocessing/pspt.c, plcm.c) ---------------
    def obs_begin(self, binning) -> None:
        """Zero a device histogram for `binning` (observer.Binning)."""
        self._obs = binning
        self._obs_c = binning.to_ctypes()
        self._check(self.lib.c2d_obs_begin(self.ctx, C.byref(self._obs_c)))

    def obs_accumulate(self, events=None) -> None:
        """Bin host events [n, 7] (t_bound, xnu, ew, rpre, zpre, wmu, phi), or
        with None the last transport step's device event buffer."""
        if events is None:
            self._check(self.lib.c2d_obs_accumulate(self.ctx, None, 0))
            return
        ev = np.ascontiguousarray(events, np.float64).reshape(-1, abi.EVENT_WORDS)
        self._check(self.lib.c2d_obs_accumulate(self.ctx, ev.ctypes.data_as(abi.PD), len(ev)))

    def obs_accumulate_device(self, ptr: int, n: int) -> None:
        """Bin n events at device address `ptr` (e.g. tensor.data_ptr() of a
        cuda float64 [n, 7] tensor on this context's GPU)."""
        self._check(self.lib.c2d_obs_accumulate_device(self.ctx, C.c_void_p(ptr), n))

    def obs_accumulate_file(self, path) -> int:
        """Bin the event file `path`, chunk by chunk as the device parses it
        (c2d_obs_accumulate_file); returns the records binned.  A C2DError
        carries them as .records."""
        n = C.c_int64()
        return self._check_records(self.lib.c2d_obs_accumulate_file(self.ctx, os.fsencode(path), C.byref(n)), n)

    def obs_result(self):
        """Raw sums (F = sum ew, F2 = sum ew^2, count), each [n_t, n_mu, n_e],
        and the device milliseconds of the binning launches so far."""
        b = self._obs
        shape = (b.n_t, b.n_mu, b.n_e)
        F, F2, cnt = (np.zeros(shape) for _ in range(3))
        ms = C.c_double()
        self._check(self.lib.c2d_obs_result(self.ctx, F.ctypes.data_as(abi.PD),
                                            F2.ctypes.data_as(abi.PD),
                                            cnt.ctypes.data_as(abi.PD), C.byref(ms)))
        return F, F2, cnt, ms.value

    def obs_begin_pspt(self, deck: str = "") -> None:
        """The SED binning of pspt's input dialogue `deck` (c2d_obs_begin_pspt)."""
        from . import observer
        self._check(self.lib.c2d_obs_begin_pspt(self.ctx, deck.encode()))
        self._obs = observer.parse_pspt_deck(deck)

    def obs_write_pspt(self, path: str = "", factor: int = 0, world_sum: bool = False) -> None:
        """Write pspt's output file from the histogram so far (c2d_obs_write_pspt)."""
        self._check(self.lib.c2d_obs_write_pspt(self.ctx, str(path).encode(), int(factor), int(world_sum)))

    # -- observer sets: several binnings in one pass over the events ----------
    def obs_set_clear(self) -> None:
        """Drop every member of the observer set (c2d_obs_set_clear)."""
        self._check(self.lib.c2d_obs_set_clear(self.ctx))

    def obs_set_add(self, binning) -> int:
        """Add `binning` (observer.Binning) with a zeroed histogram; its id."""
        i = C.c_int32(-1)
        self._check(self.lib.c2d_obs_set_add(self.ctx, C.byref(binning.to_ctypes()), C.byref(i)))
        return i.value

    def obs_set_add_pspt(self, deck: str = "") -> int:
        """Add the SED binning of pspt's input dialogue `deck`; its id."""
        i = C.c_int32(-1)
        self._check(self.lib.c2d_obs_set_add_pspt(self.ctx, deck.encode(), C.byref(i)))
        return i.value

    def obs_set_add_plcm(self, deck: str = "") -> int:
        """Add the light-curve binning of plcm's input dialogue `deck`; its id."""
        i = C.c_int32(-1)
        self._check(self.lib.c2d_obs_set_add_plcm(self.ctx, deck.encode(), C.byref(i)))
        return i.value

    def obs_set_accumulate(self, events=None) -> None:
        """Bin host events [n, 7] into every member in one pass, or with None
        the last transport step's device event buffer."""
        if events is None:
            self._check(self.lib.c2d_obs_set_accumulate(self.ctx, None, 0))
            return
        ev = np.ascontiguousarray(events, np.float64).reshape(-1, abi.EVENT_WORDS)
        self._check(self.lib.c2d_obs_set_accumulate(self.ctx, ev.ctypes.data_as(abi.PD), len(ev)))

    def obs_set_accumulate_device(self, ptr: int, n: int) -> None:
        """Bin n events at device address `ptr` into every member."""
        self._check(self.lib.c2d_obs_set_accumulate_device(self.ctx, C.c_void_p(ptr), n))

    def obs_set_accumulate_file(self, path) -> int:
        """Bin the event file `path` into every member, chunk by chunk as the
        device parses it; returns the records binned."""
        n = C.c_int64()
        return self._check_records(self.lib.c2d_obs_set_accumulate_file(self.ctx, os.fsencode(path), C.byref(n)), n)

    def obs_set_shape(self, member: int):
        """(n_t, n_mu, n_e, lds_rows) of a member: its histogram shape and
        the leading time rows the kernel keeps in LDS."""
        v = [C.c_int32() for _ in range(4)]
        self._check(self.lib.c2d_obs_set_shape(self.ctx, int(member), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def obs_set_result(self, member: int):
        """Raw sums (F, F2, count) of a member, each [n_t, n_mu, n_e]."""
        shape = self.obs_set_shape(member)[:3]
        F, F2, cnt = (np.zeros(shape) for _ in range(3))
        self._check(self.lib.c2d_obs_set_result(self.ctx, int(member), F.ctypes.data_as(abi.PD),
                                                F2.ctypes.data_as(abi.PD), cnt.ctypes.data_as(abi.PD)))
        return F, F2, cnt

    def obs_set_kernel_ms(self):
        """Device milliseconds and number of the set's kernel launches so far."""
        ms, n = C.c_double(), C.c_int32()
        self._check(self.lib.c2d_obs_set_kernel_ms(self.ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def obs_set_write(self, member: int, path: str = "", factor: int = 0, world_sum: bool = False) -> None:
        """The tool's files of a deck member: `path` is pspt's output file, or
        the directory of plcm's files ("" = the deck's name / ".")."""
        self._check(self.lib.c2d_obs_set_write(self.ctx, int(member), str(path).encode(), int(factor),
                                               int(world_sum)))

    def obs_set_exact(self, w_max: float) -> None:
        """Make the observer set exact (c2d_obs_set_exact): integer sums, the
        same bits for any event order, batch split or shard count.  w_max
        bounds the rest-frame weight of any single event."""
        self._check(self.lib.c2d_obs_set_exact(self.ctx, float(w_max)))

    def obs_set_exact_info(self, member: int):
        """(e, n_rejected) of a member of an exact set: its exponent bound
        and the events whose weight the bound did not admit."""
        e, r = C.c_int32(), C.c_int64()
        self._check(self.lib.c2d_obs_set_exact_info(self.ctx, int(member), C.byref(e), C.byref(r)))
        return e.value, r.value

    def obs_set_state(self, member: int) -> np.ndarray:
        """The integers of a member of an exact set as its state, u64 words
        (include/compton2d.h "Exact observer sets")."""
        n = C.c_int64()
        self._check(self.lib.c2d_obs_set_state_words(self.ctx, int(member), C.byref(n)))
        out = np.zeros(n.value, np.uint64)
        self._check(self.lib.c2d_obs_set_state(self.ctx, int(member), out.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               out.size))
        return out

    def obs_set_merge(self, member: int, state) -> None:
        """Add an exported state into a member of an exact set."""
        s = np.ascontiguousarray(state, np.uint64).reshape(-1)
        self._check(self.lib.c2d_obs_set_merge(self.ctx, int(member), s.ctypes.data_as(C.POINTER(C.c_uint64)), s.size))

    def fp_tridag(self, a, b, c, r, x0=None) -> np.ndarray:
        """Batched tridag (src/update2d.f:2476-2518); arrays [ncell, nt]."""
        a, b, c, r = (np.ascontiguousarray(x, np.float64) for x in (a, b, c, r))
        ncell, nt = a.shape
        x = np.zeros_like(a) if x0 is None else np.array(x0, np.float64, copy=True)
        fin = abi.FpIn(ncell, a.ctypes.data_as(abi.PD), b.ctypes.data_as(abi.PD),
                       c.ctypes.data_as(abi.PD), r.ctypes.data_as(abi.PD), nt)
        self._check(self.lib.c2d_fp_tridag(self.ctx, C.byref(fin), x.ctypes.data_as(abi.PD)))
        return x


def obs_engine(device: int = 0) -> Engine:
    """A context for observer-frame binning only (no transport tables used)."""
    from . import synth
    g = synth.c2_workload(nz=1, nr=1, sources=1, device=device, census_capacity=1024,
                          event_capacity=1024).grid
    g.queue_capacity = 1024
    return Engine(g)


def device_mcdonald(z: np.ndarray, device: int = 0):
    """K2(z), K3(z) by the GPU's wave-level McDonald series and the shader
    cycles of each evaluation (c2d_selftest_mcdonald)."""
    lib = load_library()
    lib.c2d_selftest_mcdonald.restype = C.c_int
    lib.c2d_selftest_mcdonald.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
    z = np.ascontiguousarray(z, np.float64)
    out = np.zeros((len(z), 3))
    rc = lib.c2d_selftest_mcdonald(device, z.ctypes.data_as(abi.PD), len(z), out.ctypes.data_as(abi.PD))
    if rc != 0:
        raise C2DError(rc, "c2d_selftest_mcdonald failed")
    return out[:, 0], out[:, 1], out[:, 2]


def device_mcd_fast(z: np.ndarray, device: int = 0) -> np.ndarray:
    """The fast FP kernel's McDonald pair at z from its moment table and from
    its term-by-term series (c2d_selftest_mcd_fast): rows (K2, K3 table, K2,
    K3 series, table answered, cycles of the table's gamma_bar, cycles of the
    series, gamma_bar from the table as the fast kernel forms it)."""
    lib = load_library()
    lib.c2d_selftest_mcd_fast.restype = C.c_int
    lib.c2d_selftest_mcd_fast.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
    z = np.ascontiguousarray(z, np.float64)
    out = np.zeros((len(z), 8))
    rc = lib.c2d_selftest_mcd_fast(device, z.ctypes.data_as(abi.PD), len(z), out.ctypes.data_as(abi.PD))
    if rc != 0:
        raise C2DError(rc, "c2d_selftest_mcd_fast failed")
    return out


def fp_fast_dims():
    """(block, tpt) of the fast FP kernel: its workgroup size and its McDonald
    terms per thread per pass (c2d_selftest_fp_dims; needs no GPU)."""
    lib = load_library()
    lib.c2d_selftest_fp_dims.restype = C.c_int
    lib.c2d_selftest_fp_dims.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    bs, tpt = C.c_int32(), C.c_int32()
    lib.c2d_selftest_fp_dims(C.byref(bs), C.byref(tpt))
    return bs.value, tpt.value


FP_SOLVE_SPIKE, FP_SOLVE_PCR = 0, 1


def device_fp_solve(solver: int, a, b, c, d, device: int = 0) -> np.ndarray:
    """The fast FP kernel's tridiagonal solver (FP_SOLVE_SPIKE: the one it
    runs, FP_SOLVE_PCR: plain cyclic reduction) on the systems a, b, c, d
    [nsys, 200], one workgroup solving them one after another
    (c2d_selftest_fp_solve): x [nsys, block], every thread's result."""
    lib = load_library()
    lib.c2d_selftest_fp_solve.restype = C.c_int
    lib.c2d_selftest_fp_solve.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_double)] * 4 + \
        [C.c_int, C.POINTER(C.c_double)]
    a, b, c, d = (np.ascontiguousarray(v, np.float64) for v in (a, b, c, d))
    nsys, nt = a.shape
    if nt != abi.NUM_NT or not (b.shape == c.shape == d.shape == a.shape):
        raise ValueError("systems are [nsys, %d]" % abi.NUM_NT)
    x = np.zeros((nsys, fp_fast_dims()[0]))
    rc = lib.c2d_selftest_fp_solve(device, int(solver), *(v.ctypes.data_as(abi.PD) for v in (a, b, c, d)),
                                   nsys, x.ctypes.data_as(abi.PD))
    if rc != 0:
        raise C2DError(rc, "c2d_selftest_fp_solve failed")
    return x


FP_BLK_SUM2, FP_BLK_SCAN, FP_BLK_SCAN_SUM, FP_BLK_MINMAX, FP_BLK_MIN2, FP_BLK_FIRSTS = range(6)


def device_fp_block(op: int, in_a, in_b=None, device: int = 0) -> np.ndarray:
    """One block primitive of the fast FP kernel on per-thread values
    (c2d_selftest_fp_block), every thread's results: [nvec, R, block].
    sum2, scan_sum: float64 in_a, in_b [nvec, block] -> (a, b) / (prefix,
    total, sum of in_b); scan: in_a -> (prefix, total); minmax, min2: int32
    -> int32 pairs; firsts: flags [nvec, tpt, block] -> int32 first set terms."""
    lib = load_library()
    lib.c2d_selftest_fp_block.restype = C.c_int
    lib.c2d_selftest_fp_block.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    bs, tpt = fp_fast_dims()
    tin = np.float64 if op <= FP_BLK_SCAN_SUM else (np.int32 if op <= FP_BLK_MIN2 else np.uint8)
    shape = (tpt, bs) if op == FP_BLK_FIRSTS else (bs,)
    a = np.ascontiguousarray(in_a, tin)
    b = a if in_b is None and op == FP_BLK_SCAN else np.ascontiguousarray(in_b, tin)
    if a.shape[1:] != shape or b.shape != a.shape:
        raise ValueError("op %d takes [nvec, %s]" % (op, ", ".join(map(str, shape))))
    nres = 3 if op == FP_BLK_SCAN_SUM else 2
    out = np.zeros((a.shape[0], nres, bs), np.float64 if op <= FP_BLK_SCAN_SUM else np.int32)
    rc = lib.c2d_selftest_fp_block(device, int(op), a.ctypes.data, b.ctypes.data, a.shape[0], out.ctypes.data)
    if rc != 0:
        raise C2DError(rc, "c2d_selftest_fp_block failed")
    return out


def device_geom(nr: int, rays: np.ndarray, device: int = 0) -> np.ndarray:
    """(disbr, trldb) of the flight step's r-boundary distance for rays
    (rpre, Eta, wmu, rbnd) on the GPU, with the fast build's sqrt / reciprocal
    after `nr` Newton steps, or IEEE (nr = 0) (c2d_selftest_geom)."""
    lib = load_library()
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 4)
    out = np.zeros((rays.shape[0], 2))
    rc = lib.c2d_selftest_geom(device, nr, rays.ctypes.data_as(abi.PD), out.ctypes.data_as(abi.PD),
                               rays.shape[0])
    if rc != 0:
        raise C2DError(rc, "c2d_selftest_geom failed")
    return out


def device_math(fn: int, x: np.ndarray, device: int = 0) -> np.ndarray:
    """Evaluate c2d_math function `fn` on the GPU (c2d_selftest_math)."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float64)
    y = np.zeros_like(x)
    rc = lib.c2d_selftest_math(device, fn, x.ctypes.data_as(abi.PD), y.ctypes.data_as(abi.PD),
                               x.size)
    if rc != 0:
        raise C2DError(rc, "c2d_selftest_math failed")
    return y


def device_fmt_e14_7(x: np.ndarray, device: int = 0) -> np.ndarray:
    """Fortran E14.7 of every value of x on the GPU (c2d_selftest_fmt): uint8 [n, 14]."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float64).ravel()
    out = C.create_string_buffer(14 * x.size + 1)
    rc = lib.c2d_selftest_fmt(device, x.ctypes.data_as(abi.PD), x.size, out)
    if rc != 0:
        raise C2DError(rc, "c2d_selftest_fmt failed")
    return np.frombuffer(out.raw[:14 * x.size], np.uint8).reshape(-1, 14)


def device_reflect(boundary: int, cr_sent: int, spec_switch: int, states: np.ndarray, keys: np.ndarray,
                   device: int = 0):
    """The kernels' reflection functions on packet states (c2d_selftest_reflect):
    states [n, 8] = xnu, ew, wmu, rpre, zpre, phi, dcen, tbbl; keys uint64 [n].
    Returns (out [n, 10] = xnu, ew, wmu, rpre, zpre, t_bound, draws, idead, n_in,
    n_out; the sum of the scratch Ed_ref)."""
    lib = load_library()
    st = np.ascontiguousarray(states, np.float64).reshape(-1, 8)
    k = np.ascontiguousarray(keys, np.uint64).ravel()
    assert k.size == st.shape[0]
    out = np.zeros((st.shape[0], 10))
    ed = C.c_double()
    rc = lib.c2d_selftest_reflect(device, int(boundary), int(cr_sent), int(spec_switch), st.ctypes.data_as(abi.PD),
                                  k.ctypes.data_as(C.POINTER(C.c_uint64)), st.shape[0], out.ctypes.data_as(abi.PD),
                                  C.byref(ed))
    if rc != 0:
        raise C2DError(rc, "c2d_selftest_reflect failed")
    return out, ed.value


def device_scan_e14_7(fields, device: int = 0):
    """Parse 14-byte E14.7 fields (bytes of length 14 n, or a uint8 array
    [n, 14]) on the GPU (c2d_selftest_scan): (bits uint64 [n], status int32
    [n]); a field that is not canonical has status -1 and bits 0."""
    lib = load_library()
    text = fields if isinstance(fields, (bytes, bytearray)) else np.ascontiguousarray(fields, np.uint8).tobytes()
    assert len(text) % 14 == 0
    n = len(text) // 14
    out = np.zeros(n, np.float64)
    st = np.zeros(n, np.int32)
    rc = lib.c2d_selftest_scan(device, bytes(text), n, out.ctypes.data_as(abi.PD), st.ctypes.data_as(abi.PI32))
    if rc != 0:
        raise C2DError(rc, "c2d_selftest_scan failed")
    return out.view(np.uint64), st


def ic_loss(gnt: np.ndarray, E_field: np.ndarray, device: int = 0, fortran: bool = False,
            kernel_ms: Optional[list] = None) -> np.ndarray:
    """F_IC [n_el, n_ph] of IC_loss (src/icloss2d.f) on the GPU (c2d_ic_loss).
    fortran=True fills a Fortran-ordered F_IC(n_el, n_ph) through the strides
    (s_i = 1, s_ph = n_el).  kernel_ms: a list that receives the HIP-event time
    of the series kernel in ms."""
    lib = load_library()
    gnt, E_field = abi.setup_grid_args(gnt, E_field)
    F, s_i, s_ph = abi.ic_loss_out(gnt.size, E_field.size, fortran)
    ms = C.c_double(0.0)
    rc = lib.c2d_ic_loss_timed(device, gnt.ctypes.data_as(abi.PD), gnt.size, E_field.ctypes.data_as(abi.PD),
                               E_field.size, F.ctypes.data_as(abi.PD), s_i, s_ph,
                               C.byref(ms) if kernel_ms is not None else None)
    if rc != 0:
        raise C2DError(rc, "c2d_ic_loss failed")
    if kernel_ms is not None:
        kernel_ms.append(ms.value)
    return F


def setup_electrons(tea, amxwl, gmin, gmax, p_nth, device: int = 0) -> dict:
    """gam_min and P_nontherm (src/gamma1_2d.f, src/nontherm2d.f) of n zones on
    the GPU (c2d_setup_electrons): gmin, N_nth, gbar_nth [n], f_nt, Pnt [n, 200]."""
    lib = load_library()
    ins, out = abi.setup_electron_args(tea, amxwl, gmin, gmax, p_nth)
    rc = lib.c2d_setup_electrons(device, ins[0].size, *[a.ctypes.data_as(abi.PD) for a in ins],
                                 *[out[k].ctypes.data_as(abi.PD) for k in abi.SETUP_ELECTRON_OUT])
    if rc != 0:
        raise C2DError(rc, "c2d_setup_electrons failed")
    return out
