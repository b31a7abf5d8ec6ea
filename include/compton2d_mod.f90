! compton2d_mod.f90 -- Fortran 2003 (iso_c_binding) interface to include/compton2d.h.
!
! This is the binding a maintainer adds to the reference's Fortran host
! (bbw7561135/Compton2d src/) so that the worker-side calls
!     call imcfield2d ; call imcvol2d ; call imcsurf2d      (src/xec2d.f:167-176)
! become one c2d_transport_step() per GPU, and `call update`
! (src/xec2d.f:86-87, src/update2d.f:7-327) one c2d_fp_step(), with the COMMON
! tables passed in place through (c_loc, strides).  See INTEGRATION.md.
module compton2d
  use iso_c_binding
  implicit none

  integer(c_int), parameter :: C2D_OK = 0, C2D_E_ARG = -1, C2D_E_HIP = -2, &
       C2D_E_CENSUS_OVERFLOW = -3, C2D_E_EVENT_OVERFLOW = -4, C2D_E_QUEUE_OVERFLOW = -5, &
       C2D_E_NOMEM = -6, C2D_E_STATE = -7, C2D_E_FP = -8, C2D_E_RCCL = -9, C2D_E_IO = -10, &
       C2D_E_NONFINITE = -11
  ! c2d_step_in%device_tables flags; RCCL unique-id size (c2d_comm_unique_id)
  integer(c_int32_t), parameter :: C2D_DEV_EMISSION = 1, C2D_DEV_ELECTRONS = 2
  integer(c_int32_t), parameter :: C2D_FP_EXACT = 0, C2D_FP_FAST = 1, C2D_FP_AUTO = 2
  integer, parameter :: C2D_COMM_ID_BYTES = 128
  integer(c_int32_t), parameter :: C2D_COMTOT_EXACT = 0, C2D_COMTOT_TABLE = 1
  integer(c_int32_t), parameter :: C2D_TRK_SRC = 0, C2D_TRK_2012_11 = 1
  integer(c_int32_t), parameter :: C2D_CKPT_HAS_KAPPA = 1, C2D_CKPT_HAS_ELECTRONS = 2
  integer(c_int32_t), parameter :: C2D_CKPT_APPEND = 1, C2D_CKPT_CENSUS_ONLY = 2
  integer, parameter :: C2D_NCOUNTERS = 16, C2D_CNT_STEPS = 0, C2D_CNT_ESCAPES = 1, &
       C2D_CNT_CENSUS = 2

  type, bind(C) :: c2d_array3
     type(c_ptr) :: data = c_null_ptr
     integer(c_int64_t) :: s_i = 0, s_j = 0, s_k = 0
  end type c2d_array3

  type, bind(C) :: c2d_array2
     type(c_ptr) :: data = c_null_ptr
     integer(c_int64_t) :: s_j = 0, s_k = 0
  end type c2d_array2

  type, bind(C) :: c2d_spectrum
     integer(c_int32_t) :: nfile = 0
     type(c_ptr) :: E_file = c_null_ptr, a1 = c_null_ptr, I_file = c_null_ptr, &
          F_file = c_null_ptr, P_file = c_null_ptr
  end type c2d_spectrum

  type, bind(C) :: c2d_config
     integer(c_int32_t) :: nz = 0, nr = 0
     real(c_double) :: rmin = 0, zmin = 0
     type(c_ptr) :: z = c_null_ptr, r = c_null_ptr, E_ph = c_null_ptr, &
          E_field = c_null_ptr, gnt = c_null_ptr
     integer(c_int32_t) :: nphtotal = 0
     type(c_ptr) :: hu = c_null_ptr
     integer(c_int32_t) :: nph_lc = 0
     type(c_ptr) :: Elcmin = c_null_ptr, Elcmax = c_null_ptr
     integer(c_int32_t) :: nmu = 0
     type(c_ptr) :: mu = c_null_ptr
     integer(c_int32_t) :: split1 = 10, split2 = 10, split3 = 3, spl3_trg = 10
     integer(c_int32_t) :: spec_switch = 0, cr_sent = 0, pair_switch = 0, kappa_lag = 1
     integer(c_int32_t) :: comtot_mode = C2D_COMTOT_TABLE, device = 0
     integer(c_int64_t) :: seed = 99999
     integer(c_int32_t) :: rank = 0, world = 1
     integer(c_int64_t) :: census_capacity = 5000000, event_capacity = 5000000, &
          queue_capacity = 262144
     integer(c_int32_t) :: census_inplace = 0
     integer(c_int32_t) :: trk_variant = 0
  end type c2d_config

  type, bind(C) :: c2d_step_in
     integer(c_int32_t) :: ncycle = 0
     real(c_double) :: time = 0, dt = 0
     type(c2d_array3) :: kappa_tot, eps_tot, eps_th, f_nt, Pnt
     type(c2d_array2) :: n_e, Eloss_th, Eloss_tot, zsurf, ewsv
     type(c2d_array2) :: nsv                     ! int32 data (c2d_iarray2)
     type(c_ptr) :: nsurfi = c_null_ptr, nsurfo = c_null_ptr, ewsurfi = c_null_ptr, &
          ewsurfo = c_null_ptr, nsurfu = c_null_ptr, nsurfl = c_null_ptr, &
          ewsurfu = c_null_ptr, ewsurfl = c_null_ptr
     type(c_ptr) :: tbbi = c_null_ptr, tbbo = c_null_ptr, tbbu = c_null_ptr, tbbl = c_null_ptr
     type(c_ptr) :: spec_i = c_null_ptr, spec_o = c_null_ptr, spec_u = c_null_ptr, &
          spec_l = c_null_ptr
     integer(c_int32_t) :: n_spectra = 0
     type(c_ptr) :: spectra = c_null_ptr
     integer(c_int32_t) :: device_tables = 0     ! C2D_DEV_* flags
  end type c2d_step_in

  ! ---- Fokker-Planck update (c2d_fp_set_config / c2d_fp_step) ----
  integer, parameter :: C2D_FP_NDIAG = 8, C2D_FP_STEPS = 5, C2D_FP_SKIPPED = 6

  ! census population control (c2d_census_stats / c2d_census_roulette)
  integer, parameter :: C2D_ROULETTE_GROUPS_MAX = 32

  type, bind(C) :: c2d_roulette_out
     integer(c_int64_t) :: n_before = 0, n_after = 0, n_tested = 0   ! n_tested: records with ew < w
     real(c_double) :: e_before = 0, e_after = 0, kernel_ms = 0
  end type c2d_roulette_out

  ! census splitting (c2d_census_split): the upper weight window
  integer, parameter :: C2D_SPLIT_COPIES_MAX = 64
  integer(c_int32_t), parameter :: C2D_SPLIT_DRY = 1   ! flags: count only, the census stays as it is

  type, bind(C) :: c2d_split_out
     integer(c_int64_t) :: n_before = 0, n_after = 0, n_split = 0   ! n_split: records with m > 1
     real(c_double) :: e_before = 0, e_after = 0, kernel_ms = 0
  end type c2d_split_out

  ! the census comb (c2d_census_comb_hist / c2d_census_comb_collect)
  integer, parameter :: C2D_COMB_BINS = 2048

  type, bind(C) :: c2d_comb_out
     integer(c_int64_t) :: n_records = 0, n_fixed = 0, n_pool = 0, n_match = 0
     real(c_double) :: kernel_ms = 0
  end type c2d_comb_out

  type, bind(C) :: c2d_marray3
     type(c_ptr) :: data = c_null_ptr
     integer(c_int64_t) :: s_i = 0, s_j = 0, s_k = 0
  end type c2d_marray3

  type, bind(C) :: c2d_marray2
     type(c_ptr) :: data = c_null_ptr
     integer(c_int64_t) :: s_j = 0, s_k = 0
  end type c2d_marray2

  type, bind(C) :: c2d_fp_config              ! reader.f:512-559, general.pa:27-28
     integer(c_int32_t) :: pair_switch = 0
     real(c_double) :: df_implicit = 1.d-2, df_T = 2.5d-1, r_esc = 0.3d0, r_acc = 1.d0
     integer(c_int32_t) :: cf_sentinel = 0
     real(c_double) :: r_flare = 0, z_flare = 0, t_flare = 0, sigma_r = 1, sigma_z = 1, &
          sigma_t = 1, flare_amp = 0
     integer(c_int32_t) :: inj_switch = 0, inj_dis = 2, g2var_switch = 0, pick_sw = 0
     real(c_double) :: inj_g1 = 0, inj_g2 = 0, inj_p = 0, inj_t = 0, inj_L = 0, &
          pick_rate = 0, inj_gg = 0, inj_sigma = 1, inj_v = 0
     type(c_ptr) :: F_IC = c_null_ptr             ! F_IC(num_nt, nphfield), COMMON /fic/
     integer(c_int64_t) :: F_IC_s_i = 1, F_IC_s_ph = 200
  end type c2d_fp_config

  type, bind(C) :: c2d_fp_step_in              ! what FP_send_job packs (fp_mpi.f:632-686)
     integer(c_int32_t) :: ncycle = 0
     real(c_double) :: time = 0, dt = 0
     type(c2d_array2) :: tea, tna, n_e, B_field, Eloss_sy, ec_old, turb_lev, vol
     type(c2d_array2) :: f_pair, ecens           ! ecens: null data = device tallies
     type(c2d_array3) :: n_field                 ! null data = device tallies
  end type c2d_fp_step_in

  type, bind(C) :: c2d_fp_step_out             ! updated in place (fp_mpi.f:972-1003)
     type(c2d_marray3) :: f_nt, Pnt
     type(c2d_marray2) :: Te_new, tea, n_e, gmin, gmax, amxwl, p_nth
     type(c_ptr) :: zone_diag = c_null_ptr
     real(c_double) :: E_tot_old = 0, E_tot_new = 0, hr_total = 0, hr_st_total = 0, dT_max = 0
  end type c2d_fp_step_out

  ! ---- emission / absorption tables (c2d_volume_em; imcgen2d.f:209-333) ----
  type, bind(C) :: c2d_iarray2
     type(c_ptr) :: data = c_null_ptr
     integer(c_int64_t) :: s_j = 0, s_k = 0
  end type c2d_iarray2

  type, bind(C) :: c2d_vem_in
     real(c_double) :: dt = 0
     type(c2d_array2) :: tea, tna, n_e, B_field, f_pair, zsurf, vol
     type(c2d_iarray2) :: ep_switch              ! null data: all 0
     type(c2d_array3) :: f_nt
  end type c2d_vem_in

  type, bind(C) :: c2d_vem_out
     type(c2d_marray3) :: kappa_tot, eps_tot, eps_th
     type(c2d_marray2) :: B_field, Eloss_sy, Eloss_cy, Eloss_th, Eloss_tot
     type(c_ptr) :: E_ph = c_null_ptr
  end type c2d_vem_out

  ! ---- observer-frame binning (c2d_obs_*; postprocessing/pspt.c, plcm.c) ----
  integer, parameter :: C2D_OBS_SED = 0, C2D_OBS_LC = 1
  integer, parameter :: C2D_OBS_SET_MAX = 8     ! members of an observer set (c2d_obs_set_*)

  ! a checkpoint's header as c2d_checkpoint_info reports it (c2d_ckpt_info)
  type, bind(C) :: c2d_ckpt_info
     integer(c_int32_t) :: version = 0, nz = 0, nr = 0, nmu = 0
     integer(c_int32_t) :: encoded = 0, rank = 0, world = 0, ncycle = 0
     integer(c_int32_t) :: sections = 0, fp_auto_known = 0, fp_auto_exact = 0, reserved = 0
     integer(c_int64_t) :: grid_digest = 0, seed = 0      ! unsigned in C: the same 64 bits
     real(c_double) :: time = 0.d0, dt = 0.d0
     integer(c_int64_t) :: n_records = 0, chunk = 0, user_bytes = 0, file_bytes = 0
  end type c2d_ckpt_info

  type, bind(C) :: c2d_obs_bins
     integer(c_int32_t) :: mode = 0
     real(c_double) :: gam_bulk = 33.d0, rmax = 1.d16, t_offset = 0.d0
     integer(c_int32_t) :: n_t = 0
     type(c_ptr) :: t0 = c_null_ptr, t1 = c_null_ptr
     integer(c_int32_t) :: n_mu = 0
     type(c_ptr) :: mu0 = c_null_ptr, mu1 = c_null_ptr
     integer(c_int32_t) :: n_e = 0
     type(c_ptr) :: E0 = c_null_ptr, E1 = c_null_ptr
  end type c2d_obs_bins

  type, bind(C) :: c2d_tally_layout
     integer(c_int64_t) :: edep, prdep, ecens, npcen, n_field, E_IC, nelectron, fout, &
          edout, erlki, erlko, erlku, erlkl, Ed_in, counters, total
  end type c2d_tally_layout

  interface
     integer(c_int) function c2d_init(cfg, ctx) bind(C, name='c2d_init')
       import :: c_int, c_ptr, c2d_config
       type(c2d_config), intent(in) :: cfg
       type(c_ptr), intent(out) :: ctx
     end function c2d_init

     subroutine c2d_finalize(ctx) bind(C, name='c2d_finalize')
       import :: c_ptr
       type(c_ptr), value :: ctx
     end subroutine c2d_finalize

     type(c_ptr) function c2d_last_error(ctx) bind(C, name='c2d_last_error')
       import :: c_ptr
       type(c_ptr), value :: ctx
     end function c2d_last_error

     integer(c_int) function c2d_transport_step(ctx, sin) bind(C, name='c2d_transport_step')
       import :: c_int, c_ptr, c2d_step_in
       type(c_ptr), value :: ctx
       type(c2d_step_in), intent(in) :: sin
     end function c2d_transport_step

     integer(c_int) function c2d_set_step(ctx, sin) bind(C, name='c2d_set_step')
       import :: c_int, c_ptr, c2d_step_in
       type(c_ptr), value :: ctx
       type(c2d_step_in), intent(in) :: sin
     end function c2d_set_step

     integer(c_int) function c2d_set_clock(ctx, ncycle, time, dt) bind(C, name='c2d_set_clock')
       import :: c_int, c_ptr, c_int32_t, c_double
       type(c_ptr), value :: ctx
       integer(c_int32_t), value :: ncycle
       real(c_double), value :: time, dt
     end function c2d_set_clock

     integer(c_int) function c2d_run_step(ctx) bind(C, name='c2d_run_step')
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2d_run_step

     integer(c_int) function c2d_tally_layout_get(ctx, lay) bind(C, name='c2d_tally_layout_get')
       import :: c_int, c_ptr, c2d_tally_layout
       type(c_ptr), value :: ctx
       type(c2d_tally_layout), intent(out) :: lay
     end function c2d_tally_layout_get

     integer(c_int) function c2d_tally_download(ctx, host, n) bind(C, name='c2d_tally_download')
       import :: c_int, c_ptr, c_double, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: host(*)
       integer(c_int64_t), value :: n
     end function c2d_tally_download

     integer(c_int) function c2d_tally_download_range(ctx, host, offset, n) &
         bind(C, name='c2d_tally_download_range')
       import :: c_int, c_ptr, c_double, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: host(*)
       integer(c_int64_t), value :: offset, n
     end function c2d_tally_download_range

     integer(c_int) function c2d_events(ctx, buf, cap, n) bind(C, name='c2d_events')
       import :: c_int, c_ptr, c_double, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: buf(7, *)
       integer(c_int64_t), value :: cap
       integer(c_int64_t), intent(out) :: n
     end function c2d_events

     ! the last step's escape events as p###_evb.dat text (imcleak2d.f:181),
     ! formatted on the device; path NUL-terminated; append /= 0 adds to the file
     integer(c_int) function c2d_events_write(ctx, path, append, n_written) &
          bind(C, name='c2d_events_write')
       import :: c_int, c_ptr, c_char, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int32_t), value :: append
       integer(c_int64_t), intent(out) :: n_written
     end function c2d_events_write

     ! the same for n caller-supplied events: c_loc of a host array
     ! (on_device = 0) or a device address (on_device /= 0)
     integer(c_int) function c2d_events_write_from(ctx, events, n, on_device, path, append) &
          bind(C, name='c2d_events_write_from')
       import :: c_int, c_ptr, c_char, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx, events
       integer(c_int64_t), value :: n
       integer(c_int32_t), value :: on_device
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int32_t), value :: append
     end function c2d_events_write_from

     ! an event file back to events, parsed on the device: the first
     ! min(cap, n) records to buf (c_loc of a host array, or a device
     ! address with on_device /= 0); n = the records of the file
     integer(c_int) function c2d_events_read(ctx, path, buf, cap, on_device, n) &
          bind(C, name='c2d_events_read')
       import :: c_int, c_ptr, c_char, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       type(c_ptr), value :: buf
       integer(c_int64_t), value :: cap
       integer(c_int32_t), value :: on_device
       integer(c_int64_t), intent(out) :: n
     end function c2d_events_read

     ! bin an event file chunk by chunk as it is parsed (after c2d_obs_begin)
     integer(c_int) function c2d_obs_accumulate_file(ctx, path, n) &
          bind(C, name='c2d_obs_accumulate_file')
       import :: c_int, c_ptr, c_char, c_int64_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int64_t), intent(out) :: n
     end function c2d_obs_accumulate_file

     integer(c_int) function c2d_last_events_read_ms(ctx, io_ms, wait_ms, kernel_ms, host_parse_ms, &
          canonical, host_parsed, exact_fields, chunks) bind(C, name='c2d_last_events_read_ms')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: io_ms, wait_ms, kernel_ms, host_parse_ms
       integer(c_int64_t), intent(out) :: canonical, host_parsed, exact_fields
       integer(c_int32_t), intent(out) :: chunks
     end function c2d_last_events_read_ms

     integer(c_int) function c2d_census_count(ctx, n) bind(C, name='c2d_census_count')
       import :: c_int, c_ptr, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int64_t), intent(out) :: n
     end function c2d_census_count

     integer(c_int) function c2d_census_export(ctx, d6, i5, keys, cap, n) &
          bind(C, name='c2d_census_export')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: d6(6, *)
       integer(c_int32_t), intent(out) :: i5(5, *)
       integer(c_int64_t), intent(out) :: keys(*)
       integer(c_int64_t), value :: cap
       integer(c_int64_t), intent(out) :: n
     end function c2d_census_export

     integer(c_int) function c2d_census_import(ctx, d6, i5, keys, n) &
          bind(C, name='c2d_census_import')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: d6(6, *)
       integer(c_int32_t), intent(in) :: i5(5, *)
       integer(c_int64_t), intent(in) :: keys(*)
       integer(c_int64_t), value :: n
     end function c2d_census_import

     ! the census as the record file of write_cens (and path.keys),
     ! formatted on the device; n_written = the records written
     integer(c_int) function c2d_census_write(ctx, path, n_written) bind(C, name='c2d_census_write')
       import :: c_int, c_ptr, c_char, c_int64_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int64_t), intent(out) :: n_written
     end function c2d_census_write

     ! the same for n caller-supplied records in the layout of c2d_census_export
     integer(c_int) function c2d_census_write_from(ctx, d6, i5, keys, n, path) &
          bind(C, name='c2d_census_write_from')
       import :: c_int, c_ptr, c_char, c_double, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), intent(in) :: d6(6, *)
       integer(c_int32_t), intent(in) :: i5(5, *)
       integer(c_int64_t), intent(in) :: keys(*)
       integer(c_int64_t), value :: n
       character(kind=c_char), intent(in) :: path(*)
     end function c2d_census_write_from

     ! a census record file (read_cens) into the context's census, parsed
     ! and converted on the device; n = the records of the file
     integer(c_int) function c2d_census_read(ctx, path, n) bind(C, name='c2d_census_read')
       import :: c_int, c_ptr, c_char, c_int64_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int64_t), intent(out) :: n
     end function c2d_census_read

     ! parse only: the first min(cap, n) records to host arrays (c_loc of
     ! them, or c_null_ptr with cap = 0 to count); the census is untouched
     integer(c_int) function c2d_census_read_records(ctx, path, d6, i5, keys, cap, n) &
          bind(C, name='c2d_census_read_records')
       import :: c_int, c_ptr, c_char, c_int64_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       type(c_ptr), value :: d6, i5, keys
       integer(c_int64_t), value :: cap
       integer(c_int64_t), intent(out) :: n
     end function c2d_census_read_records

     integer(c_int) function c2d_last_census_file_ms(ctx, io_ms, wait_ms, kernel_ms, convert_ms, &
          device_records, host_records, chunks) bind(C, name='c2d_last_census_file_ms')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: io_ms, wait_ms, kernel_ms, convert_ms
       integer(c_int64_t), intent(out) :: device_records, host_records
       integer(c_int32_t), intent(out) :: chunks
     end function c2d_last_census_file_ms

     ! Binary checkpoints (include/compton2d.h "Checkpoints"): the census bit
     ! for bit, kappa_prev, the device electrons, the FP flags and `user`
     ! (c_loc of the host's own state, user_bytes of it).  Observer sums and
     ! the finished step's tallies and events are NOT in a checkpoint.
     integer(c_int) function c2d_checkpoint_write(ctx, path, user, user_bytes, n_written) &
          bind(C, name='c2d_checkpoint_write')
       import :: c_int, c_ptr, c_char, c_int64_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       type(c_ptr), value :: user
       integer(c_int64_t), value :: user_bytes
       integer(c_int64_t), intent(out) :: n_written
     end function c2d_checkpoint_write

     ! records [first, first + count) (count = -1: to the end); flags:
     ! C2D_CKPT_APPEND | C2D_CKPT_CENSUS_ONLY; user takes min(user_cap,
     ! user_bytes) bytes of the blob
     integer(c_int) function c2d_checkpoint_read(ctx, path, first, count, flags, user, user_cap, &
          user_bytes, n_records) bind(C, name='c2d_checkpoint_read')
       import :: c_int, c_ptr, c_char, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int64_t), value :: first, count
       integer(c_int32_t), value :: flags
       type(c_ptr), value :: user
       integer(c_int64_t), value :: user_cap
       integer(c_int64_t), intent(out) :: user_bytes, n_records
     end function c2d_checkpoint_read

     ! the header of a checkpoint; no context, no GPU
     integer(c_int) function c2d_checkpoint_info(path, info) bind(C, name='c2d_checkpoint_info')
       import :: c_int, c_char, c2d_ckpt_info
       character(kind=c_char), intent(in) :: path(*)
       type(c2d_ckpt_info), intent(out) :: info
     end function c2d_checkpoint_info

     integer(c_int) function c2d_last_checkpoint_ms(ctx, io_ms, wait_ms, kernel_ms, bytes, chunks) &
          bind(C, name='c2d_last_checkpoint_ms')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: io_ms, wait_ms, kernel_ms
       integer(c_int64_t), intent(out) :: bytes
       integer(c_int32_t), intent(out) :: chunks
     end function c2d_last_checkpoint_ms

     integer(c_int) function c2d_fp_set_config(ctx, fcfg) bind(C, name='c2d_fp_set_config')
       import :: c_int, c_ptr, c2d_fp_config
       type(c_ptr), value :: ctx
       type(c2d_fp_config), intent(in) :: fcfg
     end function c2d_fp_set_config

     ! C2D_FP_EXACT (default, bit for bit the reference order) | C2D_FP_FAST
     ! | C2D_FP_AUTO (per update: exact on the tea clamp, fast off it)
     integer(c_int) function c2d_fp_set_mode(ctx, mode) bind(C, name='c2d_fp_set_mode')
       import :: c_int, c_ptr, c_int32_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), value :: mode
     end function c2d_fp_set_mode

     integer(c_int) function c2d_last_fp_mode(ctx, mode) bind(C, name='c2d_last_fp_mode')
       import :: c_int, c_ptr, c_int32_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), intent(out) :: mode
     end function c2d_last_fp_mode

     integer(c_int) function c2d_fp_step(ctx, fin, fout) bind(C, name='c2d_fp_step')
       import :: c_int, c_ptr, c2d_fp_step_in, c2d_fp_step_out
       type(c_ptr), value :: ctx
       type(c2d_fp_step_in), intent(in) :: fin
       type(c2d_fp_step_out), intent(inout) :: fout
     end function c2d_fp_step

     integer(c_int) function c2d_volume_em(ctx, vin, vout) bind(C, name='c2d_volume_em')
       import :: c_int, c_ptr, c2d_vem_in, c2d_vem_out
       type(c_ptr), value :: ctx
       type(c2d_vem_in), intent(in) :: vin
       type(c2d_vem_out), intent(inout) :: vout
     end function c2d_volume_em

     integer(c_int) function c2d_obs_begin(ctx, bins) bind(C, name='c2d_obs_begin')
       import :: c_int, c_ptr, c2d_obs_bins
       type(c_ptr), value :: ctx
       type(c2d_obs_bins), intent(in) :: bins
     end function c2d_obs_begin

     integer(c_int) function c2d_obs_accumulate(ctx, events, n) bind(C, name='c2d_obs_accumulate')
       import :: c_int, c_ptr, c_int64_t
       type(c_ptr), value :: ctx, events           ! c_null_ptr: device events of the last step
       integer(c_int64_t), value :: n
     end function c2d_obs_accumulate

     integer(c_int) function c2d_obs_result(ctx, F, F2, cnt, kernel_ms) bind(C, name='c2d_obs_result')
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx, F, F2, cnt       ! [n_e, n_mu, n_t] in Fortran order
       real(c_double), intent(out) :: kernel_ms
     end function c2d_obs_result

     ! pspt's dialogue (one answer a line, C string) -> the SED binning
     integer(c_int) function c2d_obs_begin_pspt(ctx, deck) bind(C, name='c2d_obs_begin_pspt')
       import :: c_int, c_ptr, c_char
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: deck(*)   ! NUL-terminated
     end function c2d_obs_begin_pspt

     ! pspt's output file from the histogram so far (path NUL-terminated,
     ! empty = the deck's name); world_sum: summed over the communicator
     integer(c_int) function c2d_obs_write_pspt(ctx, path, factor, world_sum) &
          bind(C, name='c2d_obs_write_pspt')
       import :: c_int, c_ptr, c_char, c_int32_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int32_t), value :: factor, world_sum
     end function c2d_obs_write_pspt

     ! ---- Compton reflection (c2d_config%cr_sent 1..4) ----
     ! the tables of src/ref_matrix.f on the host: E_ref(500), P_ref(500,500),
     ! W_abs(500,500) in the reference's own COMMON layout (n_out, n_in)
     integer(c_int) function c2d_reflect_tables_host(E_ref, P_ref, W_abs) &
          bind(C, name='c2d_reflect_tables_host')
       import :: c_int, c_double
       real(c_double), intent(out) :: E_ref(*), P_ref(*), W_abs(*)
     end function c2d_reflect_tables_host

     ! ---- run setup (no context; the *_host calls use no GPU) ----
     ! gnt(200), E_field(400), E_ph(400) as the reference's setup builds them
     integer(c_int) function c2d_setup_grids(gnt, E_field, E_ph) bind(C, name='c2d_setup_grids')
       import :: c_int, c_double
       real(c_double), intent(out) :: gnt(*), E_field(*), E_ph(*)
     end function c2d_setup_grids

     ! IC_loss: s_i = 1, s_ph = num_nt fills COMMON F_IC(num_nt, nphfield) in place
     integer(c_int) function c2d_ic_loss(device, gnt, n_el, E_field, n_ph, F_IC, s_i, s_ph) &
          bind(C, name='c2d_ic_loss')
       import :: c_int, c_double, c_int64_t
       integer(c_int), value :: device, n_el, n_ph
       real(c_double), intent(in) :: gnt(*), E_field(*)
       real(c_double), intent(out) :: F_IC(*)
       integer(c_int64_t), value :: s_i, s_ph
     end function c2d_ic_loss

     ! libm /= 0: the C library's log (the reference's bits); 0: the GPU's bits
     integer(c_int) function c2d_ic_loss_host(gnt, n_el, E_field, n_ph, F_IC, s_i, s_ph, libm) &
          bind(C, name='c2d_ic_loss_host')
       import :: c_int, c_double, c_int64_t
       integer(c_int), value :: n_el, n_ph, libm
       real(c_double), intent(in) :: gnt(*), E_field(*)
       real(c_double), intent(out) :: F_IC(*)
       integer(c_int64_t), value :: s_i, s_ph
     end function c2d_ic_loss_host

     ! gam_min + P_nontherm of n zones; f_nt, Pnt are (200, n) in Fortran order
     integer(c_int) function c2d_setup_electrons(device, n, tea, amxwl, gmin, gmax, p_nth, gmin_out, &
          N_nth, gbar_nth, f_nt, Pnt) bind(C, name='c2d_setup_electrons')
       import :: c_int, c_double, c_int64_t
       integer(c_int), value :: device
       integer(c_int64_t), value :: n
       real(c_double), intent(in) :: tea(*), amxwl(*), gmin(*), gmax(*), p_nth(*)
       real(c_double), intent(out) :: gmin_out(*), N_nth(*), gbar_nth(*), f_nt(*), Pnt(*)
     end function c2d_setup_electrons

     integer(c_int) function c2d_setup_electrons_host(n, tea, amxwl, gmin, gmax, p_nth, gmin_out, &
          N_nth, gbar_nth, f_nt, Pnt, libm) bind(C, name='c2d_setup_electrons_host')
       import :: c_int, c_double, c_int64_t
       integer(c_int64_t), value :: n
       real(c_double), intent(in) :: tea(*), amxwl(*), gmin(*), gmax(*), p_nth(*)
       real(c_double), intent(out) :: gmin_out(*), N_nth(*), gbar_nth(*), f_nt(*), Pnt(*)
       integer(c_int), value :: libm
     end function c2d_setup_electrons_host

     ! the context's device copies (cr_sent 1..3)
     integer(c_int) function c2d_reflect_tables(ctx, E_ref, P_ref, W_abs) &
          bind(C, name='c2d_reflect_tables')
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: E_ref(*), P_ref(*), W_abs(*)
     end function c2d_reflect_tables

     ! the last step's Ed_ref(1:nr) and the specular, matrix and disk counts
     integer(c_int) function c2d_reflect_result(ctx, Ed_ref, counts, world_sum) &
          bind(C, name='c2d_reflect_result')
       import :: c_int, c_ptr, c_double, c_int64_t, c_int32_t
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: Ed_ref(*)
       integer(c_int64_t), intent(out) :: counts(3)
       integer(c_int32_t), value :: world_sum
     end function c2d_reflect_result

     ! diagnostics: the kernels' reflection functions on n packet states
     integer(c_int) function c2d_selftest_reflect(device, boundary, cr_sent, spec_switch, in, keys, n, &
          out, Ed_ref_sum) bind(C, name='c2d_selftest_reflect')
       import :: c_int, c_double, c_int64_t
       integer(c_int), value :: device, boundary, cr_sent, spec_switch
       real(c_double), intent(in) :: in(*)
       integer(c_int64_t), intent(in) :: keys(*)
       integer(c_int64_t), value :: n
       real(c_double), intent(out) :: out(*)
       real(c_double), intent(out) :: Ed_ref_sum
     end function c2d_selftest_reflect

     ! ---- observer sets: up to C2D_OBS_SET_MAX binnings filled in one pass
     !      over the escapes (several pspt SEDs and plcm light curves) ----
     integer(c_int) function c2d_obs_set_clear(ctx) bind(C, name='c2d_obs_set_clear')
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2d_obs_set_clear

     integer(c_int) function c2d_obs_set_add(ctx, bins, id) bind(C, name='c2d_obs_set_add')
       import :: c_int, c_ptr, c_int32_t, c2d_obs_bins
       type(c_ptr), value :: ctx
       type(c2d_obs_bins), intent(in) :: bins
       integer(c_int32_t), intent(out) :: id           ! the member's number, from 0
     end function c2d_obs_set_add

     ! pspt's / plcm's dialogue (one answer a line, NUL-terminated) -> a member
     integer(c_int) function c2d_obs_set_add_pspt(ctx, deck, id) bind(C, name='c2d_obs_set_add_pspt')
       import :: c_int, c_ptr, c_char, c_int32_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: deck(*)
       integer(c_int32_t), intent(out) :: id
     end function c2d_obs_set_add_pspt

     integer(c_int) function c2d_obs_set_add_plcm(ctx, deck, id) bind(C, name='c2d_obs_set_add_plcm')
       import :: c_int, c_ptr, c_char, c_int32_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: deck(*)
       integer(c_int32_t), intent(out) :: id
     end function c2d_obs_set_add_plcm

     integer(c_int) function c2d_obs_set_accumulate(ctx, events, n) bind(C, name='c2d_obs_set_accumulate')
       import :: c_int, c_ptr, c_int64_t
       type(c_ptr), value :: ctx, events           ! c_null_ptr: device events of the last step
       integer(c_int64_t), value :: n
     end function c2d_obs_set_accumulate

     integer(c_int) function c2d_obs_set_accumulate_device(ctx, d_events, n) &
          bind(C, name='c2d_obs_set_accumulate_device')
       import :: c_int, c_ptr, c_int64_t
       type(c_ptr), value :: ctx, d_events         ! device address of n events
       integer(c_int64_t), value :: n
     end function c2d_obs_set_accumulate_device

     integer(c_int) function c2d_obs_set_accumulate_file(ctx, path, n) &
          bind(C, name='c2d_obs_set_accumulate_file')
       import :: c_int, c_ptr, c_char, c_int64_t
       type(c_ptr), value :: ctx
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int64_t), intent(out) :: n
     end function c2d_obs_set_accumulate_file

     integer(c_int) function c2d_obs_set_shape(ctx, id, n_t, n_mu, n_e, lds_rows) &
          bind(C, name='c2d_obs_set_shape')
       import :: c_int, c_ptr, c_int32_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), value :: id
       integer(c_int32_t), intent(out) :: n_t, n_mu, n_e, lds_rows
     end function c2d_obs_set_shape

     integer(c_int) function c2d_obs_set_result(ctx, id, F, F2, cnt) bind(C, name='c2d_obs_set_result')
       import :: c_int, c_ptr, c_int32_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), value :: id
       type(c_ptr), value :: F, F2, cnt            ! [n_e, n_mu, n_t] in Fortran order
     end function c2d_obs_set_result

     integer(c_int) function c2d_obs_set_kernel_ms(ctx, ms, launches) bind(C, name='c2d_obs_set_kernel_ms')
       import :: c_int, c_ptr, c_double, c_int32_t
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: ms
       integer(c_int32_t), intent(out) :: launches
     end function c2d_obs_set_kernel_ms

     ! a deck member's files: path = pspt's output file, or the directory of
     ! plcm's files (NUL-terminated; empty = the deck's name / ".")
     integer(c_int) function c2d_obs_set_write(ctx, id, path, factor, world_sum) &
          bind(C, name='c2d_obs_set_write')
       import :: c_int, c_ptr, c_char, c_int32_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), value :: id
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int32_t), value :: factor, world_sum
     end function c2d_obs_set_write

     ! ---- exact observer sets: integer sums, the same bits in any order
     !      (compton2d.h "Exact observer sets"); a state is u64 words,
     !      integer(c_int64_t) here: 8 of head, then 5 per bin ----
     integer(c_int) function c2d_obs_set_exact(ctx, w_max) bind(C, name='c2d_obs_set_exact')
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), value :: w_max               ! bound on one event's rest-frame weight
     end function c2d_obs_set_exact

     integer(c_int) function c2d_obs_set_exact_info(ctx, id, e, n_rejected) &
          bind(C, name='c2d_obs_set_exact_info')
       import :: c_int, c_ptr, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), value :: id
       integer(c_int32_t), intent(out) :: e
       integer(c_int64_t), intent(out) :: n_rejected
     end function c2d_obs_set_exact_info

     integer(c_int) function c2d_obs_set_state_words(ctx, id, words) bind(C, name='c2d_obs_set_state_words')
       import :: c_int, c_ptr, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), value :: id
       integer(c_int64_t), intent(out) :: words
     end function c2d_obs_set_state_words

     integer(c_int) function c2d_obs_set_state(ctx, id, out, cap) bind(C, name='c2d_obs_set_state')
       import :: c_int, c_ptr, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), value :: id
       integer(c_int64_t), intent(out) :: out(*)
       integer(c_int64_t), value :: cap
     end function c2d_obs_set_state

     integer(c_int) function c2d_obs_set_merge(ctx, id, state, words) bind(C, name='c2d_obs_set_merge')
       import :: c_int, c_ptr, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), value :: id
       integer(c_int64_t), intent(in) :: state(*)
       integer(c_int64_t), value :: words
     end function c2d_obs_set_merge

     ! the host twin (no context, no GPU): n events added into `state`
     integer(c_int) function c2d_obs_exact_host(bins, w_max, events, n, state, cap) &
          bind(C, name='c2d_obs_exact_host')
       import :: c_int, c_ptr, c_double, c_int64_t, c2d_obs_bins
       type(c2d_obs_bins), intent(in) :: bins
       real(c_double), value :: w_max
       type(c_ptr), value :: events                  ! [7, n] f64
       integer(c_int64_t), value :: n
       integer(c_int64_t), intent(inout) :: state(*)
       integer(c_int64_t), value :: cap
     end function c2d_obs_exact_host

     integer(c_int) function c2d_obs_state_merge(into, into_words, from, from_words) &
          bind(C, name='c2d_obs_state_merge')
       import :: c_int, c_int64_t
       integer(c_int64_t), intent(inout) :: into(*)
       integer(c_int64_t), value :: into_words
       integer(c_int64_t), intent(in) :: from(*)
       integer(c_int64_t), value :: from_words
     end function c2d_obs_state_merge

     integer(c_int) function c2d_obs_state_result(state, words, F, F2, cnt) bind(C, name='c2d_obs_state_result')
       import :: c_int, c_ptr, c_int64_t
       integer(c_int64_t), intent(in) :: state(*)
       integer(c_int64_t), value :: words
       type(c_ptr), value :: F, F2, cnt            ! [n_e, n_mu, n_t] in Fortran order
     end function c2d_obs_state_result

     ! ---- RCCL tally all-reduce (replaces xec_add / graphics_collect,
     !      src/xec2d.f:325-399, and cens_add_up / E_add_up,
     !      src/update2d.f:1929-2078): rank 0 makes the id, the host
     !      broadcasts it (MPI_Bcast of C2D_COMM_ID_BYTES bytes) ----
     integer(c_int) function c2d_comm_unique_id(id, cap) bind(C, name='c2d_comm_unique_id')
       import :: c_int, c_int8_t, c_int64_t
       integer(c_int8_t), intent(out) :: id(*)
       integer(c_int64_t), value :: cap
     end function c2d_comm_unique_id

     integer(c_int) function c2d_comm_init(ctx, id, rank, world) bind(C, name='c2d_comm_init')
       import :: c_int, c_ptr, c_int8_t, c_int32_t
       type(c_ptr), value :: ctx
       integer(c_int8_t), intent(in) :: id(*)
       integer(c_int32_t), value :: rank, world
     end function c2d_comm_init

     integer(c_int) function c2d_allreduce_tallies(ctx) bind(C, name='c2d_allreduce_tallies')
       import :: c_int, c_ptr
       type(c_ptr), value :: ctx
     end function c2d_allreduce_tallies

     integer(c_int) function c2d_device_count(n) bind(C, name='c2d_device_count')
       import :: c_int, c_int32_t
       integer(c_int32_t), intent(out) :: n
     end function c2d_device_count

     integer(c_int) function c2d_electron_state(ctx, f_nt, Pnt) bind(C, name='c2d_electron_state')
       import :: c_int, c_ptr, c2d_marray3
       type(c_ptr), value :: ctx
       type(c2d_marray3), value :: f_nt, Pnt
     end function c2d_electron_state

     integer(c_int) function c2d_census_export_range(ctx, first, stride, d6, i5, keys, cap, n) &
          bind(C, name='c2d_census_export_range')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int64_t), value :: first, stride
       real(c_double), intent(out) :: d6(6, *)
       integer(c_int32_t), intent(out) :: i5(5, *)
       integer(c_int64_t), intent(out) :: keys(*)
       integer(c_int64_t), value :: cap
       integer(c_int64_t), intent(out) :: n
     end function c2d_census_export_range

     ! census population control (include/compton2d.h): per (cell, group)
     ! counts and ew sums, tables (ngroup, nr, nz) in Fortran order
     integer(c_int) function c2d_census_stats(ctx, group_of_sp, ngroup, count, energy) &
          bind(C, name='c2d_census_stats')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), intent(in) :: group_of_sp(0:*)
       integer(c_int32_t), value :: ngroup
       integer(c_int64_t), intent(out) :: count(*)
       real(c_double), intent(out) :: energy(*)
     end function c2d_census_stats

     integer(c_int) function c2d_last_census_stats_ms(ctx, ms) bind(C, name='c2d_last_census_stats_ms')
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: ctx
       real(c_double), intent(out) :: ms
     end function c2d_last_census_stats_ms

     ! weight-window roulette of the census against the floors w_min; salt is
     ! a 64-bit word (the step number)
     integer(c_int) function c2d_census_roulette(ctx, group_of_sp, ngroup, w_min, salt, res) &
          bind(C, name='c2d_census_roulette')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t, c2d_roulette_out
       type(c_ptr), value :: ctx
       integer(c_int32_t), intent(in) :: group_of_sp(0:*)
       integer(c_int32_t), value :: ngroup
       real(c_double), intent(in) :: w_min(*)
       integer(c_int64_t), value :: salt
       type(c2d_roulette_out), intent(out) :: res
     end function c2d_census_roulette

     ! the same rule on the host: no context, no GPU
     integer(c_int) function c2d_census_roulette_host(d6, i5, keys, n, nz, nr, group_of_sp, ngroup, &
          w_min, salt, keep, ew_out) bind(C, name='c2d_census_roulette_host')
       import :: c_int, c_double, c_int8_t, c_int32_t, c_int64_t
       real(c_double), intent(in) :: d6(6, *)
       integer(c_int32_t), intent(in) :: i5(5, *)
       integer(c_int64_t), intent(in) :: keys(*)
       integer(c_int64_t), value :: n
       integer(c_int32_t), value :: nz, nr
       integer(c_int32_t), intent(in) :: group_of_sp(0:*)
       integer(c_int32_t), value :: ngroup
       real(c_double), intent(in) :: w_min(*)
       integer(c_int64_t), value :: salt
       integer(c_int8_t), intent(out) :: keep(*)
       real(c_double), intent(out) :: ew_out(*)
     end function c2d_census_roulette_host

     ! census splitting against the ceilings w_max (ngroup, nr, nz) in Fortran
     ! order: a record heavier than its ceiling becomes up to max_copies
     ! records; flags = C2D_SPLIT_DRY only counts
     integer(c_int) function c2d_census_split(ctx, group_of_sp, ngroup, w_max, max_copies, salt, flags, res) &
          bind(C, name='c2d_census_split')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t, c2d_split_out
       type(c_ptr), value :: ctx
       integer(c_int32_t), intent(in) :: group_of_sp(0:*)
       integer(c_int32_t), value :: ngroup
       real(c_double), intent(in) :: w_max(*)
       integer(c_int32_t), value :: max_copies
       integer(c_int64_t), value :: salt
       integer(c_int32_t), value :: flags
       type(c2d_split_out), intent(out) :: res
     end function c2d_census_split

     ! the same rule on the host: no context, no GPU
     integer(c_int) function c2d_census_split_host(d6, i5, keys, n, nz, nr, group_of_sp, ngroup, &
          w_max, max_copies, salt, copies, ew_out) bind(C, name='c2d_census_split_host')
       import :: c_int, c_double, c_int32_t, c_int64_t
       real(c_double), intent(in) :: d6(6, *)
       integer(c_int32_t), intent(in) :: i5(5, *)
       integer(c_int64_t), intent(in) :: keys(*)
       integer(c_int64_t), value :: n
       integer(c_int32_t), value :: nz, nr
       integer(c_int32_t), intent(in) :: group_of_sp(0:*)
       integer(c_int32_t), value :: ngroup
       real(c_double), intent(in) :: w_max(*)
       integer(c_int32_t), value :: max_copies
       integer(c_int64_t), value :: salt
       integer(c_int32_t), intent(out) :: copies(*)
       real(c_double), intent(out) :: ew_out(*)
     end function c2d_census_split_host

     ! the keys of the copies 1..copies(k)-1 of every record, in that order
     integer(c_int) function c2d_census_split_keys_host(keys, copies, n, salt, keys_out) &
          bind(C, name='c2d_census_split_keys_host')
       import :: c_int, c_int32_t, c_int64_t
       integer(c_int64_t), intent(in) :: keys(*)
       integer(c_int32_t), intent(in) :: copies(*)
       integer(c_int64_t), value :: n
       integer(c_int64_t), value :: salt
       integer(c_int64_t), intent(out) :: keys_out(*)
     end function c2d_census_split_keys_host

     ! the census comb (include/compton2d.h): the digit histogram of the pool
     ! records' normalised critical values under `prefix` (prefix_bits = 0,
     ! 11, 22, 33, 44 or 55); norm (ngroup, nr, nz) in Fortran order, powers of two
     integer(c_int) function c2d_census_comb_hist(ctx, group_of_sp, ngroup, norm, salt, prefix, &
          prefix_bits, hist, res) bind(C, name='c2d_census_comb_hist')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t, c2d_comb_out
       type(c_ptr), value :: ctx
       integer(c_int32_t), intent(in) :: group_of_sp(0:*)
       integer(c_int32_t), value :: ngroup
       real(c_double), intent(in) :: norm(*)
       integer(c_int64_t), value :: salt, prefix
       integer(c_int32_t), value :: prefix_bits
       integer(c_int64_t), intent(out) :: hist(0:*)
       type(c2d_comb_out), intent(out) :: res
     end function c2d_census_comb_hist

     ! those records' values to crit_host (at most cap); n = their full number
     integer(c_int) function c2d_census_comb_collect(ctx, group_of_sp, ngroup, norm, salt, prefix, &
          prefix_bits, crit_host, cap, n) bind(C, name='c2d_census_comb_collect')
       import :: c_int, c_ptr, c_double, c_int32_t, c_int64_t
       type(c_ptr), value :: ctx
       integer(c_int32_t), intent(in) :: group_of_sp(0:*)
       integer(c_int32_t), value :: ngroup
       real(c_double), intent(in) :: norm(*)
       integer(c_int64_t), value :: salt, prefix
       integer(c_int32_t), value :: prefix_bits
       real(c_double), intent(out) :: crit_host(*)
       integer(c_int64_t), value :: cap
       integer(c_int64_t), intent(out) :: n
     end function c2d_census_comb_collect

     ! the same values on the host: no context, no GPU
     integer(c_int) function c2d_census_comb_host(d6, i5, keys, n, nz, nr, group_of_sp, ngroup, &
          norm, salt, crit, fixed) bind(C, name='c2d_census_comb_host')
       import :: c_int, c_double, c_int8_t, c_int32_t, c_int64_t
       real(c_double), intent(in) :: d6(6, *)
       integer(c_int32_t), intent(in) :: i5(5, *)
       integer(c_int64_t), intent(in) :: keys(*)
       integer(c_int64_t), value :: n
       integer(c_int32_t), value :: nz, nr
       integer(c_int32_t), intent(in) :: group_of_sp(0:*)
       integer(c_int32_t), value :: ngroup
       real(c_double), intent(in) :: norm(*)
       integer(c_int64_t), value :: salt
       real(c_double), intent(out) :: crit(*)
       integer(c_int8_t), intent(out) :: fixed(*)
     end function c2d_census_comb_host
  end interface
end module compton2d
