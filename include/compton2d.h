/*
 * compton2d.h — C-ABI of the MI355X-native Compton2d IMC engine.
 *
 * Drop-in boundary for the reference's per-step transport entry points
 * (all argument-less Fortran subroutines that talk through COMMON blocks):
 *
 *   reference entry point                         replaced by
 *   -------------------------------------------   --------------------------------------
 *   src/imcfield2d.f:5   imcfield2d (census)       c2d_transport_step  (census phase)
 *   src/imcvol2d_para.f:1 imcvol2d (volume src)    c2d_transport_step  (volume phase)
 *   src/imcsurf2d_para.f:1 imcsurf2d (surface src) c2d_transport_step  (surface phase)
 *   src/imcredist.f:5    imcredist (census bal.)   not needed: census stays on its GPU
 *   src/xec2d.f:325/371  xec_add/graphics_collect  c2d_tally_device_ptr + one all-reduce
 *   src/update2d.f:1929  cens_add_up (REDUCE)      c2d_tally_device_ptr + one all-reduce
 *   src/imcleak2d.f:171  event-file writes         c2d_events, c2d_events_write
 *   src/imcleak2d.f:104-165, :197-275 Compton      c2d_config.cr_sent (inside c2d_transport_step),
 *     reflection; src/ref_matrix.f Pref_calc,      c2d_reflect_tables_host / c2d_reflect_tables,
 *     Wref_calc (setup2d.f:40-41); Ed_ref          c2d_reflect_result
 *   postprocessing/pspt.c:245  event-file reads     c2d_events_read, c2d_obs_accumulate_file
 *   src/census2d.f:1-76  write_cens/read_cens      c2d_census_write / c2d_census_read (the files),
 *                                                  c2d_census_export / c2d_census_import (arrays)
 *   src/update2d.f:7     update (FP_calc, tridag,  c2d_fp_set_config + c2d_fp_step
 *     E_add_up, FP_send_job/recv_result)
 *
 * Every array argument is (pointer, strides) so Fortran COMMON arrays with
 * their fixed leading extents (general.pa: n_vol=400, jmax=kmax=99,
 * num_nt=200) are passed without copies; the library gathers only the
 * [1:nz,1:nr] sub-block.  Indices below are 0-based: element (i,j,k) of a
 * c2d_array3 lives at data[i*s_i + j*s_j + k*s_k] with j=0..nz-1 (z zone),
 * k=0..nr-1 (r zone).  For kappa_tot(n_vol,jmax,kmax) pass s_i=1,
 * s_j=n_vol, s_k=n_vol*jmax; for f_nt(jmax,kmax,num_nt) pass s_j=1,
 * s_k=jmax, s_i=jmax*kmax.
 *
 * Errors: every call returns 0 or a negative C2D_E_* code; the message is
 * in c2d_last_error().  Nothing calls exit() (the reference `stop`s at
 * src/imctrk2d.f:573-577, src/imcfield2d.f:84-87).
 * Threading: all calls on one context from one host thread; calls are
 * synchronous on return unless documented otherwise.
 */
#ifndef COMPTON2D_H
#define COMPTON2D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Compile-time extents of the reference (src/general.pa:7-30). */
#define C2D_N_VOL     400   /* photon energy grid of kappa_tot/eps_tot (n_vol)  */
#define C2D_NUM_NT    200   /* electron Lorentz-factor grid (num_nt)            */
#define C2D_NPHFIELD  400   /* internal photon-field grid n_field (nphfield)    */
#define C2D_NPHOMAX   128   /* spectrum bins (nphomax)                          */
#define C2D_NPHLCMAX  10    /* light-curve bands (nphlcmax)                     */
#define C2D_NMUMAX    32    /* angular bins (nmumax)                            */
#define C2D_NFMAX     500   /* external seed spectrum table (nfmax)             */
#define C2D_MAXZONE   99    /* jmax = kmax                                      */

/* Error codes. */
#define C2D_OK                  0
#define C2D_E_ARG              -1   /* bad argument / unsupported option          */
#define C2D_E_HIP              -2   /* HIP runtime error                          */
#define C2D_E_CENSUS_OVERFLOW  -3   /* replaces `stop 'too many photons'`         */
#define C2D_E_EVENT_OVERFLOW   -4   /* escape-event buffer full                   */
#define C2D_E_QUEUE_OVERFLOW   -5   /* scatter-secondary queue full               */
#define C2D_E_NOMEM            -6
#define C2D_E_STATE            -7   /* call order violated                        */
#define C2D_E_FP               -8   /* FP sub-step limit (reference `stop`,
                                       src/update2d.f:585-599), a solver guard,
                                       or NaN/Inf in n_field, ecens or the
                                       updated electron state                     */
#define C2D_E_RCCL             -9   /* RCCL (communicator / all-reduce) error     */
#define C2D_E_IO              -10   /* a file could not be written or read        */
#define C2D_E_NONFINITE       -11   /* NaN/Inf in a table, a tally or an emission
                                       output (the reference would carry it on:
                                       NaN counts, a collapsed run)               */

/* comtot (src/comtot2d.f:1-334, icoms=6) evaluation mode. */
#define C2D_COMTOT_EXACT  0   /* 199-term electron-spectrum sum per call (reference)   */
#define C2D_COMTOT_TABLE  1   /* per-cell cubic table in log(xnu), rebuilt every step  */

/* c2d_config.trk_variant: which snapshot of the reference's tracker
 * (SURVEY.md §8 hazard H1).  C2D_TRK_SRC (default) is src/imctrk2d.f, bug
 * for bug: the azimuth update uses the 3-D path, Eta = (trld + Eta*rpre)/rnew
 * (:472), a fresh colmfp after every cell boundary (`go to 100`, :518-525),
 * the clamps |wmu| <= 0.99999999 and |Eta| <= 0.999999999 (:161-162,
 * :243-244, :474-476; imcfield2d.f:119-120).  C2D_TRK_2012_11 is
 * src_20121113/imctrk2d.f: Eta = (f + Eta*rpre)/rnew with f the path's
 * projection on the r-plane (:477-479), colmfp kept across boundaries
 * (`go to 110` with colmfp -= sigsc*trld, :505, :526-533; sigabs reset
 * after 110, :159), no idead = 4 re-entry (:521-524), and |wmu|, |Eta|
 * clamped to 1 (:162-167, :481-484; imcfield2d.f:119-124). */
#define C2D_TRK_SRC       0
#define C2D_TRK_2012_11   1

typedef struct c2d_array3 { const double* data; int64_t s_i, s_j, s_k; } c2d_array3;
typedef struct c2d_array2 { const double* data; int64_t s_j, s_k; } c2d_array2;
typedef struct c2d_iarray2 { const int32_t* data; int64_t s_j, s_k; } c2d_iarray2;

/* Seed spectrum for a surface with tbb <= 0: the normalised table that
 * file_sp (src/imcsurf2d_para.f:544-685, host-side) leaves in COMMON /insp/
 * and file_sample (:694-788) draws from. */
typedef struct c2d_spectrum {
  int32_t nfile;
  const double* E_file;   /* [nfile]   */
  const double* a1;       /* [nfile-1] */
  const double* I_file;   /* [nfile-1] */
  const double* F_file;   /* [nfile]   */
  const double* P_file;   /* [nfile-1] cumulative, normalised */
} c2d_spectrum;

/* Run-constant set-up (src/setup2d.f:47-222, src/reader.f). */
typedef struct c2d_config {
  int32_t nz, nr;                 /* zones (reference nz, nr <= 99)           */
  double  rmin, zmin;             /* inner radius, lower z (zmin = 0 in ref)  */
  const double* z;                /* [nz] upper z boundary of zone j          */
  const double* r;                /* [nr] outer r boundary of zone k          */
  const double* E_ph;             /* [C2D_N_VOL] energy grid of kappa/eps     */
  const double* E_field;          /* [C2D_NPHFIELD] grid of n_field           */
  const double* gnt;              /* [C2D_NUM_NT] gamma-1 grid                */
  int32_t nphtotal;               /* spectrum bins; hu has nphtotal+1 edges   */
  const double* hu;
  int32_t nph_lc;                 /* light-curve bands                        */
  const double* Elcmin;
  const double* Elcmax;
  int32_t nmu;                    /* angular bins                             */
  const double* mu;               /* [nmu] upper bin edges                    */
  int32_t split1, split2, split3, spl3_trg;  /* variance reduction (COMMON /split/) */
  int32_t spec_switch;            /* 0: escaping spectrum into fout            */
  /* Compton reflection (imcleak2d.f:104-165, :197-275):
   *   0  none: every packet at a system boundary leaves
   *   1  lower boundary: a ring with tbbl > 0 reflects through the matrices
   *      P_ref / W_abs (new energy and weight, Ed_ref += the new weight,
   *      wmu = |wmu|), a ring with tbbl <= 0 specularly (wmu = -wmu)
   *   2  outer r-boundary: a packet with wmu <= 0 is reflected by the disk
   *      (matrices, zpre = 0, wmu uniform in (0,1)) and leaves with its new
   *      values; it counts as an escape and writes an event
   *   3  both 1 and 2
   *   4  lower boundary, always specular; needs no tables
   * Probe copies never reflect.  spec_switch = 1 adds the specular branch's
   * fout line (the spectrum incident on the boundary).  With cr_sent != 0
   * the bundle kernel's per-wave escape queue stays off (the inline path): a
   * reflection draws from the packet's stream and queue entries carry no
   * stream position. */
  int32_t cr_sent;
  int32_t pair_switch;            /* gamma-gamma; inert in the MPI reference (H6) */
  int32_t kappa_lag;              /* 1: census+volume use previous step's kappa_tot (H3) */
  int32_t comtot_mode;            /* C2D_COMTOT_EXACT | C2D_COMTOT_TABLE       */
  int32_t device;                 /* HIP device ordinal                        */
  uint64_t seed;                  /* lineage RNG seed (replaces rseed)        */
  int32_t rank, world;            /* source sharding: this context tracks sources with
                                     (global source index % world) == rank       */
  int64_t census_capacity;        /* packets (per context)                     */
  int64_t event_capacity;         /* escape events per step, >= C2D_EV_SHARDS (32): the
                                     buffer is 32 equal shards, workgroup b appends to
                                     shard b % 32, and a full shard is an overflow     */
  int64_t queue_capacity;         /* scatter records per generation            */
  int32_t census_inplace;         /* 0: census double-buffered (in + out, 128 B per
                                     record, the reference's dbufin/dbufout); 1: one
                                     chunked SoA (64 B per record + 1/16 slack: a
                                     step refills the 1024-record chunks its census
                                     sources have finished with)     */
  int32_t trk_variant;            /* C2D_TRK_SRC (0, default) | C2D_TRK_2012_11    */
} c2d_config;

/* Per-step inputs (what imcgen2d/volume_em/file_sp leave in COMMON). */
typedef struct c2d_step_in {
  int32_t ncycle;                 /* step counter (events only for ncycle > 0) */
  double  time, dt;               /* time, dt(1)                              */
  c2d_array3 kappa_tot;           /* (i<400, j, k) absorption [1/cm]          */
  c2d_array3 eps_tot;             /* (i<400, j, k) volume emission CDF        */
  c2d_array3 eps_th;              /* (i<400, j, k) thermal-surface CDF        */
  c2d_array3 f_nt;                /* (i<200, j, k) electron spectrum          */
  c2d_array3 Pnt;                 /* (i<200, j, k) electron CDF               */
  c2d_array2 n_e;                 /* electron density                         */
  c2d_array2 Eloss_th, Eloss_tot; /* thermal / total emitted energy           */
  c2d_array2 zsurf;               /* zone surface area                        */
  c2d_array2 ewsv;                /* volume packet weight                     */
  c2d_iarray2 nsv;                /* volume packets per zone                  */
  const int32_t* nsurfi; const int32_t* nsurfo;  /* [nz] inner/outer z-surface packets */
  const double*  ewsurfi; const double*  ewsurfo; /* [nz] weights                       */
  const int32_t* nsurfu; const int32_t* nsurfl;  /* [nr] upper/lower r-surface packets */
  const double*  ewsurfu; const double*  ewsurfl; /* [nr]                                */
  const double*  tbbi; const double* tbbo;        /* [nz] boundary temps at time index ti */
  const double*  tbbu; const double* tbbl;        /* [nr]                                 */
  const int32_t* spec_i; const int32_t* spec_o;   /* [nz] spectrum index for tbb<=0       */
  const int32_t* spec_u; const int32_t* spec_l;   /* [nr]                                  */
  int32_t n_spectra;
  const c2d_spectrum* spectra;
  int32_t device_tables;          /* C2D_DEV_* flags: tables already on the device  */
} c2d_step_in;

/* c2d_step_in.device_tables: take tables from the device instead of the
 * host views (which may then be NULL), so a coupled MC step
 *   c2d_volume_em -> c2d_set_step -> c2d_run_step -> c2d_fp_step
 * moves only zone scalars through the host (imcgen2d -> transport -> update,
 * src/xec2d.f:67-87, with no table re-gathering per step). */
#define C2D_DEV_EMISSION   1   /* kappa_tot, eps_tot, eps_th = last c2d_volume_em  */
#define C2D_DEV_ELECTRONS  2   /* f_nt, Pnt = the context's electron state (last
                                  c2d_set_step upload, updated in place by a
                                  c2d_fp_step called with NULL f_nt/Pnt views)    */

/* Fused per-step tally buffer (f64).  One all-reduce over this buffer
 * replaces xec_add, graphics_collect, cens_add_up and E_add_up's scalar
 * MPI_REDUCE loops.  Offsets are in doubles. */
typedef struct c2d_tally_layout {
  int64_t edep, prdep, ecens, npcen;  /* [ncell] each, cell = j*nr + k        */
  int64_t n_field;                    /* [ncell][C2D_NPHFIELD]                */
  int64_t E_IC, nelectron;            /* [C2D_NUM_NT+2] (reference index i)   */
  int64_t fout;                       /* [nmu][C2D_NPHOMAX]: fout(mu,jgpsp)   */
  int64_t edout;                      /* [nmu][C2D_NPHLCMAX]                  */
  int64_t erlki, erlko;               /* [nz]                                 */
  int64_t erlku, erlkl, Ed_in;        /* [nr]                                 */
  int64_t counters;                   /* [C2D_NCOUNTERS]                      */
  int64_t total;
} c2d_tally_layout;

/* counters[] entries (exact integers stored as f64). */
#define C2D_CNT_STEPS      0   /* packet-steps: passes through imctrk2d.f:228-485 */
#define C2D_CNT_ESCAPES    1   /* packets leaving the system (imcleak)           */
#define C2D_CNT_CENSUS     2   /* packets written to census                       */
#define C2D_CNT_COLLIDE    3   /* Compton collisions (ikind=3)                    */
#define C2D_CNT_KILLED     4   /* weight kills (ewnew <= wtmin)                   */
#define C2D_CNT_SOURCES    5   /* source packets started (census+volume+surface)  */
#define C2D_CNT_COMPB      6   /* compb2d calls                                    */
#define C2D_CNT_EVENTS     7   /* event-file records written                      */
#define C2D_CNT_GENS       8   /* scatter generations launched                    */
#define C2D_CNT_ABORTED    9   /* packets stopped by a safety cap (must stay 0)   */
#define C2D_CNT_ESC_SCAT  11   /* escapes of scattered packets (imctrk2d(1) copies) */
#define C2D_NCOUNTERS      16

static inline void c2d_tally_layout_for(int32_t nz, int32_t nr, int32_t nmu,
                                        c2d_tally_layout* L) {
  int64_t nc = (int64_t)nz * nr, o = 0;
  L->edep = o; o += nc;
  L->prdep = o; o += nc;
  L->ecens = o; o += nc;
  L->npcen = o; o += nc;
  L->n_field = o; o += nc * C2D_NPHFIELD;
  L->E_IC = o; o += C2D_NUM_NT + 2;
  L->nelectron = o; o += C2D_NUM_NT + 2;
  L->fout = o; o += (int64_t)nmu * C2D_NPHOMAX;
  L->edout = o; o += (int64_t)nmu * C2D_NPHLCMAX;
  L->erlki = o; o += nz;
  L->erlko = o; o += nz;
  L->erlku = o; o += nr;
  L->erlkl = o; o += nr;
  L->Ed_in = o; o += nr;
  L->counters = o; o += C2D_NCOUNTERS;
  L->total = o;
}

/* Escape event = one line of p###_evb.dat (src/imcleak2d.f:171,181):
 * t_bound, xnu [keV], ew [erg], rpre, zpre [cm], wmu, phi. */
#define C2D_EVENT_WORDS 7

/* Census record (src/imctrk2d.f:558-572; census2d.f 6e14.7 / 6i5):
 * d6 = rpre, zpre, wmu, phi, ew, xnu; i5 = jgpsp, jgplc, jgpmu, jph, kph
 * (1-based as in the reference); key = lineage RNG key (replaces the
 * per-packet fibran seed, hazard H5). */

typedef struct c2d_ctx c2d_ctx;

/* Fokker-Planck per-zone solve (src/update2d.f:337-1739, tridag :2476-2518). */
typedef struct c2d_fp_in {
  int32_t ncell;                  /* zones solved in this call                  */
  const double* a;                /* [ncell][nt] sub-diagonal                   */
  const double* b;                /* [ncell][nt] diagonal                       */
  const double* c;                /* [ncell][nt] super-diagonal                 */
  const double* r;                /* [ncell][nt] right-hand side                */
  int32_t nt;                     /* unknowns per zone (num_nt-1 = 199 in ref)  */
} c2d_fp_in;

/* ------------------------------------------------------------------------
 * Fokker-Planck electron update of one MC step (src/update2d.f:7-327
 * `update` + :337-1739 `FP_calc` for every zone, tridag :2476-2518).
 * Mutable (pointer, strides) views bind the caller's COMMON arrays, which
 * are updated in place exactly where the reference's FP_recv_result /
 * update write them (src/fp_mpi.f:972-1003, src/update2d.f:266-276).
 * ---------------------------------------------------------------------- */
typedef struct c2d_marray3 { double* data; int64_t s_i, s_j, s_k; } c2d_marray3;
typedef struct c2d_marray2 { double* data; int64_t s_j, s_k; } c2d_marray2;

/* Run constants of FP_calc (src/reader.f:512-559, broadcast once by
 * setup_bcast src/fp_mpi.f:12-324; df_implicit/df_T general.pa:27-28;
 * F_IC from IC_loss src/icloss2d.f:1-64, broadcast by FP_bcast
 * src/fp_mpi.f:596). */
typedef struct c2d_fp_config {
  int32_t pair_switch;            /* 0/1; 1 = inert positrons (H6), f_pair = 0  */
  double  df_implicit, df_T;      /* 1e-2, 0.25 in the reference               */
  double  r_esc, r_acc;           /* escape / acceleration time [z(nz)/c]      */
  int32_t cf_sentinel;            /* coronal flare on/off                      */
  double  r_flare, z_flare, t_flare, sigma_r, sigma_z, sigma_t, flare_amp;
  int32_t inj_switch, inj_dis, g2var_switch, pick_sw;
  double  inj_g1, inj_g2, inj_p, inj_t, inj_L, pick_rate, inj_gg, inj_sigma;
  double  inj_v;                  /* sqrt(1-1/g_bulk**2)*c_light (reader.f:559) */
  const double* F_IC;             /* F_IC(i<num_nt, i_ph<nphfield)             */
  int64_t F_IC_s_i, F_IC_s_ph;    /* Fortran F_IC(200,400): s_i=1, s_ph=200    */
} c2d_fp_config;

/* Per-step inputs of `update` (what FP_send_job packs, src/fp_mpi.f:632-686). */
typedef struct c2d_fp_step_in {
  int32_t ncycle;                 /* photon_fill (ncycle <= 1) sets dT_max=df_T */
  double time, dt;                /* time, dt(1)                               */
  c2d_array2 tea, tna, n_e, B_field, Eloss_sy, ec_old, turb_lev, vol;
  c2d_array2 f_pair;              /* NULL data = 0                             */
  c2d_array2 ecens;               /* NULL data: the context's tally buffer     */
  c2d_array3 n_field;             /* (i_ph, j, k); NULL data: tally buffer     */
} c2d_fp_step_in;

/* Per-zone diagnostics (optional output, [ncell][C2D_FP_NDIAG]). */
#define C2D_FP_E_OLD    0   /* zone's share of E_tot_old                       */
#define C2D_FP_E_NEW    1   /* zone's share of E_tot_new                       */
#define C2D_FP_HR       2   /* zone's share of hr_total                        */
#define C2D_FP_HR_ST    3   /* zone's share of hr_st_total                     */
#define C2D_FP_DELTA_T  4   /* |Te_new - tea| / Te_new                         */
#define C2D_FP_STEPS    5   /* implicit FP sub-steps taken                     */
#define C2D_FP_SKIPPED  6   /* 1: n_lept < 1e-11, zone left untouched          */
#define C2D_FP_NDIAG    8

/* In/out state.  f_nt, Pnt, n_e, gmin, gmax, amxwl, p_nth and tea are read
 * and updated in place; Te_new is written.  Views with NULL data are
 * skipped (tea: the update2d.f:266-276 clamp is then left to the caller).
 * f_nt and Pnt both NULL: the context's device electron state is read and
 * updated in place (C2D_DEV_ELECTRONS) and nothing 200-bin crosses the host. */
typedef struct c2d_fp_step_out {
  c2d_marray3 f_nt, Pnt;          /* (i<num_nt, j, k)                          */
  c2d_marray2 Te_new, tea, n_e, gmin, gmax, amxwl, p_nth;
  double* zone_diag;              /* optional [ncell][C2D_FP_NDIAG], cell=j*nr+k */
  double  E_tot_old, E_tot_new, hr_total, hr_st_total, dT_max;  /* E_add_up */
} c2d_fp_step_out;

/* ------------------------------------------------------------------------
 * Per-step emission / absorption tables (replaces the per-cell loop of
 * imcgen2d, src/imcgen2d.f:209-333, with volume_em, src/volume2d.f:10-394):
 * B from ep_switch, l_min, volume_em (kappa_tot = kappa_sy, eps_tot, eps_th,
 * Eloss_cy, Eloss_th), Eloss_sy from f_nt, and the dt*vol / dt*zsurf scaling.
 * Pair annihilation is inert (volume2d.f:322 skips it for f_pair < 1e-10; with
 * pair_switch = 1 a larger f_pair is C2D_E_ARG, hazard H6).
 * ---------------------------------------------------------------------- */
typedef struct c2d_vem_in {
  double dt;                                         /* dt(1)                     */
  c2d_array2 tea, tna, n_e, B_field, f_pair, zsurf, vol;
  c2d_iarray2 ep_switch;                             /* null data: all 0          */
  c2d_array3 f_nt;                                   /* (e-bin, j, k) like Pnt;
                                                        null data: the context's
                                                        device electron state   */
} c2d_vem_in;

typedef struct c2d_vem_out {                         /* any data may be NULL      */
  c2d_marray3 kappa_tot, eps_tot, eps_th;            /* (energy, j, k)            */
  c2d_marray2 B_field, Eloss_sy, Eloss_cy, Eloss_th, Eloss_tot;
  double* E_ph;                                      /* [C2D_N_VOL] photon grid   */
} c2d_vem_out;

/* ------------------------------------------------------------------------
 * Observer-frame binning of escape events on the device (replaces running
 * postprocessing/pspt.c:245-322 and plcm.c:382-456 over p###_evb.dat).
 * Bin edges are explicit arrays so each tool's own edge arithmetic is kept
 * (pspt: t0[n] = t0[0] + n*dt; plcm: t1[k] = t0[k+1] = t0[k] + dt).
 * ---------------------------------------------------------------------- */
#define C2D_OBS_SED 0   /* pspt.c: one closed mu window [mu0,mu1], first energy bin  */
#define C2D_OBS_LC  1   /* plcm.c: time - t_offset >= 0, half-open mu bins, every
                           energy band containing E                                 */
#define C2D_OBS_MAX_T   1024
#define C2D_OBS_MAX_MU  32
#define C2D_OBS_MAX_E   256

typedef struct c2d_obs_bins {
  int32_t mode;                   /* C2D_OBS_SED | C2D_OBS_LC                  */
  double  gam_bulk, rmax;         /* bulk Lorentz factor, r_max [cm]           */
  double  t_offset;               /* LC only                                   */
  int32_t n_t;  const double* t0; const double* t1;    /* observer time bins [s] */
  int32_t n_mu; const double* mu0; const double* mu1;  /* observer-frame cos   */
  int32_t n_e;  const double* E0; const double* E1;    /* observer energy [keV] */
} c2d_obs_bins;

const char* c2d_version(void);
int  c2d_init(const c2d_config* cfg, c2d_ctx** out);
void c2d_finalize(c2d_ctx* ctx);
const char* c2d_last_error(c2d_ctx* ctx);

/* One MC time step: census + volume + surface transport, all scatter
 * generations, tallies into the fused device buffer.  Synchronous.
 * Equivalent to c2d_set_step followed by c2d_run_step. */
int  c2d_transport_step(c2d_ctx* ctx, const c2d_step_in* in);

/* Upload the per-step tables (what imcgen2d/volume_em/file_sp produce) and
 * the clock; rebuilds the comtot table in C2D_COMTOT_TABLE mode. */
int  c2d_set_step(c2d_ctx* ctx, const c2d_step_in* in);
/* Advance the clock only (tables unchanged, e.g. T_const=1 runs). */
int  c2d_set_clock(c2d_ctx* ctx, int32_t ncycle, double time, double dt);
/* Transport with the tables of the last c2d_set_step.
 * On failure the double-buffered census (census_inplace = 0) is left as it
 * was.  The chunked census (census_inplace = 1) is rewritten in place once
 * generation 0 runs, so a failure after that LOSES it: c2d_census_count
 * then reports 0, and the census export/pack/append calls and the next
 * c2d_run_step return C2D_E_STATE until c2d_census_import or
 * c2d_census_truncate starts a new census. */
int  c2d_run_step(c2d_ctx* ctx);
/* Use caller-owned device memory (>= layout.total doubles on the context's
 * device) as the fused tally buffer, e.g. a torch tensor that is then
 * all-reduced over RCCL in place.  NULL restores the internal buffer. */
int  c2d_set_tally_buffer(c2d_ctx* ctx, double* device_ptr);

int  c2d_tally_layout_get(c2d_ctx* ctx, c2d_tally_layout* out);
/* Device pointer of the fused tally buffer (layout above), valid until the
 * next step; callers may all-reduce it in place (RCCL) before reading. */
double* c2d_tally_device_ptr(c2d_ctx* ctx);
/* Copy the fused tally buffer to host memory (total doubles). */
int  c2d_tally_download(c2d_ctx* ctx, double* host, int64_t n);
/* Copy tally words [offset, offset + n) of the fused buffer to host memory
 * (e.g. one tally and the counters, instead of the whole buffer per step). */
int  c2d_tally_download_range(c2d_ctx* ctx, double* host, int64_t offset, int64_t n);

/* Escape events of the last step: copies min(cap, n) records. */
int  c2d_events(c2d_ctx* ctx, double* buf, int64_t cap, int64_t* n);
/* The last step's escape events as p###_evb.dat text (imcleak2d.f:181),
 * formatted on the device; append != 0 adds to an existing file as the
 * reference's per-step writes do.  *n_written = records written (n_written
 * may be NULL).  The events are those of c2d_events, in its order; the call
 * returns when the file is complete and closed, waits for an asynchronous
 * observer pass over the same events and changes neither the event buffer
 * nor the observer state.  Errors: C2D_E_STATE before the first step;
 * C2D_E_IO if the file cannot be opened or written; C2D_E_NONFINITE if an
 * event holds a NaN or Inf (the message names the first such record): the
 * events are scanned before the file is opened, so the file is then exactly
 * as it was.  No events: an empty file (append == 0) or an untouched one.
 * The text is staged in chunks of C2D_EVTEXT_CHUNK events (environment, read
 * at every call; default 1048576) through two pinned host buffers: memory is
 * bounded by the chunk, not by the event count. */
int  c2d_events_write(c2d_ctx* ctx, const char* path, int32_t append, int64_t* n_written);
/* The same for n caller-supplied events (7 f64 each), on the host or
 * (on_device != 0) in device memory on this context's GPU. */
int  c2d_events_write_from(c2d_ctx* ctx, const double* events, int64_t n, int32_t on_device,
                           const char* path, int32_t append);
/* Diagnostics of the last c2d_events_write*: milliseconds of the non-finite
 * scan and of the formatting kernels (device time), host time spent waiting
 * for chunks and in fwrite, the values the kernel's fast path could not
 * decide (exact ties, round values), those of them that went through the
 * multi-limb path, and the chunk count.  Any pointer may be NULL. */
int  c2d_last_events_write_ms(c2d_ctx* ctx, double* scan_ms, double* kernel_ms, double* wait_ms,
                              double* io_ms, int64_t* ambiguous, int64_t* multilimb, int32_t* chunks);
/* The inverse: the text of an event file back to events (7 f64 a record),
 * parsed on the device.  Stores the first min(cap, *n) records at buf, in
 * host memory or (on_device != 0) in device memory on this context's GPU;
 * *n = the records of the file; buf == NULL with cap == 0 only counts.
 * Canonical records (105 bytes: seven right-justified 14-byte fields
 * [ -]0.dddddddE[+-]dd or [ -]0.ddddddd[+-]ddd, one blank between them, a
 * newline at the end) are parsed by a kernel, each field to the double
 * nearest to its value, ties to even: the bits of strtod of the field (the
 * E-less three-digit-exponent form, which fscanf("%lf") would split in two,
 * is read as the number that was written).  From the first record that is not
 * canonical to the end of the file, and for a tail shorter than a record, a
 * host parser takes over: blank-separated tokens (canonical fields, else
 * strtod of the whole token: free format, CRLF, NaN and Infinity), grouped in
 * sevens, a trailing group of fewer dropped.  A token neither accepts gives
 * C2D_E_IO with its byte offset in the message; the records before it have
 * been delivered and *n counts them (the file is streamed in chunks of
 * C2D_EVTEXT_CHUNK events through two pinned buffers, not validated first:
 * memory is bounded by the chunk, not by the file).  C2D_E_IO also if the
 * file cannot be opened or read; an empty file is 0 records. */
int  c2d_events_read(c2d_ctx* ctx, const char* path, double* buf, int64_t cap, int32_t on_device, int64_t* n);
/* Diagnostics of the last c2d_events_read / c2d_obs_accumulate_file /
 * c2d_obs_set_accumulate_file: host milliseconds in read(), waiting for a
 * chunk's copy and parse kernel, device milliseconds of the parse kernels,
 * host milliseconds of the host parser; records parsed on the device and on
 * the host, fields the device decided by the multi-limb path, device chunks.
 * Any pointer may be NULL. */
int  c2d_last_events_read_ms(c2d_ctx* ctx, double* io_ms, double* wait_ms, double* kernel_ms,
                             double* host_parse_ms, int64_t* canonical, int64_t* host_parsed,
                             int64_t* exact_fields, int32_t* chunks);

/* Census held on the device for the next step. */
int  c2d_census_count(c2d_ctx* ctx, int64_t* n);
int  c2d_census_export(c2d_ctx* ctx, double* d6, int32_t* i5, uint64_t* keys,
                       int64_t cap, int64_t* n);
int  c2d_census_import(c2d_ctx* ctx, const double* d6, const int32_t* i5,
                       const uint64_t* keys, int64_t n);
/* Census records in device memory, for moving census between GPUs without
 * the host (imcredist, src/imcredist.f:5-133, as RCCL send/recv or
 * hipMemcpyPeer of packed records): C2D_CENSUS_REC_WORDS 64-bit words per
 * record = rpre, zpre, wmu, phi, ew, xnu (f64 bits), jk | bins << 32, key. */
#define C2D_CENSUS_REC_WORDS 8
/* pack records [first, first+n) into d_rec (device memory of this context's GPU) */
int  c2d_census_pack(c2d_ctx* ctx, int64_t first, int64_t n, uint64_t* d_rec);
/* append n packed records (device memory) to the census */
int  c2d_census_append(c2d_ctx* ctx, const uint64_t* d_rec, int64_t n);
/* keep the first n records (drop the tail, e.g. after packing it for a send) */
int  c2d_census_truncate(c2d_ctx* ctx, int64_t n);

/* Records first, first+stride, ... (at most cap of them) of the census:
 * checkpoints in chunks, or a strided sample of a large census. */
int  c2d_census_export_range(c2d_ctx* ctx, int64_t first, int64_t stride, double* d6,
                             int32_t* i5, uint64_t* keys, int64_t cap, int64_t* n);

/* Census population control: weight-window roulette on the device
 * (csrc/c2d_roulette.h, csrc/roulette.hip).  The reference
 * stops at ucens records a rank (imctrk2d.f:573-577) and this library returns
 * C2D_E_CENSUS_OVERFLOW; with these calls a host bounds the census instead.
 * Opt-in: nothing else in the library calls them.
 *
 * group_of_sp[C2D_NPHOMAX + 1] maps a record's spectral bin jgpsp (bits 0-7
 * of its bins word, larger values taken as C2D_NPHOMAX) to a group
 * 0..ngroup-1, 1 <= ngroup <= C2D_ROULETTE_GROUPS_MAX; tables are
 * [nz][nr][ngroup], host memory.
 *
 * c2d_census_stats: per (cell, group) the exact record count and the sum of
 * ew of the census, which stays as it is.
 *
 * c2d_census_roulette: a record in cell (jph, kph) and group g with
 * w = w_min[jph-1][kph-1][g] is untouched if !(w > 0), if w is not finite, if
 * !(ew >= 0) or if ew >= w.  Otherwise it survives with probability ew / w,
 * its ew then exactly w and nothing else changed (its key included), or is
 * removed: the expected energy is unchanged.  The decision is draw 0 of the
 * key derived from the record's key with the tag C2D_TAG_ROULETTE and `salt`
 * (c2d_rng.h), a function of the record, its floor and the salt alone, so it
 * does not depend on the census mode, the record's place or the GPU; use a
 * new salt for every pass (the step number).  The census stays a valid
 * census in both modes, the chunks it no longer needs are free again as
 * after c2d_census_truncate, and the order of the survivors is free; with no
 * floor that can test a record the census is left exactly as it is.
 * out->n_tested counts the records with ew < w; e_before and e_after are the
 * sums of ew; kernel_ms is the device time of the pass.
 *
 * Errors: C2D_E_ARG, before the census is touched, for a null pointer, ngroup
 * out of range or a group id outside 0..ngroup-1; C2D_E_STATE if the census
 * was lost.  A HIP failure after c2d_census_roulette has begun rewriting
 * leaves the census lost, exactly as a failed in-place step does: the count
 * is 0 and census reads and c2d_run_step return C2D_E_STATE until the next
 * c2d_census_import, c2d_census_read or c2d_census_truncate.
 *
 * c2d_census_roulette_host: the same rule on n records in the layout of
 * c2d_census_export; keep[i] = 1 for a record that stays, ew_out[i] its ew
 * afterwards (the floor for a survivor of a test, else ew as given).  Needs
 * no context and no GPU; C2D_E_ARG also for a record whose cell is off the
 * nz x nr grid or whose jgpsp is outside 0..255. */
#define C2D_ROULETTE_GROUPS_MAX 32
typedef struct {
  int64_t n_before, n_after, n_tested;   /* n_tested: records with ew < w */
  double e_before, e_after, kernel_ms;
} c2d_roulette_out;
int  c2d_census_stats(c2d_ctx* ctx, const int32_t* group_of_sp, int32_t ngroup,
                      int64_t* count, double* energy);
/* device time of the last c2d_census_stats kernel (0 before the first) */
int  c2d_last_census_stats_ms(c2d_ctx* ctx, double* ms);
int  c2d_census_roulette(c2d_ctx* ctx, const int32_t* group_of_sp, int32_t ngroup,
                         const double* w_min, uint64_t salt, c2d_roulette_out* out);
int  c2d_census_roulette_host(const double* d6, const int32_t* i5, const uint64_t* keys, int64_t n,
                              int32_t nz, int32_t nr, const int32_t* group_of_sp, int32_t ngroup,
                              const double* w_min, uint64_t salt, uint8_t* keep, double* ew_out);

/* Census splitting: the upper weight window, and k-fold multiplication
 * (csrc/c2d_split.h, csrc/split.hip).  Opt-in, as the roulette;
 * group_of_sp, ngroup and the table layout are the roulette's.
 *
 * c2d_census_split: a record in cell (jph, kph) and group g with
 * W = w_max[jph-1][kph-1][g] is untouched if !(W > 0), if W or ew is not
 * finite or if !(ew > W).  Otherwise it becomes m records,
 * m = min(max_copies, ceil(ew / W)) >= 2 (ew / W one IEEE division), each of
 * weight ew / m (one IEEE division): copy 0 is the record itself with only
 * its ew changed, copy i = 1..m-1 equals it word for word but for its key,
 * which is derived from the record's key with the tag C2D_TAG_SPLIT, `salt`
 * and the sub i (c2d_rng.h), so the copies fly on independent streams and the
 * expected value of every tally is unchanged.  2 <= max_copies <=
 * C2D_SPLIT_COPIES_MAX; use a new salt for every pass (the step number).
 * The originals keep their places as census items [0, n_before); the copies
 * are the items [n_before, n_after) in (source item, i) order, so the result
 * is a function of the census, the ceilings, max_copies and the salt alone,
 * the same in both census modes and both builds.  With flags =
 * C2D_SPLIT_DRY the pass only counts: out is what a committed pass would
 * report, the census stays as it is.  With no ceiling that can test a record
 * the census is byte for byte what it was.  out: the counts, n_split the
 * records with m > 1, the sums of ew before and after, kernel_ms the device
 * time of the pass.
 *
 * Errors: C2D_E_ARG, before anything runs, for a null pointer, ngroup, a
 * group id or max_copies out of range or unknown flag bits; C2D_E_STATE if
 * the census was lost; C2D_E_CENSUS_OVERFLOW, before a single byte is
 * written and with the census exactly as it was, if n_after exceeds the
 * capacity or the free chunks.  A HIP failure after writing has begun leaves
 * the census lost, as for c2d_census_roulette.
 *
 * c2d_census_split_host: the same rule on n records in the layout of
 * c2d_census_export; copies[i] = m and ew_out[i] = the weight of each of the
 * m records (ew as given for m = 1).  Needs no context and no GPU; C2D_E_ARG
 * also for a record whose cell is off the nz x nr grid or whose jgpsp is
 * outside 0..255.  c2d_census_split_keys_host: the keys of the copies
 * i = 1..copies[k]-1 of the records k = 0..n-1, in that order
 * (sum (copies[k] - 1) of them). */
#define C2D_SPLIT_COPIES_MAX 64
#define C2D_SPLIT_DRY 1            /* flags: count only, the census stays as it is */
typedef struct {
  int64_t n_before, n_after, n_split;   /* n_split: records with m > 1 */
  double e_before, e_after, kernel_ms;
} c2d_split_out;
int  c2d_census_split(c2d_ctx* ctx, const int32_t* group_of_sp, int32_t ngroup, const double* w_max,
                      int32_t max_copies, uint64_t salt, int32_t flags, c2d_split_out* out);
int  c2d_census_split_host(const double* d6, const int32_t* i5, const uint64_t* keys, int64_t n,
                           int32_t nz, int32_t nr, const int32_t* group_of_sp, int32_t ngroup,
                           const double* w_max, int32_t max_copies, uint64_t salt,
                           int32_t* copies /* m per record */, double* ew_out /* ew' per record */);
int  c2d_census_split_keys_host(const uint64_t* keys, const int32_t* copies, int64_t n, uint64_t salt,
                                uint64_t* keys_out);

/* Census comb: floors that leave exactly a wanted number of records
 * (csrc/c2d_comb.h, csrc/comb.hip).  Opt-in, as the roulette.
 *
 * Under c2d_census_roulette a record of weight ew whose draw is u survives
 * the floor w iff u < ew / w; its critical floor w* is the largest finite
 * double for which that holds (0 for ew = 0), and it stays iff w <= w*.
 * With floors t * norm[jph-1][kph-1][g], norm a power of two, a record's
 * normalised critical value is c = w* / norm, and the floors keep exactly
 * the records with c >= t: t one step above the (M+1)-th largest c keeps M
 * of them.  These calls find that value where the census lies; the floors
 * are then applied by c2d_census_roulette with the same group_of_sp and the
 * same salt.  A record is `fixed`, kept by every floor of the family, if
 * !(norm > 0), norm is not finite, !(ew >= 0), ew is not finite or its cell
 * is off the grid; the others are the pool.
 *
 * The 64-bit pattern of c >= 0 orders as an unsigned integer and is read in
 * six digits: bits 63-53, 52-42, 41-31, 30-20, 19-9 (11 bits each) and 8-0.
 * prefix_bits is 0, 11, 22, 33, 44 or 55, and `prefix` holds that many bits.
 *
 * c2d_census_comb_hist: hist[d] = the pool records whose c has `prefix` in
 * its top prefix_bits bits and d as its next digit, exactly; out->n_pool the
 * pool, n_match the histogram's sum, n_fixed, n_records, kernel_ms the device
 * time of the pass.
 *
 * c2d_census_comb_collect: the c of those records to crit_host, in any order
 * and at most cap of them; *n is their full number, so *n <= cap says that
 * all arrived.
 *
 * Both leave the census exactly as it is.  Errors: C2D_E_ARG, before
 * anything runs, as for c2d_census_roulette and for a norm entry that is
 * positive and finite but no power of two, a prefix_bits off the list or a
 * prefix with bits above prefix_bits; C2D_E_STATE if the census was lost.
 *
 * c2d_census_comb_host: c and the fixed flag (crit 0 there) of n records in
 * the layout of c2d_census_export, norm [nz][nr][ngroup].  Needs no context
 * and no GPU; C2D_E_ARG also for a jgpsp outside 0..255. */
#define C2D_COMB_BINS 2048
typedef struct {
  int64_t n_records, n_fixed, n_pool, n_match;
  double kernel_ms;
} c2d_comb_out;
int  c2d_census_comb_hist(c2d_ctx* ctx, const int32_t* group_of_sp, int32_t ngroup, const double* norm,
                          uint64_t salt, uint64_t prefix, int32_t prefix_bits, uint64_t hist[C2D_COMB_BINS],
                          c2d_comb_out* out);
int  c2d_census_comb_collect(c2d_ctx* ctx, const int32_t* group_of_sp, int32_t ngroup, const double* norm,
                             uint64_t salt, uint64_t prefix, int32_t prefix_bits, double* crit_host, int64_t cap,
                             int64_t* n);
int  c2d_census_comb_host(const double* d6, const int32_t* i5, const uint64_t* keys, int64_t n,
                          int32_t nz, int32_t nr, const int32_t* group_of_sp, int32_t ngroup,
                          const double* norm, uint64_t salt, double* crit, uint8_t* fixed);

/* The census as the record file of write_cens / read_cens (census2d.f:1-76),
 * formatted on the device: two lines a record, (6e14.7) rpre zpre wmu phi ew
 * xnu and (6i5) jgpsp jgplc jgpmu jph kph seed, 116 bytes with their
 * newlines and no separators; the sixth integer is key mod 100000 and the
 * full 64-bit lineage keys go to `path`.keys (little-endian u64, one a
 * record).  The records are those of c2d_census_export, in its order;
 * *n_written = records written (n_written may be NULL).  The call returns
 * when both files are complete and closed and leaves the census unchanged.
 * Errors: C2D_E_STATE if the census was lost by a failed in-place step;
 * C2D_E_NONFINITE if a record holds a NaN or Inf (the message names the
 * first such record): the records are scanned before either file is opened,
 * so both files are then exactly as they were; C2D_E_IO if a file cannot be
 * opened or written.  An empty census gives two empty files.  The text is
 * staged in chunks of C2D_CENSTEXT_CHUNK records (environment, read at every
 * call; default 1048576) through two pinned host buffers: memory is bounded
 * by the chunk, not by the census. */
int  c2d_census_write(c2d_ctx* ctx, const char* path, int64_t* n_written);
/* The same for n caller-supplied records in host memory, in the layout of
 * c2d_census_export (d6 [n][6], i5 [n][5], keys [n]).  Nothing in the
 * records is checked against the grid; an integer outside -9999..99999 is
 * written as five asterisks, as Fortran's I5 does. */
int  c2d_census_write_from(c2d_ctx* ctx, const double* d6, const int32_t* i5, const uint64_t* keys,
                           int64_t n, const char* path);
/* The inverse: replaces the context's census with the records of the file,
 * parsed and converted on the device (what c2d_census_import does with host
 * arrays); *n = the records of the file (n may be NULL).  Keys come from
 * `path`.keys if it exists, else (a file written by the reference) they are
 * derived from the seed column and the record index (splitmix64, as
 * compton2d_amd/census_io.py derive_key).  Canonical records (116 bytes:
 * fields [ -]0.dddddddE[+-]dd or [ -]0.ddddddd[+-]ddd, integers as blanks, an
 * optional '-' and digits, both newlines in place) are parsed by a kernel,
 * each double to the bits of strtod of its field.  From the first record
 * that is not canonical to the end of the file, and for a tail shorter than
 * a record, a host parser takes over: CR stripped, blank lines skipped,
 * fixed 14- and 5-column fields, the E-less three-digit exponent repaired, D
 * or a lower-case e as the exponent letter, a missing final newline
 * accepted.  Errors: C2D_E_IO with the byte offset in the message for a
 * field the host parser cannot read (asterisks included) and for an odd
 * number of lines; C2D_E_IO if a file cannot be opened or read or `path`.keys
 * does not hold 8 bytes a record; C2D_E_ARG for a record out of range, as in
 * c2d_census_import; C2D_E_CENSUS_OVERFLOW if the file holds more records
 * than census_capacity: for a wholly canonical file this is decided from
 * the file's size before the census is touched.  A call that fails after it
 * has begun storing leaves the census lost, as a failed in-place step does:
 * the count is 0 and census reads and c2d_run_step return C2D_E_STATE until
 * the next c2d_census_import, c2d_census_read or c2d_census_truncate.  A
 * call that fails before that (a file that cannot be opened) leaves the
 * census as it was.  An empty file is a census of 0 records. */
int  c2d_census_read(c2d_ctx* ctx, const char* path, int64_t* n);
/* Parses only: the first min(cap, *n) records into host arrays in the layout
 * of c2d_census_export; *n = the records of the file; NULL buffers with
 * cap == 0 only count.  The context's census is untouched. */
int  c2d_census_read_records(c2d_ctx* ctx, const char* path, double* d6, int32_t* i5, uint64_t* keys,
                             int64_t cap, int64_t* n);
/* Diagnostics of the last c2d_census_write* / c2d_census_read*: host
 * milliseconds in file I/O and waiting for chunks, device milliseconds of
 * the format or parse kernels and of the record conversion kernels (write:
 * both passes over the census, the non-finite scan included; 0 for
 * caller-supplied records and for c2d_census_read_records), records parsed
 * on the device and on the host (0 after a write), and the chunk count.
 * Any pointer may be NULL. */
int  c2d_last_census_file_ms(c2d_ctx* ctx, double* io_ms, double* wait_ms, double* kernel_ms,
                             double* convert_ms, int64_t* device_records, int64_t* host_records,
                             int32_t* chunks);

/* Checkpoints: what one step hands to the next, as one binary file, bit for
 * bit.  A checkpoint is taken between steps and holds the census (the raw
 * words of c2d_census_pack, in the order of c2d_census_export: nothing is
 * decoded, so the fast build's encoded azimuth and the bins a record carries
 * travel as they are), the lagged kappa table of hazard H3 (kappa_prev), the
 * device-resident electron state (f_nt, Pnt), the C2D_FP_AUTO decision
 * carried from the last update, and an opaque blob of the caller's (its own
 * state: step number, zone scalars).  NOT in a checkpoint: the tallies,
 * escape events, reflection results and timers of the finished step (they
 * are outputs; after a restore they read as on a fresh context), and the
 * observer accumulations (c2d_obs_*, c2d_obs_set_*): they are sums.  An
 * exact set's (c2d_obs_set_exact) travel in the user blob: the host exports
 * each member's state (c2d_obs_set_state) before it saves and merges it into
 * the re-created set afterwards (c2d_obs_set_merge), bit for bit, as
 * CoupledRun.save(observer_set=True) does.  The f64 sums have no such call:
 * a host that keeps them reads them before it saves and adds them to the
 * later results itself.
 *
 * The file (little-endian, every part 8-byte aligned; the same state gives
 * the same bytes: no timestamps, no host names):
 *
 *   header, 128 bytes, as 16 words:
 *      0 magic "C2DCKPT\0"           8 version u32, header bytes u32 (128)
 *     16 nz i32, nr i32             24 nmu i32, encoded i32 (the census azimuth
 *                                      column is cos(phi) + the C2D_CENS_ESW bit:
 *                                      a C2D_COMTOT_TABLE context)
 *     32 grid digest u64: digest_sum of the words z[nz] r[nr] rmin zmin
 *        E_ph[400] E_field[400] (a record carries its cell and its E_ph /
 *        E_field bins)
 *     40 seed u64                   48 rank i32, world i32
 *     56 ncycle i32, sections u32 (C2D_CKPT_HAS_*)
 *     64 time f64                   72 dt f64    (the last step's clock, informational)
 *     80 n_records i64              88 records per chunk i64
 *     96 fp_auto_known i32, fp_auto_exact i32
 *    104 user blob bytes i64       112 digest_sum of the padded blob
 *    120 digest_sum of words 0..14
 *   user blob, zero-padded to a multiple of 8
 *   kappa_prev  [ncell][400] f64   (C2D_CKPT_HAS_KAPPA: once a step has run)
 *   f_nt, Pnt   [ncell][200] f64 each (C2D_CKPT_HAS_ELECTRONS)
 *      each table: (words i64, digest_sum, digest_xor), then the words
 *   census: chunks of at most C2D_CKPT_CHUNK records (environment, read at
 *      every call; default 1048576), all full but the last; each chunk:
 *      (m i64, digest_sum, digest_xor), then m records of 8 u64
 *   trailer, 24 bytes: magic "C2DCEND\0", n_records, t, where
 *      t = mix(n_records + G) and per chunk t = mix(mix(t ^ sum) ^ xor)
 *
 * The digest (mod 2^64; G = 0x9E3779B97F4A7C15; mix is SplitMix64's
 * finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *=
 * 0x94D049BB133111EB; z ^= z >> 31): the record at index g of the census,
 * words w0..w7, hashes to h = a8 with a0 = mix(g + G), a(k+1) = mix(ak ^ wk).
 * A chunk's digest is (sum of h, xor of h) over its records, g counted from
 * the census's first record: any order of reduction gives it, a change to
 * one record changes the sum (mix is a bijection), and so do two records
 * swapped (g enters).  Tables and the blob use the same rule on groups of 8
 * words, the last zero-padded, g counted from the section's start.
 * compton2d_amd/checkpoint.py is the same format in numpy. */
#define C2D_CKPT_VERSION        1
#define C2D_CKPT_HAS_KAPPA      1   /* sections */
#define C2D_CKPT_HAS_ELECTRONS  2
#define C2D_CKPT_APPEND         1   /* c2d_checkpoint_read flags */
#define C2D_CKPT_CENSUS_ONLY    2
typedef struct c2d_ckpt_info {
  int32_t version, nz, nr, nmu;
  int32_t encoded, rank, world, ncycle;
  int32_t sections, fp_auto_known, fp_auto_exact, reserved;
  uint64_t grid_digest, seed;
  double time, dt;
  int64_t n_records, chunk, user_bytes, file_bytes;
} c2d_ckpt_info;
/* Writes the context's state to `path`: to `path`.tmp, renamed at the end, so
 * the file is flushed to the disk (fsync) before it takes the name;
 * a failed call leaves an older checkpoint at `path` as it was (a path that
 * exists and is not a regular file, /dev/null, is written in place).  user
 * (user_bytes >= 0; NULL with 0) is the caller's blob.  *n_written = census
 * records written (may be NULL).  The census is gathered through the chunk
 * list and its digest computed in one kernel pass; chunks stream through two
 * pinned host buffers, bounded by C2D_CKPT_CHUNK.  The context is unchanged.
 * Before the first step the table sections are absent; an empty census is
 * valid.  Errors: C2D_E_NONFINITE if a census record or a table holds a NaN
 * or Inf (scanned before the file is opened); C2D_E_STATE if the census was
 * lost by a failed in-place step; C2D_E_IO if the file cannot be written. */
int  c2d_checkpoint_write(c2d_ctx* ctx, const char* path, const void* user, int64_t user_bytes,
                          int64_t* n_written);
/* Restores records [first, first + count) of the file's census (count = -1:
 * to the end; a range is clipped to the file) and, unless
 * C2D_CKPT_CENSUS_ONLY, kappa_prev, the electrons and the FP flags as far as
 * the file holds them.  C2D_CKPT_APPEND adds the records behind the present
 * census instead of replacing it.  user (user_cap bytes; may be NULL with 0)
 * takes the first min(user_cap, *user_bytes) bytes of the blob; *user_bytes
 * = its size; *n_records = records stored (all three are written only when
 * the whole call has succeeded; c2d_checkpoint_info gives the blob's size
 * beforehand).  A range that begins or ends
 * inside a chunk reads and verifies the whole chunks that cover it.  Every
 * record is checked on the device before it is stored (digest; cell in
 * 1..nz x 1..nr, E_ph bin in 1..400, E_field bin in 0..400, the bin bytes,
 * six finite doubles): nothing indexes a table with what a file says.
 * Decided before anything is touched, the context unchanged: C2D_E_IO for a
 * file that is missing, shorter than its header says, of another magic or
 * version, or whose header or trailer fails; C2D_E_ARG, naming which, for
 * another nz/nr/nmu, grid digest or azimuth encoding;
 * C2D_E_CENSUS_OVERFLOW for more records than fit.  The tables are read and
 * verified into staging and committed only when the whole call has
 * succeeded.  A chunk or table whose digest or record check fails, or a
 * trailer that disagrees, gives C2D_E_IO with the chunk and its byte offset
 * in the message and stores nothing of that chunk; with C2D_CKPT_APPEND the
 * census is then truncated back to what it held (the context is unchanged),
 * else the census is lost as after a failed c2d_census_read: C2D_E_STATE
 * until an import, read or truncate.  The file may come from either census
 * layout and go into either. */
int  c2d_checkpoint_read(c2d_ctx* ctx, const char* path, int64_t first, int64_t count, int32_t flags,
                         void* user, int64_t user_cap, int64_t* user_bytes, int64_t* n_records);
/* The header of a checkpoint, checked against its digest, the file's size and
 * the trailer; needs no context and no GPU.  C2D_E_IO for a file that fails. */
int  c2d_checkpoint_info(const char* path, c2d_ckpt_info* out);
/* Diagnostics of the last c2d_checkpoint_write / _read: host milliseconds in
 * file I/O and waiting for chunks, device milliseconds of the chunks' gather
 * or verify kernels (the scan before a write and the tables' digests are not
 * in it), the file bytes moved and the census chunks.  Any pointer may be
 * NULL. */
int  c2d_last_checkpoint_ms(c2d_ctx* ctx, double* io_ms, double* wait_ms, double* kernel_ms, int64_t* bytes,
                            int32_t* chunks);

/* Batched tridiagonal (Thomas with the reference's clipping) solve: one
 * zone per wavefront.  x is [ncell][nt] on the host. */
int  c2d_fp_tridag(c2d_ctx* ctx, const c2d_fp_in* in, double* x);

/* Fokker-Planck run constants (once per run; replaces setup_bcast and the
 * F_IC part of FP_bcast). */
int  c2d_fp_set_config(c2d_ctx* ctx, const c2d_fp_config* cfg);
/* One `update` (src/update2d.f:7-327) over all nz*nr zones: FP_calc for
 * every zone on the GPU (one wavefront per zone, state in LDS), the
 * E_add_up sums (zone order), the dT_max reduction and the tea update.
 * Replaces FP_send_job / FP_calc / FP_send_result / E_add_up /
 * FP_end_bcast.  Synchronous. */
int  c2d_fp_step(c2d_ctx* ctx, const c2d_fp_step_in* in, c2d_fp_step_out* out);
/* FP_calc arithmetic of the following c2d_fp_step calls:
 *   C2D_FP_EXACT (default): every sum, tridag's Thomas recurrence and
 *     McDonald's series in the reference's order -- bit for bit the det-math
 *     oracle (one in-order latency chain per zone);
 *   C2D_FP_FAST: the same per-bin and per-term arithmetic, the sums as block
 *     reductions/scans, tridag by partitions (each wave reduces its 64 rows by
 *     cyclic reduction with two coupling spikes, then a chain over the wave
 *     interfaces; plain parallel cyclic reduction, 8 levels with a barrier
 *     each, is the C2D_FPF_SPIKE=0 build), McDonald's terms
 *     summed as a tree (the same terms: the reference's stopping index) --
 *     equal to the exact mode within rounding (DESIGN.md §4b states the
 *     tolerance: f_nt 1e-10 relative, Te_new on the same 1.005 lattice);
 *   C2D_FP_AUTO: per update, C2D_FP_EXACT when every zone's tea sits on the
 *     reference's clamp (tea <= temp_min = 5 or >= temp_max = 1000 keV, the
 *     last update's Te_new clamped, src/update2d.f:266-276; skipped zones
 *     aside) and the last update's slowest zone took <= C2D_FP_AUTO_STEPS
 *     implicit sub-steps (src/update2d.f:1473; no last update: not asked):
 *     the exact kernel's in-order chain is then short (C3: 5 sub-steps,
 *     1.1 ms against the fast kernel's 3.4 ms); C2D_FP_FAST otherwise (off
 *     the clamp: ~29 ms against ~380 ms).  c2d_last_fp_mode reports it.
 * A fast update with no measured zone order yet (the context's first update;
 * either kernel's sub-step counts order the next) takes the zones costliest
 * first by an a-priori estimate: a probe launch evaluates every zone's first
 * implicit sub-step and orders the zones by 1/f_t_implicit (the sub-steps it
 * implies, src/update2d.f:662-665). */
#define C2D_FP_EXACT 0
#define C2D_FP_FAST  1
#define C2D_FP_AUTO  2
#define C2D_FP_AUTO_STEPS 64
int  c2d_fp_set_mode(c2d_ctx* ctx, int32_t mode);
/* The arithmetic the last c2d_fp_step used (C2D_FP_EXACT or C2D_FP_FAST:
 * C2D_FP_AUTO's choice); -1 before the first update. */
int  c2d_last_fp_mode(c2d_ctx* ctx, int32_t* mode);

/* Device timing of the last step's dominant kernel (transport generation 0):
 * milliseconds and launches, measured with HIP events on the library's
 * own stream. */
int  c2d_last_kernel_ms(c2d_ctx* ctx, double* gen0_ms, double* all_ms, int32_t* launches);
/* Diagnostic: section counters of the last step's transport launches
 * (wave-level shader cycles and event counts, tools/tr_prof.py).  All zero
 * unless the library was built with -DC2D_TR_PROF (FAST_FLAGS / EXACT). */
#define C2D_TR_PROF_WORDS 32
int  c2d_transport_prof(c2d_ctx* ctx, uint64_t* out, int32_t n);
/* Start an observer-frame histogram (zeroed on the device): sums of ew, of
 * ew^2 and counts per [n_t][n_mu][n_e] bin. */
int  c2d_obs_begin(c2d_ctx* ctx, const c2d_obs_bins* bins);
/* Bin escape events into it: events == NULL bins the last transport step's
 * device event buffer (c2d_events layout); otherwise n host events of 7 f64
 * (t_bound, xnu, ew, rpre, zpre, wmu, phi). */
int  c2d_obs_accumulate(c2d_ctx* ctx, const double* events, int64_t n);
/* Same for n events already in device memory on the context's GPU (e.g. a
 * gathered event buffer or a torch tensor); no copy. */
int  c2d_obs_accumulate_device(c2d_ctx* ctx, const double* d_events, int64_t n);
/* The same over an event file (c2d_events_read's parser): each chunk is
 * binned from device memory as it is parsed; *n = the records binned (n may
 * be NULL), also when the call fails on a bad token (C2D_E_IO).  Synchronous
 * on return.  C2D_E_STATE without c2d_obs_begin. */
int  c2d_obs_accumulate_file(c2d_ctx* ctx, const char* path, int64_t* n);
/* Download the raw sums ([n_t][n_mu][n_e] each; any pointer may be NULL)
 * and the device time of the binning launches so far (ms). */
int  c2d_obs_result(c2d_ctx* ctx, double* F, double* F2, double* count, double* kernel_ms);
/* The SED tool's binning from its own input dialogue: `deck` is pspt's stdin
 * (one answer a line, an empty line keeps pspt's default, "" or NULL = all
 * defaults; e.g. postprocessing/mrk421_sed.input), parsed and turned into
 * edges with pspt's arithmetic (postprocessing/pspt.c:105-205), then
 * c2d_obs_begin.  Replaces writing p###_evb.dat and running pspt on it. */
int  c2d_obs_begin_pspt(c2d_ctx* ctx, const char* deck);
/* Write pspt's output file (pspt.c:323-353, byte for byte its format) from
 * the histogram so far: `path` (NULL/"" = the deck's output file name),
 * `factor` as pspt's "#factor" line.  world_sum != 0: the histograms of every
 * rank of the context's communicator are summed first (RCCL; every rank
 * calls, rank 0 writes). */
int  c2d_obs_write_pspt(c2d_ctx* ctx, const char* path, int32_t factor, int32_t world_sum);

/* Observer sets: up to C2D_OBS_SET_MAX binnings (pspt SEDs of several
 * windows, plcm light curves, raw c2d_obs_bins), each with its own Gamma,
 * r_max, t_offset and edges, filled by ONE pass over the escape events: an
 * accumulate call reads the events once and launches the same number of
 * kernels however many members the set has.  The set's state is separate
 * from the single histogram of c2d_obs_begin; both may be used after the
 * same step (each waits for the other's binning of the device event buffer).
 * The edges of all members are staged in one workgroup's LDS (63 KiB):
 * an add that would exceed it fails with C2D_E_ARG and leaves the set as it
 * was.  Members are numbered from 0 in the order they are added. */
#define C2D_OBS_SET_MAX 8
/* Drop every member (and its histogram). */
int  c2d_obs_set_clear(c2d_ctx* ctx);
/* Add a member with a zeroed histogram; *id (may be NULL) receives its
 * number.  Arguments and limits as c2d_obs_begin; a ninth member is
 * C2D_E_ARG; adding after the first accumulate since c2d_obs_set_clear is
 * C2D_E_STATE. */
int  c2d_obs_set_add(c2d_ctx* ctx, const c2d_obs_bins* bins, int32_t* id);
/* Add a member from pspt's dialogue (as c2d_obs_begin_pspt) or from plcm's
 * (postprocessing/plcm.c:97-302, e.g. postprocessing/mrk421_lc.input: names,
 * angular bins, dt, t_offset, t_max, energy bands; plcm's 1024 chained time
 * bins). */
int  c2d_obs_set_add_pspt(c2d_ctx* ctx, const char* deck, int32_t* id);
int  c2d_obs_set_add_plcm(c2d_ctx* ctx, const char* deck, int32_t* id);
/* Bin events into every member: events == NULL bins the last transport
 * step's device event buffer (asynchronously, like c2d_obs_accumulate: the
 * next step's first launch and every reader wait for it), otherwise n host
 * events of 7 f64.  C2D_E_STATE on an empty set. */
int  c2d_obs_set_accumulate(c2d_ctx* ctx, const double* events, int64_t n);
/* Same for n events already in device memory on the context's GPU. */
int  c2d_obs_set_accumulate_device(c2d_ctx* ctx, const double* d_events, int64_t n);
/* The same over an event file, as c2d_obs_accumulate_file; C2D_E_STATE on an
 * empty set. */
int  c2d_obs_set_accumulate_file(c2d_ctx* ctx, const char* path, int64_t* n);
/* A member's histogram shape and how many of its leading time rows the
 * kernel keeps in LDS (the rest use global atomics); any pointer may be NULL. */
int  c2d_obs_set_shape(c2d_ctx* ctx, int32_t id, int32_t* n_t, int32_t* n_mu, int32_t* n_e, int32_t* lds_rows);
/* Download a member's raw sums ([n_t][n_mu][n_e] each; any may be NULL). */
int  c2d_obs_set_result(c2d_ctx* ctx, int32_t id, double* F, double* F2, double* count);
/* Device time (ms) and number of the set's kernel launches since the clear. */
int  c2d_obs_set_kernel_ms(c2d_ctx* ctx, double* ms, int32_t* launches);
/* Write the tool's files of a deck member from its histogram so far
 * (C2D_E_STATE for a member added with raw bins).  pspt member: `path` is
 * the output file (NULL/"" = the deck's name), as c2d_obs_write_pspt.  plcm
 * member: `path` is a directory (NULL/"" = "."); the files take the deck's
 * names: <name> and <name>_aux per angular bin and one <name>_particles
 * (plcm.c:377-388, 466-552).  world_sum != 0: F, F2 and count of the member
 * are summed over the context's communicator first (every rank calls, rank
 * 0 writes). */
int  c2d_obs_set_write(c2d_ctx* ctx, int32_t id, const char* path, int32_t factor, int32_t world_sum);

/* Exact observer sets: order-independent sums.  The f64 sums
 * above are added with atomics in an unspecified order, so two runs over the
 * same events agree to rounding only.  After c2d_obs_set_exact every member
 * of the set accumulates integers instead, and integer addition commutes:
 * the same events give the same bits in any order, batch split, shard count
 * or, through the exported state, across processes and checkpoints.
 *
 * The arithmetic.  E(x) is the frexp exponent (x = f 2^E(x), 0.5 <= f < 1).
 * w_max bounds the rest-frame weight ew of any single event.  A member with
 * bulk factor G has the exponent bound e = E(w_max) + E(2 G): a boosted
 * weight w = ew G (1 + mu beta), |mu| <= 1, lies below 2^e.  Each bin holds
 *   F      unsigned 128-bit, in units of 2^qF,  qF  = e - 84
 *   F2     unsigned 128-bit, in units of 2^qF2, qF2 = 2 e - 84
 *   count  unsigned 64-bit
 * and an event that the bin decision of the f64 set puts into bin h adds
 * floor(w / 2^qF) to F[h], floor(fl(w w) / 2^qF2) to F2[h] and 1 to
 * count[h], with w and fl(w w) the doubles the f64 set adds.  Both addends
 * are below 2^84: a bin has 2^44 worst-case addends of headroom.  An event
 * whose w is NaN, negative or >= 2^e is added nowhere; if a bin would have
 * taken it, it is counted in the member's n_rejected (once per event).
 * Truncation depends on the addend alone, so 0 <= sum(w) - F 2^qF <
 * count 2^qF.  -469 <= e <= 489 keeps every quantum and every sum a normal
 * double.  Reported F, F2 and count are the integers scaled and rounded to
 * nearest, ties to even: one rounding per bin.  A generous w_max costs only
 * spare low bits (84 bits below 2^e are kept); one set too low surfaces as
 * n_rejected, never as a silent loss.
 *
 * The state of a member, u64 words (little-endian when stored):
 *   0 magic "C2DOBSX\0"        1 version u32 (1), mode u32 (C2D_OBS_SED | C2D_OBS_LC)
 *   2 n_t u32, n_mu u32        3 n_e u32, zero u32
 *   4 e, i64                   5 digest_sum of the words G, rmax, t_offset and the
 *                                edges t0 t1 mu0 mu1 E0 E1 (the checkpoint's rule)
 *   6 n_rejected               7 digest_sum of the payload
 *   then 5 words per bin in [n_t][n_mu][n_e] order: F_lo F_hi F2_lo F2_hi count */
#define C2D_OBS_STATE_HEAD_WORDS 8
#define C2D_OBS_STATE_BIN_WORDS  5
/* Make the set exact: after c2d_obs_set_clear and before the first
 * accumulate (later: C2D_E_STATE, as a second call is).  Every member, added
 * before or after the call, accumulates exactly, by all three accumulate
 * routes; c2d_obs_set_clear ends exact mode.  C2D_E_ARG for a w_max that is
 * not finite and positive, and, here or at the add, for a member whose e
 * falls outside [-469, 489]; the set is then as it was.  On an exact set
 * c2d_obs_set_result and c2d_obs_set_write give the rounded doubles, and
 * C2D_E_NONFINITE, naming the count and w_max, when n_rejected != 0;
 * c2d_obs_set_write with world_sum sums the integers over the communicator
 * (32-bit halves in u64 containers, carries normalised afterwards) and
 * c2d_obs_set_shape reports the rows the exact kernel privatises (a bin is 5
 * words of LDS, not 3). */
int  c2d_obs_set_exact(c2d_ctx* ctx, double w_max);
/* A member's exponent bound and rejected events (either may be NULL).
 * C2D_E_STATE on a set that is not exact, here and below. */
int  c2d_obs_set_exact_info(c2d_ctx* ctx, int32_t id, int32_t* e, int64_t* n_rejected);
/* The member's state: its size in words, and the words (cap < size:
 * C2D_E_ARG). */
int  c2d_obs_set_state_words(c2d_ctx* ctx, int32_t id, int64_t* words);
int  c2d_obs_set_state(c2d_ctx* ctx, int32_t id, uint64_t* out, int64_t cap);
/* Add an exported state into member `id` (sums, counts and n_rejected), e.g.
 * another rank's, or a saved one into a re-created set after a restore; from
 * then on the set takes no further member.  C2D_E_ARG, leaving the member
 * unchanged, for another shape, mode, e or binning digest, a failed payload
 * digest, or a sum that would carry out of bit 127. */
int  c2d_obs_set_merge(c2d_ctx* ctx, int32_t id, const uint64_t* in, int64_t words);
/* The host twin of the exact kernel for one binning, no context and no GPU:
 * adds n events into `state` (cap words >= 8 + 5 n_t n_mu n_e), which is
 * either zeroed (state[0] == 0: a fresh state is begun) or a state of this
 * binning and bound.  C2D_E_ARG (state unchanged) for a bad binning, w_max
 * or e, a short buffer or a state of another binning. */
int  c2d_obs_exact_host(const c2d_obs_bins* bins, double w_max, const double* events, int64_t n,
                        uint64_t* state, int64_t cap);
/* into += from on the host, with c2d_obs_set_merge's checks. */
int  c2d_obs_state_merge(uint64_t* into, int64_t into_words, const uint64_t* from, int64_t from_words);
/* A state's rounded doubles ([n_t][n_mu][n_e] each; any may be NULL);
 * C2D_E_ARG for words that are no state or fail the payload digest.
 * n_rejected is word 6 of the state: the caller's to look at. */
int  c2d_obs_state_result(const uint64_t* state, int64_t words, double* F, double* F2, double* count);

/* Copy the context's device electron state (C2D_DEV_ELECTRONS) into the
 * caller's f_nt / Pnt views (either may have NULL data), e.g. before
 * write_record (src/write_record.f) in a device-resident run. */
int  c2d_electron_state(c2d_ctx* ctx, c2d_marray3 f_nt, c2d_marray3 Pnt);

/* Device time of the last c2d_fp_step's FP kernel (HIP events, ms). */
int  c2d_last_fp_ms(c2d_ctx* ctx, double* ms);

/* imcgen2d's per-cell emission/absorption loop (volume_em for every cell)
 * on the GPU, one workgroup per cell; results written to the host arrays of
 * `out` that are non-NULL and kept on the device for a following
 * c2d_set_step with C2D_DEV_EMISSION.  Synchronous. */
int  c2d_volume_em(c2d_ctx* ctx, const c2d_vem_in* in, c2d_vem_out* out);
/* Device time of the last c2d_volume_em kernel (HIP events, ms). */
int  c2d_last_vem_ms(c2d_ctx* ctx, double* ms);
/* Packet-steps executed by that generation-0 launch (roofline numerator). */
int  c2d_last_gen0_steps(c2d_ctx* ctx, int64_t* steps);
/* Lane path-steps of the last step: passes of a GPU lane through the
 * geometry block (imctrk2d.f:228-379), of the generation-0 launch and of all
 * launches.  The per-copy tracker makes one per packet-step; a probe bundle
 * one per shared step of all the copies on its path, so
 * packet-steps / path-steps is the work sharing factor.  Either pointer may
 * be NULL. */
int  c2d_last_path_steps(c2d_ctx* ctx, int64_t* gen0_paths, int64_t* all_paths);
/* How the last step closed its census (the dbufout/ibufout of
 * imctrk2d.f:558-572 + imcfield2d.f:96-97): double-buffered, the rounds of
 * the compaction that closed the dead chunk tails and the records it moved;
 * chunked (census_inplace), the batches that packed the partly filled chunks
 * and their records.  physical = the census slots the context holds.  Any
 * pointer may be NULL. */
int  c2d_last_compaction(c2d_ctx* ctx, int32_t* rounds, int64_t* moved, int64_t* physical);
/* Chunked census (census_inplace = 1): the chunks the census occupies, the
 * chunks the last step's bundle kernel freed and refilled within the step,
 * the census chunks it could not count down (these wait for the next step),
 * and the chunks the context holds (1024 records each).  Double-buffered:
 * zeros.  Any pointer may be NULL. */
int  c2d_last_census_chunks(c2d_ctx* ctx, int64_t* chunks, int64_t* recycled, int64_t* unrecycled,
                            int64_t* physical);

/* ------------------------------------------------------------------------
 * Multi-GPU tally reduction over RCCL (xGMI), for hosts that drive one
 * context per GPU themselves (the kept Fortran driver, one MPI rank per GPU).
 * Replaces the per-step scalar MPI_REDUCE loops of xec_add /
 * graphics_collect (src/xec2d.f:325-399) and cens_add_up / E_add_up
 * (src/update2d.f:1929-2078) with ONE in-place all-reduce of the fused tally
 * buffer (c2d_tally_layout) per step.
 *   rank 0: c2d_comm_unique_id(id); the host broadcasts the C2D_COMM_ID_BYTES
 *   bytes (e.g. MPI_Bcast); every rank: c2d_comm_init(ctx, id, rank, world);
 *   per step after c2d_run_step: c2d_allreduce_tallies(ctx).
 * ---------------------------------------------------------------------- */
#define C2D_COMM_ID_BYTES 128
int  c2d_comm_unique_id(void* id, int64_t cap);
int  c2d_comm_init(c2d_ctx* ctx, const void* id, int32_t rank, int32_t world);
/* ncclAllReduce(sum, f64) in place on the context's tally buffer, on the
 * context's stream; synchronous.  Without c2d_comm_init: C2D_E_STATE. */
int  c2d_allreduce_tallies(c2d_ctx* ctx);
/* GPUs visible to this process (hipGetDeviceCount), so an MPI host can map
 * its ranks to devices (c2d_config.device); 0 and C2D_E_HIP without one. */
int  c2d_device_count(int32_t* n);

/* Diagnostics: evaluate the transport kernels' elementary functions on the
 * device (fn 0 log, 1 exp, 2 cos, 3 acos, 4 cbrt-by-pow, 5 sqrt, 6 x/3,
 * 7 Philox draw with key=x, counter=index) for bit-parity checks. */
int  c2d_selftest_math(int device, int fn, const double* x, double* y, int64_t n);
/* Diagnostics: the r-boundary distance of the flight step (src/imctrk2d.f:
 * 251-277: psq, dpbsq, disbr = inout*sqrt(dpbsq) - Eta*rpre, trldb =
 * disbr/sqrt(1 - wmu^2)) for n rays in[4n] = (rpre, Eta, wmu, rbnd; rbnd < 0:
 * the inner boundary |rbnd|, inout = -1) with
 * the fast build's square root / reciprocal sequences after `nr` Newton
 * steps (nr 1: the fast build, 2: its former default) and with IEEE sqrt
 * and division (nr 0: the exact build); out[2n] = (disbr, trldb). */
int  c2d_selftest_geom(int device, int nr, const double* in, double* out, int64_t n);
/* Diagnostics: the fast FP kernel's McDonald pair (volume2d.f:598-626) at n
 * arguments z from its moment table and from its term-by-term series;
 * out[8n] = (K2, K3 from the table, K2, K3 from the series, 1 if the table
 * answered, shader cycles of the table's gamma_bar and of the series,
 * gamma_bar = K3/K2 - 1/z as the fast kernel forms it from the table). */
int  c2d_selftest_mcd_fast(int device, const double* z, int n, double* out);
/* Diagnostics: the fast FP kernel's workgroup size (C2D_FPF_BS) and its
 * McDonald terms per thread per pass (C2D_FPF_TPT), which shape the arrays of
 * the two entries below.  Either pointer may be null. */
int  c2d_selftest_fp_dims(int32_t* block, int32_t* tpt);
/* Diagnostics: the fast FP kernel's tridiagonal solvers (solver 0: the
 * partitioned solver it runs, 1: plain parallel cyclic reduction) on nsys
 * systems a x_{i-1} + b x_i + c x_{i+1} = d of C2D_NUM_NT rows, arrays
 * [nsys][C2D_NUM_NT]: one workgroup of `block` threads solves them one after
 * another as the kernel's sub-steps do, thread t holding row t+1 and the
 * threads past the last row the identity row.  x[nsys][block]: every thread's
 * result (0 past the last row). */
int  c2d_selftest_fp_solve(int device, int solver, const double* a, const double* b, const double* c,
                           const double* d, int nsys, double* x);
/* Diagnostics: one of the fast FP kernel's block primitives on nvec vectors
 * of per-thread values, one workgroup of `block` threads taking them one after
 * another; every thread's results are returned.
 *   op 0 sum2:     double in_a, in_b [nvec][block] -> double out[nvec][2][block]
 *   op 1 scan:     double in_a (in_b unused)       -> (prefix, total)
 *   op 2 scan_sum: double in_a (scanned), in_b (summed) -> out[nvec][3][block]
 *                  (prefix, total, sum of in_b)
 *   op 3 minmax:   int32 in_a, in_b -> int32 out[nvec][2][block] (min a, max b)
 *   op 4 min2:     int32 in_a, in_b -> (min a, min b)
 *   op 5 firsts:   flag bytes in_a, in_b [nvec][tpt][block], term k*block + t
 *                  at [k][t] -> int32 (first set term of a, of b; INT_MAX: none) */
int  c2d_selftest_fp_block(int device, int op, const void* in_a, const void* in_b, int nvec, void* out);
/* Diagnostics: Fortran E14.7 of n doubles on the GPU (csrc/c2d_fmt.h as the
 * event writer runs it), 14 bytes each at out + 14 i, no terminator.
 * C2D_E_NONFINITE if a value is NaN or Inf (its 14 bytes are then '#').
 * C2D_FMT_SELFTEST_MULTILIMB=1 (environment, read at every call) sends every
 * value the fast path cannot decide through the multi-limb path. */
int  c2d_selftest_fmt(int device, const double* x, int64_t n, char* out);
/* Diagnostics: n 14-byte E14.7 fields at text + 14 i parsed on the GPU
 * (csrc/c2d_scan.h as the event reader runs it): status[i] = 0, 1 (decided by
 * the multi-limb path) or -1 (not canonical; out[i] is then left as it was).
 * C2D_SCAN_SELFTEST_EXACT=1 (environment, read at every call; the event
 * reader honours it too) sends every field through the multi-limb path. */
int  c2d_selftest_scan(int device, const char* text, int64_t n, double* out, int32_t* status);

/* ---- Compton reflection (c2d_config.cr_sent) ---- */
#define C2D_NREF 500   /* n_ref: energies of the reflection tables (general.pa) */
/* The run-constant tables of src/ref_matrix.f built on the host in the
 * reference's summation order; needs no context and no GPU.  E_ref[500] in
 * keV; P_ref and W_abs are [n_in][n_out] (500 x 500, n_out fastest: the
 * reference's P_ref(n_out, n_in) in memory).  Any pointer may be null.
 * C2D_E_ARG if a P_ref column is not non-decreasing in n_out. */
int  c2d_reflect_tables_host(double* E_ref, double* P_ref, double* W_abs);
/* The context's device copies of the same tables (uploaded by c2d_init for
 * cr_sent 1..3); C2D_E_STATE for cr_sent 0 and 4, which use none. */
int  c2d_reflect_tables(c2d_ctx* ctx, double* E_ref, double* P_ref, double* W_abs);
/* The last step's Ed_ref[nr] (imcleak2d.f:155: the reflected weight per lower
 * ring) and counts[3] = packets reflected specularly, through the matrix at
 * the lower boundary, and by the disk.  They live beside the tally buffer
 * (c2d_tally_layout is unchanged) and are zeroed when a step starts.
 * world_sum != 0 sums over the context's communicator first (c2d_comm_init).
 * C2D_E_STATE before the first step; zeros with cr_sent = 0. */
int  c2d_reflect_result(c2d_ctx* ctx, double* Ed_ref, int64_t counts[3], int32_t world_sum);
/* Diagnostics: the kernels' reflection functions (csrc/c2d_reflect.hpp) on n
 * packet states.  boundary 0 = lower (one ring), 1 = outer r-boundary; time =
 * 100, dt = 10; in[8 n] = xnu, ew, wmu, rpre, zpre, phi, dcen, tbbl; stream
 * (keys[i], sub 0) from counter 0.  out[10 n] = xnu, ew, wmu, rpre, zpre,
 * t_bound, draws taken, idead, n_in, n_out (1-based; 0 when no matrix lookup
 * was made); t_bound = time + dt - rad_cp dcen unless the disk reflected.
 * *Ed_ref_sum = the sum of the scratch Ed_ref the adds went to. */
int  c2d_selftest_reflect(int device, int boundary, int cr_sent, int spec_switch, const double* in,
                          const uint64_t* keys, int64_t n, double* out, double* Ed_ref_sum);

/* ---- Run setup: what the reference's `setup` computes before the first step ---- */
/* None of these needs a context.  The *_host calls use no GPU; `libm` != 0
 * evaluates log/exp/pow with the C library (the reference's bits: F_IC equals
 * its IC_loss bit for bit, f_nt/Pnt its P_nontherm), `libm` = 0 with the
 * library's own c2d_log/c2d_exp/c2d_pow, which is what the GPU calls run: a
 * device call and its host twin with libm = 0 agree bit for bit.
 * Errors: C2D_E_ARG for a null pointer, a size out of range or a value that
 * must be positive and is not; C2D_E_NONFINITE for a NaN or Inf input;
 * C2D_E_FP if a series or loop reaches its iteration cap.  Arguments are
 * checked before anything is launched or written. */
/* gnt[C2D_NUM_NT] as P_nontherm builds it (nontherm2d.f:52-100), E_field
 * [C2D_NPHFIELD] (setup2d.f:216-222), E_ph[C2D_N_VOL] (volume2d.f:53, 96-113);
 * any pointer may be null.  Host only. */
int  c2d_setup_grids(double* gnt, double* E_field, double* E_ph);
/* IC_loss (src/icloss2d.f): F_IC[i_el * s_i + i_ph * s_ph] for i_el < n_el <=
 * C2D_NUM_NT, i_ph < n_ph <= C2D_NPHFIELD (strides in elements: s_i = 1, s_ph
 * = num_nt fills a Fortran F_IC(num_nt, nphfield) in place, as c2d_fp_config
 * takes it).  gnt and E_field must be positive.  Entries of the
 * Klein-Nishina branch at high photon energy are cancellation residue, some
 * negative: the reference's table, reproduced as it is. */
int  c2d_ic_loss(int device, const double* gnt, int n_el, const double* E_field, int n_ph,
                 double* F_IC, int64_t s_i, int64_t s_ph);
int  c2d_ic_loss_host(const double* gnt, int n_el, const double* E_field, int n_ph,
                      double* F_IC, int64_t s_i, int64_t s_ph, int libm);
/* c2d_ic_loss that also reports the series kernel's HIP-event time in ms
 * (kernel_ms may be null). */
int  c2d_ic_loss_timed(int device, const double* gnt, int n_el, const double* E_field, int n_ph,
                       double* F_IC, int64_t s_i, int64_t s_ph, double* kernel_ms);
/* gam_min then P_nontherm (src/gamma1_2d.f:2-52, src/nontherm2d.f:20-121, the
 * ncycle = 0 branch) of n <= C2D_MAXZONE^2 zones on the grid of
 * c2d_setup_grids: inputs [n]; gmin_out (gmin as gam_min adjusts it), N_nth,
 * gbar_nth [n]; f_nt, Pnt [n][C2D_NUM_NT].  tea, gmin, gmax must be positive.
 * p_nth = 1 with amxwl < 1 gives NaN spectra, as in the reference (0/0 in
 * P_nontherm). */
int  c2d_setup_electrons(int device, int64_t n, const double* tea, const double* amxwl,
                         const double* gmin, const double* gmax, const double* p_nth,
                         double* gmin_out, double* N_nth, double* gbar_nth, double* f_nt, double* Pnt);
int  c2d_setup_electrons_host(int64_t n, const double* tea, const double* amxwl,
                              const double* gmin, const double* gmax, const double* p_nth,
                              double* gmin_out, double* N_nth, double* gbar_nth, double* f_nt,
                              double* Pnt, int libm);

#ifdef __cplusplus
}
#endif
#endif /* COMPTON2D_H */
