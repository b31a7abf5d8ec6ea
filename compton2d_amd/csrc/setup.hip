/*
 * setup.hip — the inputs that start a run, on the device and on the host:
 *   c2d_ic_loss / c2d_ic_loss_host             F_IC (src/icloss2d.f IC_loss)
 *   c2d_setup_electrons / ..._host             gam_min + P_nontherm per zone
 *   c2d_setup_grids                            gnt, E_field, E_ph
 * The arithmetic is setup_host.h's, shared by both routes; the device runs
 * its c2d_math flavour, so device and c2d_*_host(libm = 0) agree bit for bit.
 *
 * c2d_icloss_kernel.  IC_loss is ~1e5 independent f_Li series, each a strictly
 * sequential recurrence sd_n = sd_{n-1} ((n-1)/n)^2 / y, sum += sd_n with 1
 * to 78 000 terms.  One lane runs one series in order (f_Li(z1) and f_Li(z2)
 * of an entry are two lanes' work; the reference evaluates each twice, in f1
 * and in f2).  A wave holds 64 neighbouring i_ph of one i_el and one of the
 * two arguments, whose trip counts vary smoothly; the waves are launched
 * longest first (the host sorts them by an estimate of their longest lane), so
 * the few 78 000-term waves start at once and the short ones fill in behind.
 * What differs from the reference's loop changes no value:
 *   - ((n-1)/n)^2 comes from a table of the same IEEE quotient and product
 *     (the factor is the same for every lane at term n); past the table's
 *     end it is computed in place;
 *   - `dabs(sd/sum) > 1e-10` is decided without the division when |sd| is
 *     outside [1 - 2^-40, 1 + 2^-40] * fl(1e-10 |sum|): both roundings
 *     involved are below 2^-52 relative, far inside the margin.  Otherwise
 *     the exact quotient is formed and compared.
 * No reciprocal multiply, no FMA (-ffp-contract=off), no reordering of sum.
 * A series that has not stopped after C2D_SU_FLI_CAP terms flags C2D_E_FP.
 *
 * c2d_esetup_kernel.  One wave per zone: the zone scalars wave-uniform,
 * gamma_bar by the wave-level routine of the FP kernels (c2d_wave.hpp), f_nt
 * one bin per lane, the 200-bin running sum by lane 0 in bin order.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "c2d_device.hpp"
#include "c2d_math.h"
#include "c2d_wave.hpp"
#include "setup_host.h"

/* selftest.hip: the McDonald abscissa table as c2d_fp_config builds it */
std::vector<double> c2d_mcd_abscissae();

namespace c2d {

constexpr int SU_WAVE = 64;
enum { SU_ERR_CAP = 1 };

/* items[3 b] = i_el, first i_ph, which argument (0: z1, 1: z2) of block b;
 * fli[(i_el n_ph + i_ph) 2 + which] = f_Li */
__global__ void __launch_bounds__(SU_WAVE)
    c2d_icloss_kernel(const int* __restrict__ items, const double* __restrict__ gnt,
                      const double* __restrict__ E_field, int n_ph, const double* __restrict__ r2tab,
                      int ntab, double* __restrict__ fli, int* __restrict__ err) {
  const int* it = items + 3 * (size_t)blockIdx.x;
  const int i_el = it[0], p = it[1] + (int)threadIdx.x, which = it[2];
  if (p >= n_ph) return;
  c2d_su_ic_entry e;
  if (!c2d_su_ic_args(gnt[i_el], E_field[p], &e)) return;
  const double z = which ? e.z2 : e.z1;
  const double y = 1.0 + 2.0 * z;
  double sum = c2d_su_fli_start(z, 0);
  double sd = 1.0 / y;
  sum = sum + sd;
  const double hi = 1.0 + 0x1p-40, lo = 1.0 - 0x1p-40;
  /* ((n-1)/n)^2 of term n; the load of term n + 1 is issued before term n's
   * division so that it is not waited for on the chain */
  auto r2_at = [&](int m) -> double {
    if (m < ntab) return r2tab[m];
    const double nn = (double)m;
    const double q = (nn - 1.0) / nn;
    return q * q;
  };
  int n = 2; /* the next term */
  double r2 = r2_at(n);
  for (;;) {
    const double as = fabs(sd), t = 1.0e-10 * fabs(sum);
    bool go;
    if (t > 1.0e-290 && as > t * hi)
      go = true;
    else if (t > 1.0e-290 && as < t * lo)
      go = false;
    else
      go = fabs(sd / sum) > 1.0e-10;
    if (!go) break;
    if (n > C2D_SU_FLI_CAP) {
      atomicOr(err, SU_ERR_CAP);
      break;
    }
    const double r2n = r2_at(n + 1);
    sd = sd * r2 / y;
    sum = sum + sd;
    n++;
    r2 = r2n;
  }
  fli[((size_t)i_el * n_ph + p) * 2 + which] = sum;
}

/* F[i_el n_ph + i_ph] from the series values (icloss2d.f:31-42) */
__global__ void c2d_icloss_finish_kernel(const double* __restrict__ gnt, const double* __restrict__ E_field,
                                         int n_el, int n_ph, const double* __restrict__ fli,
                                         double* __restrict__ F) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_el * n_ph) return;
  c2d_su_ic_entry e;
  if (c2d_su_ic_args(gnt[k / n_ph], E_field[k % n_ph], &e))
    F[k] = c2d_su_ic_kn(&e, fli[2 * (size_t)k], fli[2 * (size_t)k + 1], 0);
  else
    F[k] = c2d_su_ic_thomson(&e);
}

/* zone b: in[5][n] = tea, amxwl, gmin, gmax, p_nth; scal[3][n] = gmin_out,
 * N_nth, gbar_nth; f_nt, Pnt [n][200] */
__global__ void __launch_bounds__(SU_WAVE)
    c2d_esetup_kernel(int n, const double* __restrict__ in, const double* __restrict__ gnt,
                      const double* __restrict__ mcd, double* __restrict__ scal, double* __restrict__ f_nt,
                      double* __restrict__ Pnt, int* __restrict__ err) {
  __shared__ double s_mcd[4 * wave::FPB];
  __shared__ double s_f[C2D_SU_NUM_NT], s_P[C2D_SU_NUM_NT];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= n) return;
  const double tea = in[b], amxwl = in[(size_t)n + b], gmin0 = in[2 * (size_t)n + b],
               gmax = in[3 * (size_t)n + b], p_nth = in[4 * (size_t)n + b];
  c2d_su_gm gm;
  int capped = 0;
  long long guard = 0;
  double gbar;
  if (c2d_su_gam_min(tea, amxwl, gmin0, gmax, p_nth, 0, &gm))
    gbar = wave::gamma_bar_w(gm.Theta, lane, mcd, guard, s_mcd);
  else
    gbar = c2d_su_gbar_pl(&gm, gmax, 0);
  if (guard > wave::GUARD_MAX) capped = 1;
  const double Theta = tea / 5.11e2;
  double Ntherm, Nnth;
  c2d_su_pnt_norm(Theta, amxwl, gm.gmin, gmax, p_nth, 0, &Ntherm, &Nnth, &capped);
  for (int i = lane; i < C2D_SU_NUM_NT; i += SU_WAVE)
    s_f[i] = c2d_su_fnt_bin(gnt[i], Theta, amxwl, gm.gmin, gmax, p_nth, Ntherm, Nnth, 0);
  __syncthreads();
  if (lane == 0) {
    double sum = 0.0;
    for (int i = 1; i < C2D_SU_NUM_NT; i++) {
      sum = sum + s_f[i - 1] * (gnt[i] - gnt[i - 1]);
      s_P[i - 1] = sum;
    }
    s_P[C2D_SU_NUM_NT - 1] = sum;
    scal[b] = gm.gmin;
    scal[(size_t)n + b] = gm.N_nth;
    scal[2 * (size_t)n + b] = gbar;
    if (capped) atomicOr(err, SU_ERR_CAP);
  }
  __syncthreads();
  const double sum = s_P[C2D_SU_NUM_NT - 1];
  for (int i = lane; i < C2D_SU_NUM_NT; i += SU_WAVE) {
    Pnt[(size_t)b * C2D_SU_NUM_NT + i] = s_P[i] / sum;
    f_nt[(size_t)b * C2D_SU_NUM_NT + i] = s_f[i] / sum;
  }
}

}  // namespace c2d

namespace {

/* 0, C2D_E_ARG for a value <= 0, C2D_E_NONFINITE for a NaN or Inf */
int check_positive(const double* v, int64_t n) {
  int rc = C2D_OK;
  for (int64_t i = 0; i < n; i++) {
    if (!std::isfinite(v[i])) return C2D_E_NONFINITE;
    if (!(v[i] > 0.0)) rc = C2D_E_ARG;
  }
  return rc;
}
int check_finite(const double* v, int64_t n) {
  for (int64_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return C2D_E_NONFINITE;
  return C2D_OK;
}

int ic_loss_args(const double* gnt, int n_el, const double* E_field, int n_ph, const double* F_IC) {
  if (!gnt || !E_field || !F_IC) return C2D_E_ARG;
  if (n_el < 1 || n_el > C2D_NUM_NT || n_ph < 1 || n_ph > C2D_NPHFIELD) return C2D_E_ARG;
  int rc = check_positive(gnt, n_el);
  if (rc == C2D_E_NONFINITE) return rc;
  const int rc2 = check_positive(E_field, n_ph);
  return rc2 == C2D_E_NONFINITE ? rc2 : (rc ? rc : rc2);
}

int electrons_args(int64_t n, const double* const in[5], double* const out[5]) {
  for (int k = 0; k < 5; k++)
    if (!in[k] || !out[k]) return C2D_E_ARG;
  if (n < 1 || n > (int64_t)C2D_MAXZONE * C2D_MAXZONE) return C2D_E_ARG;
  for (int k = 0; k < 5; k++)
    if (check_finite(in[k], n)) return C2D_E_NONFINITE;
  /* tea, gmin, gmax > 0 (gmin and gmax are arguments of pow) */
  if (check_positive(in[0], n) || check_positive(in[2], n) || check_positive(in[3], n)) return C2D_E_ARG;
  return C2D_OK;
}

/* length of the ((n-1)/n)^2 table: every term of the longest series a valid
 * grid can hold; C2D_ICLOSS_TAB_N (environment, read at every call) shortens
 * it so that a test reaches the terms computed in place */
int icloss_tab_n() {
  int n = 78200;
  const char* e = getenv("C2D_ICLOSS_TAB_N");
  if (e && *e) {
    const long v = strtol(e, nullptr, 10);
    if (v >= 2 && v <= 1 << 20) n = (int)v;
  }
  return n;
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  template <class T>
  T* as() const { return (T*)p; }
};

}  // namespace

extern "C" int c2d_setup_grids(double* gnt, double* E_field, double* E_ph) {
  c2d_su_grids(gnt, E_field, E_ph);
  return C2D_OK;
}

extern "C" int c2d_ic_loss_host(const double* gnt, int n_el, const double* E_field, int n_ph,
                                double* F_IC, int64_t s_i, int64_t s_ph, int libm) {
  const int rc = ic_loss_args(gnt, n_el, E_field, n_ph, F_IC);
  if (rc) return rc;
  return c2d_su_ic_loss(gnt, n_el, E_field, n_ph, F_IC, s_i, s_ph, libm) ? C2D_E_FP : C2D_OK;
}

/* kernel_ms (may be null): HIP-event time of the series kernel */
extern "C" int c2d_ic_loss_timed(int device, const double* gnt, int n_el, const double* E_field,
                                 int n_ph, double* F_IC, int64_t s_i, int64_t s_ph, double* kernel_ms) {
  const int rc = ic_loss_args(gnt, n_el, E_field, n_ph, F_IC);
  if (rc) return rc;
  /* the waves, longest first: a series of argument z has about
   * min(7.8e4, 23 / log(1 + 2 z)) terms (sd_n <= y^-n, 1e-10 = e^-23) */
  struct Item {
    int i_el, p0, which;
    double cost;
  };
  std::vector<Item> items;
  for (int i = 0; i < n_el; i++)
    for (int p0 = 0; p0 < n_ph; p0 += c2d::SU_WAVE)
      for (int w = 0; w < 2; w++) {
        double cost = 0.0;
        for (int p = p0; p < std::min(n_ph, p0 + c2d::SU_WAVE); p++) {
          c2d_su_ic_entry e;
          if (!c2d_su_ic_args(gnt[i], E_field[p], &e)) continue;
          const double ly = log1p(2.0 * (w ? e.z2 : e.z1));
          cost = std::max(cost, ly > 0.0 ? std::min(7.8e4, 23.0 / ly) : 7.8e4);
        }
        if (cost > 0.0) items.push_back({i, p0, w, cost});
      }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.cost > b.cost; });
  std::vector<int> flat(3 * items.size());
  for (size_t k = 0; k < items.size(); k++) {
    flat[3 * k] = items[k].i_el;
    flat[3 * k + 1] = items[k].p0;
    flat[3 * k + 2] = items[k].which;
  }
  const int ntab = icloss_tab_n();
  std::vector<double> r2(ntab, 0.0);
  for (int n = 2; n < ntab; n++) {
    const double nn = (double)n;
    const double q = (nn - 1.0) / nn;
    r2[n] = q * q;
  }

  if (hipSetDevice(device) != hipSuccess) return C2D_E_HIP;
  const size_t ne = (size_t)n_el * n_ph;
  DevBuf d_items, d_gnt, d_E, d_r2, d_fli, d_F, d_err;
  if (d_items.alloc(flat.size() * sizeof(int)) != hipSuccess || d_gnt.alloc(n_el * sizeof(double)) != hipSuccess ||
      d_E.alloc(n_ph * sizeof(double)) != hipSuccess || d_r2.alloc(r2.size() * sizeof(double)) != hipSuccess ||
      d_fli.alloc(2 * ne * sizeof(double)) != hipSuccess || d_F.alloc(ne * sizeof(double)) != hipSuccess ||
      d_err.alloc(sizeof(int)) != hipSuccess)
    return C2D_E_HIP;
  if ((flat.size() && hipMemcpy(d_items.p, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(d_gnt.p, gnt, n_el * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_E.p, E_field, n_ph * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_r2.p, r2.data(), r2.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_fli.p, 0, 2 * ne * sizeof(double)) != hipSuccess || hipMemset(d_err.p, 0, sizeof(int)) != hipSuccess)
    return C2D_E_HIP;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (kernel_ms && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) return C2D_E_HIP;
  (void)hipGetLastError();
  if (kernel_ms) (void)hipEventRecord(ev0, 0);
  if (!items.empty())
    hipLaunchKernelGGL(c2d::c2d_icloss_kernel, dim3((unsigned)items.size()), dim3(c2d::SU_WAVE), 0, 0,
                       d_items.as<int>(), d_gnt.as<double>(), d_E.as<double>(), n_ph, d_r2.as<double>(), ntab,
                       d_fli.as<double>(), d_err.as<int>());
  if (kernel_ms) (void)hipEventRecord(ev1, 0);
  hipLaunchKernelGGL(c2d::c2d_icloss_finish_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, 0,
                     d_gnt.as<double>(), d_E.as<double>(), n_el, n_ph, d_fli.as<double>(), d_F.as<double>());
  int rc2 = C2D_OK;
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc2 = C2D_E_HIP;
  if (kernel_ms) {
    float ms = 0.f;
    if (!rc2 && hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) rc2 = C2D_E_HIP;
    *kernel_ms = ms;
    (void)hipEventDestroy(ev0);
    (void)hipEventDestroy(ev1);
  }
  if (rc2) return rc2;
  std::vector<double> F(ne);
  int err = 0;
  if (hipMemcpy(F.data(), d_F.p, ne * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return C2D_E_HIP;
  if (err) return C2D_E_FP;
  for (int i = 0; i < n_el; i++)
    for (int p = 0; p < n_ph; p++) F_IC[(int64_t)i * s_i + (int64_t)p * s_ph] = F[(size_t)i * n_ph + p];
  return C2D_OK;
}

extern "C" int c2d_ic_loss(int device, const double* gnt, int n_el, const double* E_field, int n_ph,
                           double* F_IC, int64_t s_i, int64_t s_ph) {
  return c2d_ic_loss_timed(device, gnt, n_el, E_field, n_ph, F_IC, s_i, s_ph, nullptr);
}

extern "C" int c2d_setup_electrons_host(int64_t n, const double* tea, const double* amxwl,
                                        const double* gmin, const double* gmax, const double* p_nth,
                                        double* gmin_out, double* N_nth, double* gbar_nth, double* f_nt,
                                        double* Pnt, int libm) {
  const double* const in[5] = {tea, amxwl, gmin, gmax, p_nth};
  double* const out[5] = {gmin_out, N_nth, gbar_nth, f_nt, Pnt};
  const int rc = electrons_args(n, in, out);
  if (rc) return rc;
  double gnt[C2D_SU_NUM_NT];
  c2d_su_grids(gnt, nullptr, nullptr);
  int capped = 0;
  for (int64_t b = 0; b < n; b++)
    capped |= c2d_su_electrons_zone(tea[b], amxwl[b], gmin[b], gmax[b], p_nth[b], gnt, libm, gmin_out + b,
                                    N_nth + b, gbar_nth + b, f_nt + b * C2D_SU_NUM_NT, Pnt + b * C2D_SU_NUM_NT);
  return capped ? C2D_E_FP : C2D_OK;
}

extern "C" int c2d_setup_electrons(int device, int64_t n, const double* tea, const double* amxwl,
                                   const double* gmin, const double* gmax, const double* p_nth,
                                   double* gmin_out, double* N_nth, double* gbar_nth, double* f_nt,
                                   double* Pnt) {
  const double* const in[5] = {tea, amxwl, gmin, gmax, p_nth};
  double* const out[5] = {gmin_out, N_nth, gbar_nth, f_nt, Pnt};
  const int rc = electrons_args(n, in, out);
  if (rc) return rc;
  double gnt[C2D_SU_NUM_NT];
  c2d_su_grids(gnt, nullptr, nullptr);
  const std::vector<double> mt = c2d_mcd_abscissae();
  std::vector<double> hin(5 * (size_t)n);
  for (int k = 0; k < 5; k++) std::copy(in[k], in[k] + n, hin.begin() + k * (size_t)n);

  if (hipSetDevice(device) != hipSuccess) return C2D_E_HIP;
  const size_t nb = (size_t)n * C2D_SU_NUM_NT;
  DevBuf d_in, d_gnt, d_mcd, d_scal, d_f, d_P, d_err;
  if (d_in.alloc(hin.size() * sizeof(double)) != hipSuccess || d_gnt.alloc(sizeof gnt) != hipSuccess ||
      d_mcd.alloc(mt.size() * sizeof(double)) != hipSuccess || d_scal.alloc(3 * n * sizeof(double)) != hipSuccess ||
      d_f.alloc(nb * sizeof(double)) != hipSuccess || d_P.alloc(nb * sizeof(double)) != hipSuccess ||
      d_err.alloc(sizeof(int)) != hipSuccess)
    return C2D_E_HIP;
  if (hipMemcpy(d_in.p, hin.data(), hin.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_gnt.p, gnt, sizeof gnt, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_mcd.p, mt.data(), mt.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_err.p, 0, sizeof(int)) != hipSuccess)
    return C2D_E_HIP;
  (void)hipGetLastError();
  hipLaunchKernelGGL(c2d::c2d_esetup_kernel, dim3((unsigned)n), dim3(c2d::SU_WAVE), 0, 0, (int)n,
                     d_in.as<double>(), d_gnt.as<double>(), d_mcd.as<double>(), d_scal.as<double>(),
                     d_f.as<double>(), d_P.as<double>(), d_err.as<int>());
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return C2D_E_HIP;
  std::vector<double> scal(3 * (size_t)n);
  int err = 0;
  if (hipMemcpy(scal.data(), d_scal.p, scal.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    return C2D_E_HIP;
  if (err) return C2D_E_FP;
  if (hipMemcpy(f_nt, d_f.p, nb * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(Pnt, d_P.p, nb * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return C2D_E_HIP;
  std::copy(scal.begin(), scal.begin() + n, gmin_out);
  std::copy(scal.begin() + n, scal.begin() + 2 * n, N_nth);
  std::copy(scal.begin() + 2 * n, scal.end(), gbar_nth);
  return C2D_OK;
}
