/*
 * censtext.hip — the census record file of write_cens / read_cens
 * (src/census2d.f:1-76) in both directions: plain records (d6, i5, key) to
 * the text and `<path>.keys`, formatted on the device by c2d_fmt.h and
 * c2d_censfmt.h, and the text back to plain records, parsed on the device by
 * c2d_scan.h and c2d_censfmt.h.  Both stream through two pinned host buffers
 * in chunks of C2D_CENSTEXT_CHUNK records.
 *
 * A record is 116 bytes: six E14.7 fields, a newline, six I5 fields, a
 * newline.  116 = 4 x 29: every record starts on a dword of the image, the
 * E fields on even bytes, the integer line one byte after a dword.  256
 * records are 29 696 B = 1 856 x 16 B, and a chunk starts 16-byte aligned in
 * device memory, so every workgroup's text is 16-byte aligned at its start;
 * the device text buffer is allocated to a multiple of 16 bytes and 16 bytes
 * beyond, the LDS image 16 bytes beyond the 29 696, so the last workgroup of
 * a chunk moves whole vectors too.
 *
 * Format kernel: one workgroup per 256 records.  One double per lane and
 * pass (record = i / 6, field = i % 6), its 14 bytes into the LDS image as
 * three dwords and a halfword; then one record per lane: the newline of the
 * first line, the 30 bytes of the integer line and its newline are eight
 * whole dwords of the image.  The image goes out as aligned 16-byte vectors.
 *
 * Parse kernel: the inverse.  Aligned 16-byte loads into the image, one E
 * field per lane and pass, then one integer line per lane with both
 * newlines.  A field or newline that is not canonical lowers the chunk's
 * first bad record and stores nothing.  Nothing is indexed by what the text
 * says: every address is a function of the record count alone.
 *
 * What the device does not take (the first record that is not canonical and
 * everything after it, or a tail shorter than a record) goes through a host
 * parser with read_census's rules (compton2d_amd/census_io.py): CR stripped,
 * blank lines skipped, fixed 14- and 5-column fields, the E-less three-digit
 * exponent repaired, D or a lower-case e as the exponent letter, a missing
 * final newline.
 */
#include "c2d_censtext.hpp"

#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/compton2d.h"
#include "c2d_censfmt.h"

namespace c2d {

struct CensStat {
  unsigned long long nonfinite;   /* write: NaN/Inf values met                                          */
  unsigned long long first_bad;   /* write: the smallest 6 * record + field among them;
                                     read: the first record of the chunk that is not canonical (~0: none) */
};

constexpr int CENS_IMG = C2D_CENS_BLOCK * C2D_CENS_RECORD;   /* 29 696 */
static_assert(CENS_IMG % 16 == 0 && C2D_CENS_RECORD % 4 == 0 && (C2D_CENS_LINE2 - 1) % 4 == 0,
              "the image's alignment rules (see the head of this file)");

__device__ __forceinline__ void cens_bad_value(CensStat* st, unsigned long long value_index) {
  atomicAdd(&st->nonfinite, 1ull);
  atomicMin(&st->first_bad, value_index);
}

/* NaN/Inf among the doubles of records [rec_base, rec_base + nrec) */
__global__ void __launch_bounds__(256) c2d_censscan_kernel(const uint64_t* __restrict__ d6, int64_t nrec,
                                                           int64_t rec_base, CensStat* st) {
  const int64_t nval = nrec * 6;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nval; i += (int64_t)gridDim.x * blockDim.x)
    if (((d6[i] >> 52) & 0x7ffu) == 0x7ffu) cens_bad_value(st, (unsigned long long)(rec_base * 6 + i));
}

__global__ void __launch_bounds__(C2D_CENS_BLOCK)
c2d_censtext_kernel(const double* __restrict__ d6, const int32_t* __restrict__ i5, const uint64_t* __restrict__ keys,
                    int64_t nrec, const c2d_fmt_tab* __restrict__ tab, unsigned char* __restrict__ out, CensStat* st) {
  __shared__ __attribute__((aligned(16))) unsigned char img[CENS_IMG + 16];
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * C2D_CENS_BLOCK;
  const int64_t left = nrec - r0;
  const int cnt = left < C2D_CENS_BLOCK ? (int)left : C2D_CENS_BLOCK;
  const double* src = d6 + r0 * 6;
  const int nval = cnt * 6;
  double xn = tid < nval ? __builtin_nontemporal_load(src + tid) : 0.0;
#pragma unroll 1
  for (int j = 0; j < 6; j++) {
    const int i = tid + C2D_CENS_BLOCK * j;
    if (i >= nval) break;
    const double x = xn;
    if (i + C2D_CENS_BLOCK < nval) xn = __builtin_nontemporal_load(src + i + C2D_CENS_BLOCK);
    uint64_t w0 = 0x2020202020202020ull, w1 = 0x202020202020ull;   /* a non-finite value: blanks */
    if (c2d_fmt_e14_7_pack(tab, x, &w0, &w1) == C2D_FMT_NONFINITE)
      cens_bad_value(st, (unsigned long long)(r0 * 6 + i));
    const int rec = i / 6, f = i - 6 * rec;
    /* 14 bytes V[0..14) at o, o even: a halfword before (o = 2 mod 4) or after three dwords */
    const unsigned __int128 V = (unsigned __int128)w0 | (unsigned __int128)(w1 & 0xffffffffffffull) << 64;
    const int o = rec * C2D_CENS_RECORD + 14 * f;
    const int h = o & 2;
    const unsigned __int128 M = h ? V >> 16 : V;
    uint32_t* d = reinterpret_cast<uint32_t*>(img + o + h);
    d[0] = (uint32_t)M;
    d[1] = (uint32_t)(M >> 32);
    d[2] = (uint32_t)(M >> 64);
    *reinterpret_cast<uint16_t*>(img + (h ? o : o + 12)) = h ? (uint16_t)V : (uint16_t)(V >> 96);
  }
  if (tid < cnt) {
    /* bytes 84..115 of the record: newline, six I5 fields, newline */
    const int32_t* q = i5 + (r0 + tid) * 5;
    const uint64_t key = keys[r0 + tid];
    uint32_t w[8] = {(uint32_t)'\n', 0u, 0u, 0u, 0u, 0u, 0u, (uint32_t)'\n' << 24};
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const uint64_t F = c2d_fmt_i5_pack(k < 5 ? (int64_t)q[k] : (int64_t)(key % C2D_CENS_SEEDMOD));
#pragma unroll
      for (int b = 0; b < 5; b++) {
        const int pos = 1 + 5 * k + b;
        w[pos >> 2] |= ((uint32_t)(F >> (8 * b)) & 0xffu) << (8 * (pos & 3));
      }
    }
    uint32_t* d = reinterpret_cast<uint32_t*>(img + tid * C2D_CENS_RECORD + C2D_CENS_LINE2 - 1);
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = w[k];
  }
  __syncthreads();
  /* whole vectors: the bytes past the text of a chunk's last workgroup land in the buffer's pad */
  const int nvec = (cnt * C2D_CENS_RECORD + 15) >> 4;
  const uint4* iv = reinterpret_cast<const uint4*>(img);
  uint4* ov = reinterpret_cast<uint4*>(out + r0 * C2D_CENS_RECORD);
  for (int v = tid; v < nvec; v += C2D_CENS_BLOCK) ov[v] = iv[v];
}

/* the 14 bytes at img + o as c2d_scan.h's two words */
__device__ __forceinline__ void cens_field(const unsigned char* img, int o, uint64_t* w0, uint64_t* w1) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(img + (o & ~3));
  const int sh = 8 * (o & 3);
  const uint64_t a = (uint64_t)w[0] | (uint64_t)w[1] << 32, b = (uint64_t)w[2] | (uint64_t)w[3] << 32;
  *w0 = sh ? (a >> sh) | (b << (64 - sh)) : a;
  *w1 = (b >> sh) & 0xffffffffffffull;   /* sh is 0 or 16: the six bytes lie in b */
}

__global__ void __launch_bounds__(C2D_CENS_BLOCK)
c2d_censparse_kernel(const unsigned char* __restrict__ text, int64_t nrec, int64_t rec_base,
                     const c2d_fmt_tab* __restrict__ tab, double* __restrict__ d6, int32_t* __restrict__ i5,
                     uint64_t* __restrict__ keys, int derive, CensStat* st, int force_exact) {
  __shared__ __attribute__((aligned(16))) unsigned char img[CENS_IMG + 16];
  __shared__ unsigned int wg_bad;
  const int tid = (int)threadIdx.x;
  if (tid == 0) wg_bad = 0xffffffffu;
  const int64_t r0 = (int64_t)blockIdx.x * C2D_CENS_BLOCK;
  const int64_t left = nrec - r0;
  const int cnt = left < C2D_CENS_BLOCK ? (int)left : C2D_CENS_BLOCK;
  const int nvec = (cnt * C2D_CENS_RECORD + 15) >> 4;   /* <= 1856; the buffer holds a multiple of 16 bytes */
  const uint4* src = reinterpret_cast<const uint4*>(text + r0 * C2D_CENS_RECORD);
  uint4* iv = reinterpret_cast<uint4*>(img);
  for (int v = tid; v < nvec; v += C2D_CENS_BLOCK) iv[v] = src[v];
  __syncthreads();
  const int nval = cnt * 6;
  uint64_t* dst = reinterpret_cast<uint64_t*>(d6) + r0 * 6;
  unsigned int bad = 0xffffffffu;
#pragma unroll 1
  for (int j = 0; j < 6; j++) {
    const int i = tid + C2D_CENS_BLOCK * j;
    if (i >= nval) break;
    const int rec = i / 6, f = i - 6 * rec;
    uint64_t w0, w1, bits;
    cens_field(img, rec * C2D_CENS_RECORD + 14 * f, &w0, &w1);
    if (c2d_scan_e14_7_pack_opt(tab, w0, w1, &bits, force_exact) < 0) bad = min(bad, (unsigned int)rec);
    else __builtin_nontemporal_store(bits, dst + i);
  }
  if (tid < cnt) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(img + tid * C2D_CENS_RECORD + C2D_CENS_LINE2 - 1);
    uint32_t x[8];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = w[k];
    int ok = (x[0] & 0xffu) == (uint32_t)'\n' && (x[7] >> 24) == (uint32_t)'\n';
    int32_t v[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 6; k++) {
      uint64_t F = 0;
#pragma unroll
      for (int b = 0; b < 5; b++) {
        const int pos = 1 + 5 * k + b;
        F |= (uint64_t)((x[pos >> 2] >> (8 * (pos & 3))) & 0xffu) << (8 * b);
      }
      ok &= c2d_scan_i5_pack(F, &v[k]) == 0;
    }
    if (!ok) {
      bad = min(bad, (unsigned int)tid);
    } else {
      int32_t* q = i5 + (r0 + tid) * 5;
#pragma unroll
      for (int k = 0; k < 5; k++) q[k] = v[k];
      if (derive) keys[r0 + tid] = c2d_cens_derive_key((int64_t)v[5], rec_base + r0 + tid);
    }
  }
  if (bad != 0xffffffffu) atomicMin(&wg_bad, bad);
  __syncthreads();
  if (tid == 0 && wg_bad != 0xffffffffu) atomicMin(&st->first_bad, (unsigned long long)(r0 + wg_bad));
}

/* the powers-of-ten table, built once per process */
static const c2d_fmt_tab* cens_tab() {
  static c2d_fmt_tab tab;
  static std::once_flag once;
  std::call_once(once, [] { c2d_fmt_tab_build(&tab); });
  return &tab;
}

}  // namespace c2d

using namespace c2d;

struct c2d_cens_file {
  int device = 0;
  c2d_fmt_tab* tab_d = nullptr;
  CensStat* stat_d = nullptr;
  CensStat* stat_h = nullptr;            /* pinned: [3], the last one the initial value */
  unsigned char* text_d = nullptr;       /* cap records of text, rounded up to 16 bytes and 16 beyond */
  double* d6_d = nullptr;                /* cap plain records */
  int32_t* i5_d = nullptr;
  uint64_t* keys_d = nullptr;
  unsigned char* pin[2] = {nullptr, nullptr};   /* pinned host staging: text ...  */
  uint64_t* kpin[2] = {nullptr, nullptr};       /* ... and keys, cap records each */
  int64_t cap = 0;
  hipEvent_t done[2] = {nullptr, nullptr}, ka[2] = {nullptr, nullptr}, kb[2] = {nullptr, nullptr},
             kc[2] = {nullptr, nullptr};
};

namespace {

int efail(char* err, size_t n, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (err && n) vsnprintf(err, n, fmt, ap);
  va_end(ap);
  return code;
}

#define CFCHK(x)                                                                              \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess)                                                                     \
      return efail(err, errlen, C2D_E_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
  } while (0)

/* records per chunk: C2D_CENSTEXT_CHUNK, read at every call (a test knob) */
int64_t chunk_records() {
  const char* e = getenv("C2D_CENSTEXT_CHUNK");
  if (e && *e) {
    const long long v = atoll(e);
    if (v >= 1) return (int64_t)std::min<long long>(v, 1ll << 24);
  }
  return (int64_t)1 << 20;
}

size_t text_bytes(int64_t records) { return (((size_t)records * C2D_CENS_RECORD + 15) & ~(size_t)15) + 16; }

int ensure(c2d_cens_file* w, int64_t records, char* err, size_t errlen) {
  if (!w->tab_d) {
    CFCHK(hipMalloc((void**)&w->tab_d, sizeof(c2d_fmt_tab)));
    CFCHK(hipMemcpy(w->tab_d, cens_tab(), sizeof(c2d_fmt_tab), hipMemcpyHostToDevice));
    CFCHK(hipMalloc((void**)&w->stat_d, sizeof(CensStat)));
    CFCHK(hipHostMalloc((void**)&w->stat_h, 3 * sizeof(CensStat), hipHostMallocDefault));
    for (int b = 0; b < 2; b++) {
      CFCHK(hipEventCreateWithFlags(&w->done[b], hipEventDisableTiming));
      CFCHK(hipEventCreate(&w->ka[b]));
      CFCHK(hipEventCreate(&w->kb[b]));
      CFCHK(hipEventCreate(&w->kc[b]));
    }
  }
  if (records > w->cap) {
    if (w->text_d) (void)hipFree(w->text_d);
    if (w->d6_d) (void)hipFree(w->d6_d);
    if (w->i5_d) (void)hipFree(w->i5_d);
    if (w->keys_d) (void)hipFree(w->keys_d);
    for (int b = 0; b < 2; b++) {
      if (w->pin[b]) (void)hipHostFree(w->pin[b]);
      if (w->kpin[b]) (void)hipHostFree(w->kpin[b]);
      w->pin[b] = nullptr;
      w->kpin[b] = nullptr;
    }
    w->text_d = nullptr;
    w->d6_d = nullptr;
    w->i5_d = nullptr;
    w->keys_d = nullptr;
    w->cap = 0;
    CFCHK(hipMalloc((void**)&w->text_d, text_bytes(records)));
    CFCHK(hipMemset(w->text_d, ' ', text_bytes(records)));   /* the pad is never parsed; keep it defined */
    CFCHK(hipMalloc((void**)&w->d6_d, (size_t)records * 6 * sizeof(double)));
    CFCHK(hipMalloc((void**)&w->i5_d, (size_t)records * 5 * sizeof(int32_t)));
    CFCHK(hipMalloc((void**)&w->keys_d, (size_t)records * sizeof(uint64_t)));
    for (int b = 0; b < 2; b++) {
      CFCHK(hipHostMalloc((void**)&w->pin[b], (size_t)records * C2D_CENS_RECORD, hipHostMallocDefault));
      CFCHK(hipHostMalloc((void**)&w->kpin[b], (size_t)records * sizeof(uint64_t), hipHostMallocDefault));
    }
    w->cap = records;
  }
  return C2D_OK;
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int nonfinite_error(unsigned long long count, unsigned long long first, char* err, size_t errlen) {
  return efail(err, errlen, C2D_E_NONFINITE,
               "census: %llu non-finite value(s); the first in record %llu (counted from 1), field %llu; "
               "the files were not touched", count, first / 6ull + 1ull, first % 6ull + 1ull);
}

/* records [c0, c0 + m) into the device arrays, on the stream */
int fill(c2d_cens_file* w, hipStream_t stream, c2d_cens_source src, void* user, const double* h_d6,
         const int32_t* h_i5, const uint64_t* h_keys, int64_t c0, int64_t m, char* err, size_t errlen) {
  if (src) return src(user, c0, m, w->d6_d, w->i5_d, w->keys_d);
  CFCHK(hipMemcpyAsync(w->d6_d, h_d6 + c0 * 6, (size_t)m * 6 * sizeof(double), hipMemcpyHostToDevice, stream));
  CFCHK(hipMemcpyAsync(w->i5_d, h_i5 + c0 * 5, (size_t)m * 5 * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  CFCHK(hipMemcpyAsync(w->keys_d, h_keys + c0, (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  return C2D_OK;
}

/* the chunks of [0, n) through the pinned buffers into the two files */
int write_chunks(c2d_cens_file* w, hipStream_t stream, c2d_cens_source src, void* user, const double* h_d6,
                 const int32_t* h_i5, const uint64_t* h_keys, int64_t n, int64_t chunk, FILE* f, FILE* fk,
                 const char* path, c2d_cens_times* T, char* err, size_t errlen) {
  const int64_t nchunks = (n + chunk - 1) / chunk;
  w->stat_h[2].nonfinite = 0ull;
  w->stat_h[2].first_bad = ~0ull;
  CFCHK(hipMemcpyAsync(w->stat_d, &w->stat_h[2], sizeof(CensStat), hipMemcpyHostToDevice, stream));
  for (int64_t k = 0; k <= nchunks; k++) {
    if (k < nchunks) {   /* chunk k: convert, format, copy to the pinned buffers k % 2 */
      const int b = (int)(k & 1);
      const int64_t c0 = k * chunk, m = std::min(n, c0 + chunk) - c0;
      CFCHK(hipEventRecord(w->kc[b], stream));
      { const int rc = fill(w, stream, src, user, h_d6, h_i5, h_keys, c0, m, err, errlen); if (rc) return rc; }
      CFCHK(hipEventRecord(w->ka[b], stream));
      hipLaunchKernelGGL(c2d_censtext_kernel, dim3((unsigned)((m + C2D_CENS_BLOCK - 1) / C2D_CENS_BLOCK)),
                         dim3(C2D_CENS_BLOCK), 0, stream, w->d6_d, w->i5_d, w->keys_d, m, w->tab_d, w->text_d,
                         w->stat_d);
      CFCHK(hipGetLastError());
      CFCHK(hipEventRecord(w->kb[b], stream));
      CFCHK(hipMemcpyAsync(w->pin[b], w->text_d, (size_t)m * C2D_CENS_RECORD, hipMemcpyDeviceToHost, stream));
      CFCHK(hipMemcpyAsync(w->kpin[b], w->keys_d, (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
      CFCHK(hipMemcpyAsync(&w->stat_h[b], w->stat_d, sizeof(CensStat), hipMemcpyDeviceToHost, stream));
      CFCHK(hipEventRecord(w->done[b], stream));
    }
    if (k > 0) {   /* chunk k - 1: to the files while chunk k is formatted and copied */
      const int b = (int)((k - 1) & 1);
      const int64_t c0 = (k - 1) * chunk, m = std::min(n, c0 + chunk) - c0;
      const double t0 = now_ms();
      CFCHK(hipEventSynchronize(w->done[b]));
      const double t1 = now_ms();
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, w->ka[b], w->kb[b]);
      T->kernel_ms += ms;
      if (src) {
        (void)hipEventElapsedTime(&ms, w->kc[b], w->ka[b]);
        T->conv_ms += ms;
      }
      T->wait_ms += t1 - t0;
      T->chunks++;
      if (w->stat_h[b].nonfinite)   /* the scan found none: the records changed under the call */
        return efail(err, errlen, C2D_E_STATE, "census: a non-finite value appeared while '%s' was written", path);
      const size_t bytes = (size_t)m * C2D_CENS_RECORD;
      if (fwrite(w->pin[b], 1, bytes, f) != bytes)
        return efail(err, errlen, C2D_E_IO, "census: cannot write '%s': %s", path, strerror(errno));
      if (fwrite(w->kpin[b], sizeof(uint64_t), (size_t)m, fk) != (size_t)m)
        return efail(err, errlen, C2D_E_IO, "census: cannot write '%s.keys': %s", path, strerror(errno));
      T->io_ms += now_ms() - t1;
    }
  }
  return C2D_OK;
}

/* NaN/Inf in the records, before either file is opened */
int scan_records(c2d_cens_file* w, hipStream_t stream, c2d_cens_source src, void* user, const double* h_d6,
                 int64_t n, int64_t chunk, c2d_cens_times* T, char* err, size_t errlen) {
  if (!src) {
    const uint64_t* u = reinterpret_cast<const uint64_t*>(h_d6);
    unsigned long long bad = 0, first = 0;
    for (int64_t i = 0; i < 6 * n; i++)
      if (((u[i] >> 52) & 0x7ffu) == 0x7ffu && bad++ == 0) first = (unsigned long long)i;
    return bad ? nonfinite_error(bad, first, err, errlen) : C2D_OK;
  }
  w->stat_h[2].nonfinite = 0ull;
  w->stat_h[2].first_bad = ~0ull;
  CFCHK(hipMemcpyAsync(w->stat_d, &w->stat_h[2], sizeof(CensStat), hipMemcpyHostToDevice, stream));
  CFCHK(hipEventRecord(w->kc[0], stream));
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t m = std::min(chunk, n - c0);
    { const int rc = src(user, c0, m, w->d6_d, w->i5_d, w->keys_d); if (rc) return rc; }
    const unsigned grid = (unsigned)std::min<int64_t>((6 * m + 255) / 256, 4096);
    hipLaunchKernelGGL(c2d_censscan_kernel, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const uint64_t*>(w->d6_d), m, c0, w->stat_d);
    CFCHK(hipGetLastError());
  }
  CFCHK(hipEventRecord(w->ka[0], stream));
  CFCHK(hipMemcpyAsync(&w->stat_h[0], w->stat_d, sizeof(CensStat), hipMemcpyDeviceToHost, stream));
  CFCHK(hipStreamSynchronize(stream));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, w->kc[0], w->ka[0]);
  T->conv_ms += ms;
  if (w->stat_h[0].nonfinite) return nonfinite_error(w->stat_h[0].nonfinite, w->stat_h[0].first_bad, err, errlen);
  return C2D_OK;
}

int close_both(FILE* f, FILE* fk, int rc, const char* path, char* err, size_t errlen) {
  const int c1 = fclose(f), c2 = fclose(fk);
  if ((c1 != 0 || c2 != 0) && !rc)
    rc = efail(err, errlen, C2D_E_IO, "census: cannot close '%s' or its .keys: %s", path, strerror(errno));
  return rc;
}

}  // namespace

extern "C" int c2d_censtext_write(c2d_cens_file** pw, int device, hipStream_t stream, c2d_cens_source src, void* user,
                                  const double* h_d6, const int32_t* h_i5, const uint64_t* h_keys, int64_t n,
                                  const char* path, c2d_cens_times* times, char* err, size_t errlen) {
  c2d_cens_times T = {};
  const std::string kpath = std::string(path) + ".keys";
  const int64_t chunk = chunk_records();
  if (n > 0) {
    if (!*pw) {
      *pw = new c2d_cens_file;
      (*pw)->device = device;
    }
    c2d_cens_file* w = *pw;
    { const int rc = ensure(w, std::min(chunk, n), err, errlen); if (rc) return rc; }
    { const int rc = scan_records(w, stream, src, user, h_d6, n, chunk, &T, err, errlen);
      if (rc) { (void)hipStreamSynchronize(stream); return rc; } }
  }
  FILE* f = fopen(path, "wb");
  if (!f) return efail(err, errlen, C2D_E_IO, "census: cannot open '%s': %s", path, strerror(errno));
  FILE* fk = fopen(kpath.c_str(), "wb");
  if (!fk) {
    const int e = errno;
    (void)fclose(f);
    return efail(err, errlen, C2D_E_IO, "census: cannot open '%s': %s", kpath.c_str(), strerror(e));
  }
  setvbuf(f, nullptr, _IONBF, 0);   /* the chunks are the buffer */
  setvbuf(fk, nullptr, _IONBF, 0);
  int rc = C2D_OK;
  if (n > 0) {
    rc = write_chunks(*pw, stream, src, user, h_d6, h_i5, h_keys, n, chunk, f, fk, path, &T, err, errlen);
    if (rc) (void)hipStreamSynchronize(stream);   /* nothing in flight into the staging buffers */
  }
  rc = close_both(f, fk, rc, path, err, errlen);
  if (times) *times = T;
  return rc;
}

namespace {

/* up to `want` bytes, short only at the end of the file; -1 on error */
int64_t read_full(int fd, void* buf, int64_t want) {
  int64_t got = 0;
  while (got < want) {
    const ssize_t k = read(fd, (unsigned char*)buf + got, (size_t)std::min<int64_t>(want - got, (int64_t)1 << 30));
    if (k < 0) {
      if (errno == EINTR) continue;
      return -1;
    }
    if (k == 0) break;
    got += k;
  }
  return got;
}

bool is_blank(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

/* columns [a, a + width) of the line without the blanks around them */
void columns(const std::string& s, size_t a, size_t width, const char** t, int* len) {
  size_t lo = std::min(a, s.size()), hi = std::min(a + width, s.size());
  while (lo < hi && is_blank((unsigned char)s[lo])) lo++;
  while (hi > lo && is_blank((unsigned char)s[hi - 1])) hi--;
  *t = s.data() + lo;
  *len = (int)(hi - lo);
}

/* one E field: the canonical field with its pad restored, else the E-less
 * exponent repaired, D or d as the exponent letter, and strtod of all of it */
bool double_field(const char* t, int len, double* v) {
  char f[24];
  if (len < 1 || len > 14) return false;
  if (len == 14 && t[0] == '-') {
    memcpy(f, t, 14);
    if (c2d_scan_e14_7(cens_tab(), f, v) >= 0) return true;
  } else if (len == 13) {
    f[0] = ' ';
    memcpy(f + 1, t, 13);
    if (c2d_scan_e14_7(cens_tab(), f, v) >= 0) return true;
  }
  int n = 0, last_sign = -1;
  bool has_e = false;
  for (int i = 0; i < len; i++) {
    char c = t[i];
    if (c == 'D' || c == 'd') c = 'E';
    if (c == 'E' || c == 'e') has_e = true;
    if ((c == '+' || c == '-') && i > 0) last_sign = n;
    f[n++] = c;
  }
  if (!has_e && last_sign > 0) {
    memmove(f + last_sign + 1, f + last_sign, (size_t)(n - last_sign));
    f[last_sign] = 'E';
    n++;
  }
  f[n] = 0;
  char* end = nullptr;
  *v = strtod(f, &end);
  return end == f + n;
}

/* one I5 field: an optional sign and digits */
bool int_field(const char* t, int len, int32_t* v) {
  int i = 0;
  bool neg = false;
  if (len > 0 && (t[0] == '-' || t[0] == '+')) { neg = t[0] == '-'; i = 1; }
  if (i >= len || len > 10) return false;
  int64_t a = 0;
  for (; i < len; i++) {
    if (t[i] < '0' || t[i] > '9') return false;
    a = a * 10 + (t[i] - '0');
  }
  *v = (int32_t)(neg ? -a : a);
  return true;
}

struct HostParse {
  std::vector<double> d6;
  std::vector<int32_t> i5;
  std::vector<int64_t> seed;
  std::vector<uint64_t> keys;
  int64_t cap;          /* records per delivery */
  int kfd;              /* the keys file, or -1 */
  c2d_cens_sink sink;
  void* user;
  int64_t* delivered;
  c2d_cens_times* T;
  const char* path;
  int flush(char* err, size_t errlen) {
    const int64_t n = (int64_t)seed.size();
    if (n == 0) return C2D_OK;
    keys.resize((size_t)n);
    if (kfd >= 0) {
      int64_t got = 0;
      while (got < 8 * n) {
        const ssize_t k = pread(kfd, (unsigned char*)keys.data() + got, (size_t)(8 * n - got),
                                (off_t)(8 * *delivered + got));
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) break;
        got += k;
      }
      if (got != 8 * n)
        return efail(err, errlen, C2D_E_IO, "census: '%s.keys' holds fewer keys than '%s' has records", path, path);
    } else {
      for (int64_t r = 0; r < n; r++) keys[(size_t)r] = c2d_cens_derive_key(seed[(size_t)r], *delivered + r);
    }
    const int rc = sink ? sink(user, d6.data(), i5.data(), keys.data(), n, 0) : C2D_OK;
    if (rc) return rc;
    *delivered += n;
    T->host_records += n;
    d6.clear();
    i5.clear();
    seed.clear();
    return C2D_OK;
  }
};

/* the host parser from byte `off` (the start of a record) to the end of the file */
int host_parse(int fd, int kfd, int64_t off, int64_t chunk, c2d_cens_sink sink, void* user, int64_t* delivered,
               c2d_cens_times* T, const char* path, char* err, size_t errlen) {
  if (lseek(fd, (off_t)off, SEEK_SET) < 0)
    return efail(err, errlen, C2D_E_IO, "census: cannot seek in '%s': %s", path, strerror(errno));
  HostParse H{{}, {}, {}, {}, chunk, kfd, sink, user, delivered, T, path};
  std::vector<unsigned char> buf((size_t)1 << 20);
  std::string line, first;
  int64_t pos = off, line_off = off, first_off = 0;
  bool have_first = false;
  int rc = C2D_OK;
  for (bool eof = false; !eof && !rc;) {
    const int64_t got = read_full(fd, buf.data(), (int64_t)buf.size());
    if (got < 0) return efail(err, errlen, C2D_E_IO, "census: cannot read '%s': %s", path, strerror(errno));
    eof = got < (int64_t)buf.size();
    for (int64_t i = 0; i <= got && !rc; i++) {
      const bool end_of_text = i == got;
      if (end_of_text && !eof) break;
      if (!end_of_text && buf[(size_t)i] != '\n') {
        if (line.empty()) line_off = pos + i;
        if (line.size() < 4096) line.push_back((char)buf[(size_t)i]);
        continue;
      }
      /* a line ends here (or the text does: a missing final newline) */
      bool blank = true;
      for (char c : line) blank = blank && is_blank((unsigned char)c);
      if (blank) { line.clear(); continue; }
      if (!have_first) {
        first.swap(line);
        first_off = line_off;
        have_first = true;
        line.clear();
        continue;
      }
      have_first = false;
      const char* t;
      int len;
      for (int c = 0; c < 6 && !rc; c++) {
        double v = 0.0;
        columns(first, 14 * (size_t)c, 14, &t, &len);
        if (!double_field(t, len, &v))
          rc = efail(err, errlen, C2D_E_IO, "census: '%s': field '%.*s' at byte offset %lld is not a number", path, len,
                     t, (long long)(first_off + 14 * c));
        H.d6.push_back(v);
      }
      for (int c = 0; c < 6 && !rc; c++) {
        int32_t v = 0;
        columns(line, 5 * (size_t)c, 5, &t, &len);
        if (!int_field(t, len, &v))
          rc = efail(err, errlen, C2D_E_IO, "census: '%s': field '%.*s' at byte offset %lld is not an integer", path,
                     len, t, (long long)(line_off + 5 * c));
        if (c < 5) H.i5.push_back(v); else H.seed.push_back(v);
      }
      line.clear();
      if (!rc && (int64_t)H.seed.size() >= H.cap) rc = H.flush(err, errlen);
    }
    pos += got;
  }
  if (!rc && have_first)
    rc = efail(err, errlen, C2D_E_IO, "census: '%s': an odd number of lines: the record at byte offset %lld has no "
               "integer line", path, (long long)first_off);
  if (!rc) rc = H.flush(err, errlen);
  return rc;
}

/* chunk of `n` records in pin[b] (and kpin[b]) -> device text -> plain records */
int enqueue(c2d_cens_file* r, hipStream_t stream, int b, int64_t n, int64_t rec_base, bool have_keys, char* err,
            size_t errlen) {
  CFCHK(hipMemcpyAsync(r->text_d, r->pin[b], (size_t)n * C2D_CENS_RECORD, hipMemcpyHostToDevice, stream));
  if (have_keys)
    CFCHK(hipMemcpyAsync(r->keys_d, r->kpin[b], (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  const char* e = getenv("C2D_SCAN_SELFTEST_EXACT");
  CFCHK(hipEventRecord(r->ka[b], stream));
  hipLaunchKernelGGL(c2d_censparse_kernel, dim3((unsigned)((n + C2D_CENS_BLOCK - 1) / C2D_CENS_BLOCK)),
                     dim3(C2D_CENS_BLOCK), 0, stream, r->text_d, n, rec_base, r->tab_d, r->d6_d, r->i5_d, r->keys_d,
                     have_keys ? 0 : 1, r->stat_d, e && e[0] == '1');
  CFCHK(hipGetLastError());
  CFCHK(hipEventRecord(r->kb[b], stream));
  CFCHK(hipMemcpyAsync(&r->stat_h[b], r->stat_d, sizeof(CensStat), hipMemcpyDeviceToHost, stream));
  CFCHK(hipEventRecord(r->done[b], stream));
  return C2D_OK;
}

int read_chunks(c2d_cens_file* r, hipStream_t stream, int fd, int kfd, const char* path, int64_t chunk,
                c2d_cens_sink sink, void* user, int64_t* delivered, c2d_cens_times* T, char* err, size_t errlen) {
  const int64_t chunk_bytes = chunk * C2D_CENS_RECORD;
  r->stat_h[2].nonfinite = 0ull;
  r->stat_h[2].first_bad = ~0ull;
  CFCHK(hipMemcpyAsync(r->stat_d, &r->stat_h[2], sizeof(CensStat), hipMemcpyHostToDevice, stream));
  bool eof = false;
  int64_t prev_n = 0, prev_base = 0;   /* the chunk in flight: its records and its byte offset */
  int64_t nkeys[2] = {0, 0};           /* keys read beside each chunk (fewer than its 116-byte slots
                                          where the text is not canonical, or the keys file is short) */
  int prev_b = 0;
  int64_t host_off = -1;               /* where the host parser takes over */
  for (int64_t k = 0;; k++) {
    const int b = (int)(k & 1);
    int64_t cur_n = 0;
    if (!eof) {   /* chunk k into the pinned buffers b while chunk k - 1 is copied and parsed */
      const double t0 = now_ms();
      const int64_t got = read_full(fd, r->pin[b], chunk_bytes);
      if (got < 0) return efail(err, errlen, C2D_E_IO, "census: cannot read '%s': %s", path, strerror(errno));
      cur_n = got / C2D_CENS_RECORD;
      eof = got < chunk_bytes;
      if (got % C2D_CENS_RECORD) host_off = k * chunk_bytes + cur_n * C2D_CENS_RECORD;   /* a tail shorter than a record */
      if (kfd >= 0 && cur_n > 0) {
        const int64_t kgot = read_full(kfd, r->kpin[b], 8 * cur_n);
        if (kgot < 0) return efail(err, errlen, C2D_E_IO, "census: cannot read '%s.keys': %s", path, strerror(errno));
        nkeys[b] = kgot / 8;
      }
      T->io_ms += now_ms() - t0;
    }
    if (prev_n > 0) {   /* chunk k - 1 to the sink */
      const double t0 = now_ms();
      CFCHK(hipEventSynchronize(r->done[prev_b]));
      T->wait_ms += now_ms() - t0;
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, r->ka[prev_b], r->kb[prev_b]);
      T->kernel_ms += ms;
      T->chunks++;
      const unsigned long long fb = r->stat_h[prev_b].first_bad;
      const int64_t good = fb < (unsigned long long)prev_n ? (int64_t)fb : prev_n;
      if (kfd >= 0 && good > nkeys[prev_b])
        return efail(err, errlen, C2D_E_IO, "census: '%s.keys' holds fewer keys than '%s' has records", path, path);
      if (good > 0 && sink) {
        const int rc = sink(user, r->d6_d, r->i5_d, r->keys_d, good, 1);
        if (rc) return rc;
      }
      *delivered += good;
      T->device_records += good;
      if (good < prev_n) {   /* not canonical from here on: the host parser's */
        host_off = prev_base + good * C2D_CENS_RECORD;
        break;
      }
      prev_n = 0;
    }
    if (cur_n > 0) {
      const int rc = enqueue(r, stream, b, cur_n, k * chunk, kfd >= 0, err, errlen);
      if (rc) return rc;
      prev_n = cur_n;
      prev_b = b;
      prev_base = k * chunk_bytes;
    }
    if (eof && prev_n == 0) break;
  }
  if (host_off >= 0) return host_parse(fd, kfd, host_off, chunk, sink, user, delivered, T, path, err, errlen);
  return C2D_OK;
}

}  // namespace

extern "C" int c2d_censtext_read(c2d_cens_file** pr, int device, hipStream_t stream, const char* path,
                                 c2d_cens_sink sink, void* user, int64_t* n_records, c2d_cens_times* times,
                                 char* err, size_t errlen) {
  c2d_cens_times T = {};
  int64_t delivered = 0;
  if (n_records) *n_records = 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return efail(err, errlen, C2D_E_IO, "census: cannot open '%s': %s", path, strerror(errno));
  const std::string kpath = std::string(path) + ".keys";
  const int kfd = open(kpath.c_str(), O_RDONLY);
  if (kfd < 0 && errno != ENOENT) {
    const int e = errno;
    (void)close(fd);
    return efail(err, errlen, C2D_E_IO, "census: cannot open '%s': %s", kpath.c_str(), strerror(e));
  }
  int64_t chunk = chunk_records();
  struct stat sb;
  if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode))   /* a small file needs small buffers */
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, (int64_t)sb.st_size / C2D_CENS_RECORD));
  if (!*pr) {
    *pr = new c2d_cens_file;
    (*pr)->device = device;
  }
  int rc = ensure(*pr, chunk, err, errlen);
  if (!rc) {
    rc = read_chunks(*pr, stream, fd, kfd, path, chunk, sink, user, &delivered, &T, err, errlen);
    if (rc) (void)hipStreamSynchronize(stream);   /* nothing in flight out of the staging buffers */
  }
  if (!rc && kfd >= 0 && fstat(kfd, &sb) == 0 && (int64_t)sb.st_size != 8 * delivered)
    rc = efail(err, errlen, C2D_E_IO, "census: '%s' holds %lld bytes, '%s' %lld records (8 bytes a key)",
               kpath.c_str(), (long long)sb.st_size, path, (long long)delivered);
  (void)close(fd);
  if (kfd >= 0) (void)close(kfd);
  if (n_records) *n_records = delivered;
  if (times) *times = T;
  return rc;
}

extern "C" void c2d_censtext_free(c2d_cens_file* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  if (w->tab_d) (void)hipFree(w->tab_d);
  if (w->stat_d) (void)hipFree(w->stat_d);
  if (w->stat_h) (void)hipHostFree(w->stat_h);
  if (w->text_d) (void)hipFree(w->text_d);
  if (w->d6_d) (void)hipFree(w->d6_d);
  if (w->i5_d) (void)hipFree(w->i5_d);
  if (w->keys_d) (void)hipFree(w->keys_d);
  for (int b = 0; b < 2; b++) {
    if (w->pin[b]) (void)hipHostFree(w->pin[b]);
    if (w->kpin[b]) (void)hipHostFree(w->kpin[b]);
    if (w->done[b]) (void)hipEventDestroy(w->done[b]);
    if (w->ka[b]) (void)hipEventDestroy(w->ka[b]);
    if (w->kb[b]) (void)hipEventDestroy(w->kb[b]);
    if (w->kc[b]) (void)hipEventDestroy(w->kc[b]);
  }
  delete w;
}
