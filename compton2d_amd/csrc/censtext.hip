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
 * everything after it, or a tail shorter than a record) goes through the host
 * parser of c2d_textparse.hpp with read_census's rules (compton2d_amd/census_io.py): CR stripped,
 * blank lines skipped, fixed 14- and 5-column fields, the E-less three-digit
 * exponent repaired, D or a lower-case e as the exponent letter, a missing
 * final newline.
 */
#include "c2d_censtext.hpp"

#include <fcntl.h>
#include <sys/stat.h>

#include "c2d_textio.hpp"

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

}  // namespace c2d

using namespace c2d;

struct c2d_cens_file {
  TextStage<CensStat> st;                /* the text padded: both kernels move whole 16-byte vectors */
  double* d6_d = nullptr;                /* cap plain records */
  int32_t* i5_d = nullptr;
  uint64_t* keys_d = nullptr;
  uint64_t* kpin[2] = {nullptr, nullptr};   /* pinned host staging of the keys, cap records each */
  hipEvent_t kc[2] = {nullptr, nullptr};    /* before a chunk's conversion */
};

namespace {

constexpr CensStat CENS_STAT0 = {0ull, ~0ull};   /* nothing met yet */

void free_records(c2d_cens_file* w) {
  if (w->d6_d) (void)hipFree(w->d6_d);
  if (w->i5_d) (void)hipFree(w->i5_d);
  if (w->keys_d) (void)hipFree(w->keys_d);
  w->d6_d = nullptr;
  w->i5_d = nullptr;
  w->keys_d = nullptr;
  for (int b = 0; b < 2; b++) {
    if (w->kpin[b]) (void)hipHostFree(w->kpin[b]);
    w->kpin[b] = nullptr;
  }
}

/* the file's stage on first use, with room for `records` */
int ensure(c2d_cens_file** pw, int device, int64_t records, char* err, size_t errlen) {
  if (!*pw) {
    *pw = new c2d_cens_file;
    (*pw)->st.device = device;
  }
  c2d_cens_file* w = *pw;
  for (int b = 0; b < 2; b++)
    if (!w->kc[b]) C2D_TXCHK(hipEventCreate(&w->kc[b]));
  return w->st.ensure(records, C2D_CENS_RECORD, true, [&](int64_t n) {
    free_records(w);
    C2D_TXCHK(hipMalloc((void**)&w->d6_d, (size_t)n * 6 * sizeof(double)));
    C2D_TXCHK(hipMalloc((void**)&w->i5_d, (size_t)n * 5 * sizeof(int32_t)));
    C2D_TXCHK(hipMalloc((void**)&w->keys_d, (size_t)n * sizeof(uint64_t)));
    for (int b = 0; b < 2; b++)
      C2D_TXCHK(hipHostMalloc((void**)&w->kpin[b], (size_t)n * sizeof(uint64_t), hipHostMallocDefault));
    return C2D_OK;
  }, err, errlen);
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
  C2D_TXCHK(hipMemcpyAsync(w->d6_d, h_d6 + c0 * 6, (size_t)m * 6 * sizeof(double), hipMemcpyHostToDevice, stream));
  C2D_TXCHK(hipMemcpyAsync(w->i5_d, h_i5 + c0 * 5, (size_t)m * 5 * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  C2D_TXCHK(hipMemcpyAsync(w->keys_d, h_keys + c0, (size_t)m * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
  return C2D_OK;
}

/* the chunks of [0, n) through the pinned buffers into the two files */
int write_records(c2d_cens_file* w, hipStream_t stream, c2d_cens_source src, void* user, const double* h_d6,
                  const int32_t* h_i5, const uint64_t* h_keys, int64_t n, int64_t chunk, FILE* f, FILE* fk,
                  const char* path, c2d_cens_times* T, char* err, size_t errlen) {
  TextStage<CensStat>& st = w->st;
  auto produce = [&](int b, int64_t c0, int64_t m) {   /* convert, format */
    C2D_TXCHK(hipEventRecord(w->kc[b], stream));
    { const int rc = fill(w, stream, src, user, h_d6, h_i5, h_keys, c0, m, err, errlen); if (rc) return rc; }
    return st.timed(stream, b, [&] {
      hipLaunchKernelGGL(c2d_censtext_kernel, dim3((unsigned)((m + C2D_CENS_BLOCK - 1) / C2D_CENS_BLOCK)),
                         dim3(C2D_CENS_BLOCK), 0, stream, w->d6_d, w->i5_d, w->keys_d, m, st.tab_d, st.text_d,
                         st.stat_d);
    }, err, errlen);
  };
  auto copy_out = [&](int b, int64_t m) {
    C2D_TXCHK(hipMemcpyAsync(w->kpin[b], w->keys_d, (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    return C2D_OK;
  };
  auto counts = [&](int b) {
    float ms = 0.f;
    if (src) {
      (void)hipEventElapsedTime(&ms, w->kc[b], st.ka[b]);
      T->conv_ms += ms;
    }
  };
  auto write_side = [&](int b, int64_t m) {
    if (fwrite(w->kpin[b], sizeof(uint64_t), (size_t)m, fk) != (size_t)m)
      return efail(err, errlen, C2D_E_IO, "census: cannot write '%s.keys': %s", path, strerror(errno));
    return C2D_OK;
  };
  return write_chunks(st, stream, f, "census", path, C2D_CENS_RECORD, n, chunk, CENS_STAT0, T, produce, copy_out,
                      counts, write_side, err, errlen);
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
  TextStage<CensStat>& st = w->st;
  { const int rc = st.reset(stream, CENS_STAT0, err, errlen); if (rc) return rc; }
  C2D_TXCHK(hipEventRecord(w->kc[0], stream));
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t m = std::min(chunk, n - c0);
    { const int rc = src(user, c0, m, w->d6_d, w->i5_d, w->keys_d); if (rc) return rc; }
    const unsigned grid = (unsigned)std::min<int64_t>((6 * m + 255) / 256, 4096);
    hipLaunchKernelGGL(c2d_censscan_kernel, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const uint64_t*>(w->d6_d), m, c0, st.stat_d);
    C2D_TXCHK(hipGetLastError());
  }
  C2D_TXCHK(hipEventRecord(st.ka[0], stream));
  C2D_TXCHK(hipMemcpyAsync(&st.stat_h[0], st.stat_d, sizeof(CensStat), hipMemcpyDeviceToHost, stream));
  C2D_TXCHK(hipStreamSynchronize(stream));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, w->kc[0], st.ka[0]);
  T->conv_ms += ms;
  if (st.stat_h[0].nonfinite) return nonfinite_error(st.stat_h[0].nonfinite, st.stat_h[0].first_bad, err, errlen);
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
  const int64_t chunk = chunk_env("C2D_CENSTEXT_CHUNK", 1ll << 24);
  if (n > 0) {
    { const int rc = ensure(pw, device, std::min(chunk, n), err, errlen); if (rc) return rc; }
    { const int rc = scan_records(*pw, stream, src, user, h_d6, n, chunk, &T, err, errlen);
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
    rc = write_records(*pw, stream, src, user, h_d6, h_i5, h_keys, n, chunk, f, fk, path, &T, err, errlen);
    if (rc) (void)hipStreamSynchronize(stream);   /* nothing in flight into the staging buffers */
  }
  rc = close_both(f, fk, rc, path, err, errlen);
  if (times) *times = T;
  return rc;
}

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
  int64_t chunk = chunk_env("C2D_CENSTEXT_CHUNK", 1ll << 24);
  struct stat sb;
  if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode))   /* a small file needs small buffers */
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, (int64_t)sb.st_size / C2D_CENS_RECORD));
  int rc = ensure(pr, device, chunk, err, errlen);
  if (!rc) {
    c2d_cens_file* r = *pr;
    TextStage<CensStat>& st = r->st;
    int64_t nkeys[2] = {0, 0};   /* keys read beside each chunk (fewer than its 116-byte slots where the
                                    text is not canonical, or the keys file is short) */
    const char* e = getenv("C2D_SCAN_SELFTEST_EXACT");
    const int force_exact = e && e[0] == '1';
    auto side = [&](int b, int64_t n) {
      if (kfd < 0) return C2D_OK;
      const int64_t kgot = read_full(kfd, r->kpin[b], 8 * n);
      if (kgot < 0) return efail(err, errlen, C2D_E_IO, "census: cannot read '%s.keys': %s", path, strerror(errno));
      nkeys[b] = kgot / 8;
      return C2D_OK;
    };
    /* chunk k of n records (its keys in kpin[b]): device text -> plain records */
    auto enqueue = [&](int b, int64_t n, int64_t k) {
      if (kfd >= 0)
        C2D_TXCHK(hipMemcpyAsync(r->keys_d, r->kpin[b], (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
      return st.timed(stream, b, [&] {
        hipLaunchKernelGGL(c2d_censparse_kernel, dim3((unsigned)((n + C2D_CENS_BLOCK - 1) / C2D_CENS_BLOCK)),
                           dim3(C2D_CENS_BLOCK), 0, stream, st.text_d, n, k * chunk, st.tab_d, r->d6_d, r->i5_d,
                           r->keys_d, kfd >= 0 ? 0 : 1, st.stat_d, force_exact);
      }, err, errlen);
    };
    auto deliver = [&](int b, int64_t good) {
      if (kfd >= 0 && good > nkeys[b])
        return efail(err, errlen, C2D_E_IO, "census: '%s.keys' holds fewer keys than '%s' has records", path, path);
      if (good > 0 && sink) {
        const int rc = sink(user, r->d6_d, r->i5_d, r->keys_d, good, 1);
        if (rc) return rc;
      }
      delivered += good;
      T.device_records += good;
      return C2D_OK;
    };
    auto host = [&](int64_t off) {
      return cens_host_parse(fd, kfd, off, chunk, sink, user, &delivered, &T, path, err, errlen);
    };
    rc = read_chunks(st, stream, fd, "census", path, C2D_CENS_RECORD, chunk, CENS_STAT0, &T, side, enqueue, deliver,
                     host, err, errlen);
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
  (void)hipSetDevice(w->st.device);
  w->st.release();
  free_records(w);
  for (int b = 0; b < 2; b++)
    if (w->kc[b]) (void)hipEventDestroy(w->kc[b]);
  delete w;
}
