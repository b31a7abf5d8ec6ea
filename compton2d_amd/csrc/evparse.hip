/*
 * evparse.hip — the text of p###_evb.dat (src/imcleak2d.f:181: 6(e14.7,1x),
 * e14.7, 105 bytes a record) back to escape events (AoS 7 x f64 in device
 * memory): the inverse of evtext.hip.  The file is read into two pinned host
 * buffers in turn, copied to the device and parsed there by c2d_scan.h.
 *
 * Kernel: one workgroup per 256 records.  A chunk starts 16-byte aligned in
 * device memory and 256 records are 26 880 B = 1 680 x 16 B, so every
 * workgroup stages its text into LDS with aligned 16-byte loads.  Then one
 * field per lane and pass (record = i / 7, field = i % 7): the 15 bytes of
 * the field and its separator come out of five aligned LDS dwords whatever
 * the field's alignment, the separator is checked (a blank, or a newline
 * after the seventh field), the field is parsed and the double stored at
 * out[i]: consecutive lanes store consecutive doubles.  A field or separator
 * that is not canonical lowers the chunk's first bad record (one LDS
 * atomicMin per lane, one global one per workgroup) and stores nothing.  The
 * multi-limb path of the parser is a call (noinline) with rolled loops.
 *
 * Nothing is indexed by what the text says: every address is a function of
 * the record count alone, the text buffer is allocated to a multiple of 16
 * bytes beyond its length and the LDS image 16 bytes beyond the 26 880.
 *
 * What the device does not take (the first record that is not canonical
 * and everything after it, or a tail shorter than a record) goes through a
 * host parser: blank-separated tokens, each through c2d_scan.h's grammar
 * with its pad restored, else strtod of the whole token; groups of seven.
 */
#include "c2d_evparse.hpp"

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
#include <vector>

#include "../../include/compton2d.h"
#include "c2d_evtext.hpp"
#include "c2d_scan.h"

namespace c2d {

struct EvrStat {
  unsigned long long first_bad;   /* the first record of the chunk that is not canonical (~0: none) */
  unsigned long long exact;       /* fields decided by the multi-limb path (running total)          */
};

/* the 15 bytes at img + o: the field as c2d_scan.h's two words, and the separator */
__device__ __forceinline__ void evr_field(const unsigned char* img, int o, uint64_t* w0, uint64_t* w1, uint32_t* sep) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(img + (o & ~3));
  const int sh = 8 * (o & 3);
  const uint64_t a = (uint64_t)w[0] | (uint64_t)w[1] << 32, b = (uint64_t)w[2] | (uint64_t)w[3] << 32;
  const uint64_t c = (uint64_t)w[4];
  const uint64_t lo = sh ? (a >> sh) | (b << (64 - sh)) : a;
  const uint64_t hi = sh ? (b >> sh) | (c << (64 - sh)) : b;
  *w0 = lo;
  *w1 = hi & 0xffffffffffffull;
  *sep = (uint32_t)(hi >> 48) & 0xffu;
}

__global__ void __launch_bounds__(C2D_EVT_BLOCK)
c2d_evparse_kernel(const unsigned char* __restrict__ text, int64_t nrec, const c2d_fmt_tab* __restrict__ tab,
                   double* __restrict__ out, EvrStat* st, int force_exact) {
  __shared__ __attribute__((aligned(16))) unsigned char img[C2D_EVT_BLOCK * C2D_EVT_RECORD + 16];
  __shared__ unsigned int wg_bad, wg_exact;
  const int tid = (int)threadIdx.x;
  if (tid == 0) { wg_bad = 0xffffffffu; wg_exact = 0u; }
  const int64_t r0 = (int64_t)blockIdx.x * C2D_EVT_BLOCK;
  const int64_t left = nrec - r0;
  const int cnt = left < C2D_EVT_BLOCK ? (int)left : C2D_EVT_BLOCK;
  const int nvec = (cnt * C2D_EVT_RECORD + 15) >> 4;   /* <= 1680; the buffer holds a multiple of 16 bytes */
  const uint4* src = reinterpret_cast<const uint4*>(text + r0 * C2D_EVT_RECORD);
  uint4* iv = reinterpret_cast<uint4*>(img);
  for (int v = tid; v < nvec; v += C2D_EVT_BLOCK) iv[v] = src[v];
  __syncthreads();
  const int nval = cnt * 7;
  uint64_t* dst = reinterpret_cast<uint64_t*>(out) + r0 * 7;
  unsigned int n_exact = 0u, bad = 0xffffffffu;
#pragma unroll 1
  for (int j = 0; j < 7; j++) {
    const int i = tid + C2D_EVT_BLOCK * j;
    if (i >= nval) break;
    const int rec = i / 7, f = i - 7 * rec;
    uint64_t w0, w1, bits;
    uint32_t sep;
    evr_field(img, rec * C2D_EVT_RECORD + f * 15, &w0, &w1, &sep);
    const int rc = c2d_scan_e14_7_pack_opt(tab, w0, w1, &bits, force_exact);
    if (rc < 0 || sep != (uint32_t)(f == 6 ? '\n' : ' ')) {
      bad = min(bad, (unsigned int)rec);
    } else {
      n_exact += rc == C2D_SCAN_EXACT;
      __builtin_nontemporal_store(bits, dst + i);
    }
  }
  if (bad != 0xffffffffu) atomicMin(&wg_bad, bad);
  if (n_exact) atomicAdd(&wg_exact, n_exact);
  __syncthreads();
  if (tid == 0 && wg_bad != 0xffffffffu) atomicMin(&st->first_bad, (unsigned long long)(r0 + wg_bad));
  if (tid == 1 && wg_exact) atomicAdd(&st->exact, (unsigned long long)wg_exact);
}

/* n fields of 14 bytes -> doubles and statuses (c2d_selftest_scan) */
__global__ void c2d_scan_selftest_kernel(const c2d_fmt_tab* __restrict__ tab, const unsigned char* text, int64_t n,
                                         uint64_t* out, int32_t* status, int force_exact) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned char* s = text + 14 * i;
  uint64_t w0 = 0, w1 = 0, bits = 0;
#pragma unroll
  for (int b = 0; b < 8; b++) w0 |= (uint64_t)s[b] << (8 * b);
#pragma unroll
  for (int b = 0; b < 6; b++) w1 |= (uint64_t)s[8 + b] << (8 * b);
  const int rc = c2d_scan_e14_7_pack_opt(tab, w0, w1, &bits, force_exact);
  status[i] = rc;
  if (rc >= 0) out[i] = bits;
}

/* the powers-of-ten table, built once per process */
static const c2d_fmt_tab* scan_tab() {
  static c2d_fmt_tab tab;
  static std::once_flag once;
  std::call_once(once, [] { c2d_fmt_tab_build(&tab); });
  return &tab;
}

}  // namespace c2d

using namespace c2d;

struct c2d_evt_reader {
  int device = 0;
  c2d_fmt_tab* tab_d = nullptr;
  EvrStat* stat_d = nullptr;
  EvrStat* stat_h = nullptr;          /* pinned: [3], the last one the initial value */
  unsigned char* text_d = nullptr;    /* cap records of text, rounded up to 16 bytes */
  unsigned char* pin[2] = {nullptr, nullptr};
  double* ev_d = nullptr;             /* cap events */
  int64_t cap = 0;
  hipEvent_t done[2] = {nullptr, nullptr}, ka[2] = {nullptr, nullptr}, kb[2] = {nullptr, nullptr};
};

namespace {

int efail(char* err, size_t n, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (err && n) vsnprintf(err, n, fmt, ap);
  va_end(ap);
  return code;
}

#define EVCHK(x)                                                                              \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess)                                                                     \
      return efail(err, errlen, C2D_E_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
  } while (0)

/* events per chunk: C2D_EVTEXT_CHUNK, the writer's knob, read at every call */
int64_t chunk_events() {
  const char* e = getenv("C2D_EVTEXT_CHUNK");
  if (e && *e) {
    const long long v = atoll(e);
    if (v >= 1) return (int64_t)std::min<long long>(v, 1ll << 24);
  }
  return (int64_t)1 << 20;
}

size_t text_bytes(int64_t events) { return (((size_t)events * C2D_EVT_RECORD + 15) & ~(size_t)15) + 16; }

int ensure(c2d_evt_reader* r, int64_t events, char* err, size_t errlen) {
  if (!r->tab_d) {
    EVCHK(hipMalloc((void**)&r->tab_d, sizeof(c2d_fmt_tab)));
    EVCHK(hipMemcpy(r->tab_d, scan_tab(), sizeof(c2d_fmt_tab), hipMemcpyHostToDevice));
    EVCHK(hipMalloc((void**)&r->stat_d, sizeof(EvrStat)));
    EVCHK(hipHostMalloc((void**)&r->stat_h, 3 * sizeof(EvrStat), hipHostMallocDefault));
    for (int b = 0; b < 2; b++) {
      EVCHK(hipEventCreateWithFlags(&r->done[b], hipEventDisableTiming));
      EVCHK(hipEventCreate(&r->ka[b]));
      EVCHK(hipEventCreate(&r->kb[b]));
    }
  }
  if (events > r->cap) {
    if (r->text_d) (void)hipFree(r->text_d);
    if (r->ev_d) (void)hipFree(r->ev_d);
    for (int b = 0; b < 2; b++)
      if (r->pin[b]) (void)hipHostFree(r->pin[b]);
    r->text_d = r->pin[0] = r->pin[1] = nullptr;
    r->ev_d = nullptr;
    r->cap = 0;
    EVCHK(hipMalloc((void**)&r->text_d, text_bytes(events)));
    EVCHK(hipMemset(r->text_d, ' ', text_bytes(events)));   /* the pad is never parsed; keep it defined */
    EVCHK(hipMalloc((void**)&r->ev_d, (size_t)events * 7 * sizeof(double)));
    for (int b = 0; b < 2; b++) EVCHK(hipHostMalloc((void**)&r->pin[b], (size_t)events * C2D_EVT_RECORD, hipHostMallocDefault));
    r->cap = events;
  }
  return C2D_OK;
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* up to `want` bytes, short only at the end of the file; -1 on error */
int64_t read_full(int fd, unsigned char* buf, int64_t want) {
  int64_t got = 0;
  while (got < want) {
    const ssize_t k = read(fd, buf + got, (size_t)std::min<int64_t>(want - got, (int64_t)1 << 30));
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

/* one blank-separated token: the canonical field with its pad restored, else strtod of all of it */
bool token_value(const char* t, int len, double* v) {
  char f[14];
  if (len == 14 && t[0] == '-') {
    memcpy(f, t, 14);
    if (c2d_scan_e14_7(scan_tab(), f, v) >= 0) return true;
  } else if (len == 13) {
    f[0] = ' ';
    memcpy(f + 1, t, 13);
    if (c2d_scan_e14_7(scan_tab(), f, v) >= 0) return true;
  }
  char* end = nullptr;
  *v = strtod(t, &end);
  return len > 0 && end == t + len;
}

struct HostParse {
  std::vector<double> ev;
  int64_t cap;                 /* events per delivery */
  c2d_evr_sink sink;
  void* user;
  int64_t* delivered;
  c2d_evr_times* T;
  /* the complete records gathered so far to the sink; an incomplete one stays */
  int flush() {
    const int64_t n = (int64_t)(ev.size() / 7);
    if (n == 0) return C2D_OK;
    const int rc = sink ? sink(user, ev.data(), n, 0) : C2D_OK;
    if (rc) return rc;
    *delivered += n;
    T->host_parsed += n;
    ev.erase(ev.begin(), ev.begin() + 7 * n);
    return C2D_OK;
  }
};

/* the host parser from byte `off` to the end of the file */
int host_parse(int fd, int64_t off, int64_t chunk, c2d_evr_sink sink, void* user, int64_t* delivered,
               c2d_evr_times* T, const char* path, char* err, size_t errlen) {
  const double t0 = now_ms();
  if (lseek(fd, (off_t)off, SEEK_SET) < 0)
    return efail(err, errlen, C2D_E_IO, "events: cannot seek in '%s': %s", path, strerror(errno));
  HostParse H{{}, chunk, sink, user, delivered, T};
  std::vector<unsigned char> buf((size_t)1 << 20);
  char tok[64];
  int tl = 0;
  bool too_long = false;
  int64_t pos = off, tok_off = off;
  int rc = C2D_OK;
  for (bool eof = false; !eof && !rc;) {
    const int64_t got = read_full(fd, buf.data(), (int64_t)buf.size());
    if (got < 0) {
      rc = efail(err, errlen, C2D_E_IO, "events: cannot read '%s': %s", path, strerror(errno));
      break;
    }
    eof = got < (int64_t)buf.size();
    for (int64_t i = 0; i <= got && !rc; i++) {
      const bool end_of_text = i == got;
      if (end_of_text && !eof) break;
      const unsigned char c = end_of_text ? ' ' : buf[(size_t)i];
      if (!is_blank(c)) {
        if (tl == 0) tok_off = pos + i;
        if (tl < (int)sizeof tok - 1) tok[tl++] = (char)c; else too_long = true;
        continue;
      }
      if (tl == 0) continue;
      tok[tl] = 0;
      double v = 0.0;
      if (too_long || !token_value(tok, tl, &v)) {
        rc = H.flush();   /* the records before it are delivered */
        if (!rc)
          rc = efail(err, errlen, C2D_E_IO, "events: '%s': token '%s%s' at byte offset %lld is not a number; "
                     "%lld record(s) before it were delivered", path, tok, too_long ? "..." : "", (long long)tok_off,
                     (long long)*delivered);
        break;
      }
      tl = 0;
      H.ev.push_back(v);
      if ((int64_t)H.ev.size() >= 7 * H.cap) rc = H.flush();
    }
    pos += got;
  }
  if (!rc) rc = H.flush();   /* a trailing group of fewer than seven values is dropped */
  T->host_parse_ms += now_ms() - t0;
  return rc;
}

/* chunk of `n` records in pin[b] -> device text -> events in ev_d */
int enqueue(c2d_evt_reader* r, hipStream_t stream, int b, int64_t n, int force_exact, char* err, size_t errlen) {
  EVCHK(hipMemcpyAsync(r->text_d, r->pin[b], (size_t)n * C2D_EVT_RECORD, hipMemcpyHostToDevice, stream));
  EVCHK(hipEventRecord(r->ka[b], stream));
  hipLaunchKernelGGL(c2d_evparse_kernel, dim3((unsigned)((n + C2D_EVT_BLOCK - 1) / C2D_EVT_BLOCK)), dim3(C2D_EVT_BLOCK),
                     0, stream, r->text_d, n, r->tab_d, r->ev_d, r->stat_d, force_exact);
  EVCHK(hipGetLastError());
  EVCHK(hipEventRecord(r->kb[b], stream));
  EVCHK(hipMemcpyAsync(&r->stat_h[b], r->stat_d, sizeof(EvrStat), hipMemcpyDeviceToHost, stream));
  EVCHK(hipEventRecord(r->done[b], stream));
  return C2D_OK;
}

int read_chunks(c2d_evt_reader* r, hipStream_t stream, int fd, const char* path, int64_t chunk, c2d_evr_sink sink,
                void* user, int64_t* delivered, c2d_evr_times* T, char* err, size_t errlen) {
  const int64_t chunk_bytes = chunk * C2D_EVT_RECORD;
  r->stat_h[2].first_bad = ~0ull;
  r->stat_h[2].exact = 0ull;
  EVCHK(hipMemcpyAsync(r->stat_d, &r->stat_h[2], sizeof(EvrStat), hipMemcpyHostToDevice, stream));
  bool eof = false;
  int64_t prev_n = 0, prev_base = 0;   /* the chunk in flight: its records and its byte offset */
  int prev_b = 0;
  int64_t host_off = -1;               /* where the host parser takes over */
  for (int64_t k = 0;; k++) {
    const int b = (int)(k & 1);
    int64_t cur_n = 0;
    if (!eof) {   /* chunk k into pinned buffer b while chunk k - 1 is copied and parsed */
      const double t0 = now_ms();
      const int64_t got = read_full(fd, r->pin[b], chunk_bytes);
      T->io_ms += now_ms() - t0;
      if (got < 0) return efail(err, errlen, C2D_E_IO, "events: cannot read '%s': %s", path, strerror(errno));
      cur_n = got / C2D_EVT_RECORD;
      eof = got < chunk_bytes;
      if (got % C2D_EVT_RECORD) host_off = k * chunk_bytes + cur_n * C2D_EVT_RECORD;   /* a tail shorter than a record */
    }
    if (prev_n > 0) {   /* chunk k - 1 to the sink */
      const double t0 = now_ms();
      EVCHK(hipEventSynchronize(r->done[prev_b]));
      T->wait_ms += now_ms() - t0;
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, r->ka[prev_b], r->kb[prev_b]);
      T->kernel_ms += ms;
      T->chunks++;
      T->exact_fields = (int64_t)r->stat_h[prev_b].exact;
      const unsigned long long fb = r->stat_h[prev_b].first_bad;
      const int64_t good = fb < (unsigned long long)prev_n ? (int64_t)fb : prev_n;
      if (good > 0 && sink) {
        const int rc = sink(user, r->ev_d, good, 1);
        if (rc) return rc;
      }
      *delivered += good;
      T->canonical += good;
      if (good < prev_n) {   /* not canonical from here on: the host parser's */
        host_off = prev_base + good * C2D_EVT_RECORD;
        break;
      }
      prev_n = 0;
    }
    if (cur_n > 0) {
      const char* e = getenv("C2D_SCAN_SELFTEST_EXACT");
      const int rc = enqueue(r, stream, b, cur_n, e && e[0] == '1', err, errlen);
      if (rc) return rc;
      prev_n = cur_n;
      prev_b = b;
      prev_base = k * chunk_bytes;
    }
    if (eof && prev_n == 0) break;
  }
  if (host_off >= 0) return host_parse(fd, host_off, chunk, sink, user, delivered, T, path, err, errlen);
  return C2D_OK;
}

}  // namespace

extern "C" int c2d_evparse_file(c2d_evt_reader** pr, int device, hipStream_t stream, const char* path,
                                c2d_evr_sink sink, void* user, int64_t* n_records, c2d_evr_times* times,
                                char* err, size_t errlen) {
  c2d_evr_times T = {};
  int64_t delivered = 0;
  if (n_records) *n_records = 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return efail(err, errlen, C2D_E_IO, "events: cannot open '%s': %s", path, strerror(errno));
  int64_t chunk = chunk_events();
  struct stat sb;
  if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode))   /* a small file needs small buffers */
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, (int64_t)sb.st_size / C2D_EVT_RECORD));
  if (!*pr) {
    *pr = new c2d_evt_reader;
    (*pr)->device = device;
  }
  int rc = ensure(*pr, chunk, err, errlen);
  if (!rc) {
    rc = read_chunks(*pr, stream, fd, path, chunk, sink, user, &delivered, &T, err, errlen);
    if (rc) (void)hipStreamSynchronize(stream);   /* nothing in flight out of the staging buffers */
  }
  (void)close(fd);
  if (n_records) *n_records = delivered;
  if (times) *times = T;
  return rc;
}

extern "C" void c2d_evparse_free(c2d_evt_reader* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->tab_d) (void)hipFree(r->tab_d);
  if (r->stat_d) (void)hipFree(r->stat_d);
  if (r->stat_h) (void)hipHostFree(r->stat_h);
  if (r->text_d) (void)hipFree(r->text_d);
  if (r->ev_d) (void)hipFree(r->ev_d);
  for (int b = 0; b < 2; b++) {
    if (r->pin[b]) (void)hipHostFree(r->pin[b]);
    if (r->done[b]) (void)hipEventDestroy(r->done[b]);
    if (r->ka[b]) (void)hipEventDestroy(r->ka[b]);
    if (r->kb[b]) (void)hipEventDestroy(r->kb[b]);
  }
  delete r;
}

extern "C" int c2d_selftest_scan(int device, const char* text_host, int64_t n, double* out_host, int32_t* status_host) {
  if (n < 0 || (n > 0 && (!text_host || !out_host || !status_host))) return C2D_E_ARG;
  if (n == 0) return C2D_OK;
  if (hipSetDevice(device) != hipSuccess) return C2D_E_HIP;
  c2d_fmt_tab* tab = nullptr;
  unsigned char* text = nullptr;
  uint64_t* out = nullptr;
  int32_t* status = nullptr;
  int rc = C2D_OK;
  if (hipMalloc((void**)&tab, sizeof(c2d_fmt_tab)) != hipSuccess || hipMalloc((void**)&text, (size_t)n * 14) != hipSuccess ||
      hipMalloc((void**)&out, (size_t)n * 8) != hipSuccess || hipMalloc((void**)&status, (size_t)n * 4) != hipSuccess)
    rc = C2D_E_HIP;
  /* a field that is not canonical leaves the caller's value as it was */
  if (!rc && (hipMemcpy(tab, scan_tab(), sizeof(c2d_fmt_tab), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(text, text_host, (size_t)n * 14, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(out, out_host, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess))
    rc = C2D_E_HIP;
  if (!rc) {
    /* C2D_SCAN_SELFTEST_EXACT=1 (read at every call): every field through the
     * multi-limb path, which event files hardly ever reach */
    const char* e = getenv("C2D_SCAN_SELFTEST_EXACT");
    hipLaunchKernelGGL(c2d_scan_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, tab, text, n, out,
                       status, e && e[0] == '1');
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = C2D_E_HIP;
  }
  if (!rc && (hipMemcpy(out_host, out, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(status_host, status, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess))
    rc = C2D_E_HIP;
  (void)hipFree(tab);
  (void)hipFree(text);
  (void)hipFree(out);
  (void)hipFree(status);
  return rc;
}
