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
 * and everything after it, or a tail shorter than a record) goes through the
 * host parser of c2d_textparse.hpp: blank-separated tokens, each through c2d_scan.h's grammar
 * with its pad restored, else strtod of the whole token; groups of seven.
 */
#include "c2d_evparse.hpp"

#include <fcntl.h>
#include <sys/stat.h>

#include "c2d_evtext.hpp"
#include "c2d_textio.hpp"

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

}  // namespace c2d

using namespace c2d;

struct c2d_evt_reader {
  TextStage<EvrStat> st;     /* the text padded: the kernel stages whole 16-byte vectors */
  double* ev_d = nullptr;    /* cap events */
};

extern "C" int c2d_evparse_file(c2d_evt_reader** pr, int device, hipStream_t stream, const char* path,
                                c2d_evr_sink sink, void* user, int64_t* n_records, c2d_evr_times* times,
                                char* err, size_t errlen) {
  c2d_evr_times T = {};
  int64_t delivered = 0;
  if (n_records) *n_records = 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return efail(err, errlen, C2D_E_IO, "events: cannot open '%s': %s", path, strerror(errno));
  int64_t chunk = chunk_env("C2D_EVTEXT_CHUNK", 1ll << 24);   /* the writer's knob */
  struct stat sb;
  if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode))   /* a small file needs small buffers */
    chunk = std::min<int64_t>(chunk, std::max<int64_t>(1, (int64_t)sb.st_size / C2D_EVT_RECORD));
  if (!*pr) {
    *pr = new c2d_evt_reader;
    (*pr)->st.device = device;
  }
  c2d_evt_reader* r = *pr;
  TextStage<EvrStat>& st = r->st;
  int rc = st.ensure(chunk, C2D_EVT_RECORD, true, [&](int64_t events) {
    if (r->ev_d) (void)hipFree(r->ev_d);
    r->ev_d = nullptr;
    C2D_TXCHK(hipMalloc((void**)&r->ev_d, (size_t)events * 7 * sizeof(double)));
    return C2D_OK;
  }, err, errlen);
  if (!rc) {
    const char* e = getenv("C2D_SCAN_SELFTEST_EXACT");
    const int force_exact = e && e[0] == '1';
    /* chunk of n records: device text -> events in ev_d */
    auto enqueue = [&](int b, int64_t n, int64_t) {
      return st.timed(stream, b, [&] {
        hipLaunchKernelGGL(c2d_evparse_kernel, dim3((unsigned)((n + C2D_EVT_BLOCK - 1) / C2D_EVT_BLOCK)),
                           dim3(C2D_EVT_BLOCK), 0, stream, st.text_d, n, st.tab_d, r->ev_d, st.stat_d, force_exact);
      }, err, errlen);
    };
    auto deliver = [&](int b, int64_t good) {
      T.exact_fields = (int64_t)st.stat_h[b].exact;
      if (good > 0 && sink) {
        const int rc = sink(user, r->ev_d, good, 1);
        if (rc) return rc;
      }
      delivered += good;
      T.canonical += good;
      return C2D_OK;
    };
    auto host = [&](int64_t off) {
      return evr_host_parse(fd, off, chunk, sink, user, &delivered, &T, path, err, errlen);
    };
    rc = read_chunks(st, stream, fd, "events", path, C2D_EVT_RECORD, chunk, EvrStat{~0ull, 0ull}, &T,
                     [](int, int64_t) { return C2D_OK; }, enqueue, deliver, host, err, errlen);
    if (rc) (void)hipStreamSynchronize(stream);   /* nothing in flight out of the staging buffers */
  }
  (void)close(fd);
  if (n_records) *n_records = delivered;
  if (times) *times = T;
  return rc;
}

extern "C" void c2d_evparse_free(c2d_evt_reader* r) {
  if (!r) return;
  (void)hipSetDevice(r->st.device);
  r->st.release();
  if (r->ev_d) (void)hipFree(r->ev_d);
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
  if (!rc && (hipMemcpy(tab, fmt_tab(), sizeof(c2d_fmt_tab), hipMemcpyHostToDevice) != hipSuccess ||
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
