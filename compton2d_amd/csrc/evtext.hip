/*
 * evtext.hip — escape events (AoS 7 x f64 in device memory) to the text of
 * p###_evb.dat (src/imcleak2d.f:181: 6(e14.7,1x),e14.7, 105 bytes a record),
 * formatted on the device by c2d_fmt.h and streamed to the file through two
 * pinned host buffers.
 *
 * Kernel: one workgroup per 256 events of one segment.  Loads are coalesced
 * over the value index (event = i / 7, field = i % 7); each lane formats its
 * values and places the 15 bytes (field + blank or newline) in an LDS image
 * of the workgroup's 26 880 bytes, as three dword and three byte stores
 * whatever the field's alignment.  The image starts at the offset in LDS
 * that the workgroup's first output byte has modulo 16, so image and output
 * are 16-byte aligned together: the workgroup stores the image as 16-byte
 * vectors, and the up to 15 bytes before the first and after the last
 * aligned vector byte by byte (105 is odd: segments and chunks start at any
 * byte).  The powers-of-ten table (c2d_fmt_tab, 11 KB) is read through L2.
 * The multi-limb path of the formatter is a call (noinline) with rolled
 * loops, outside the common path's registers.
 */
#include "c2d_evtext.hpp"

#include "c2d_textio.hpp"

namespace c2d {

struct EvtSegs {
  const double* ev[C2D_EVT_MAXSEG];   /* segment s: n[s] events                          */
  int64_t n[C2D_EVT_MAXSEG];
  int64_t rec0[C2D_EVT_MAXSEG];       /* record index of its first event in the output    */
  int32_t blk0[C2D_EVT_MAXSEG + 1];   /* its first workgroup (prefix sums of ceil(n/256)) */
  int32_t nseg;
};

struct EvtStat {
  unsigned long long nonfinite;   /* NaN/Inf values met                         */
  unsigned long long first_bad;   /* the smallest 7 * record + field among them */
  unsigned long long ambiguous;   /* values the fast path could not decide      */
  unsigned long long multilimb;   /* of them, decided by the multi-limb path    */
};

/* the workgroup's segment, first event in it and event count */
__device__ __forceinline__ int evt_locate(const EvtSegs& S, int64_t* e0, int* cnt) {
  int s = 0;
  while (s + 1 < S.nseg && (int)blockIdx.x >= S.blk0[s + 1]) s++;
  *e0 = (int64_t)((int)blockIdx.x - S.blk0[s]) * C2D_EVT_BLOCK;
  const int64_t left = S.n[s] - *e0;
  *cnt = left < C2D_EVT_BLOCK ? (int)left : C2D_EVT_BLOCK;
  return s;
}

__device__ __forceinline__ void evt_bad(EvtStat* st, unsigned long long value_index) {
  atomicAdd(&st->nonfinite, 1ull);
  atomicMin(&st->first_bad, value_index);
}

/* NaN/Inf among the events: counted before a byte of the file is written */
__global__ void __launch_bounds__(C2D_EVT_BLOCK) c2d_evscan_kernel(EvtSegs S, EvtStat* st) {
  int64_t e0;
  int cnt;
  const int s = evt_locate(S, &e0, &cnt);
  const uint64_t* src = reinterpret_cast<const uint64_t*>(S.ev[s]) + e0 * 7;
  const int nval = cnt * 7;
#pragma unroll
  for (int j = 0; j < 7; j++) {
    const int i = (int)threadIdx.x + C2D_EVT_BLOCK * j;
    if (i < nval && ((src[i] >> 52) & 0x7ffu) == 0x7ffu)
      evt_bad(st, (unsigned long long)(S.rec0[s] + e0) * 7ull + (unsigned long long)i);
  }
}

__global__ void __launch_bounds__(C2D_EVT_BLOCK)
c2d_evtext_kernel(EvtSegs S, const c2d_fmt_tab* __restrict__ tab, char* __restrict__ out, EvtStat* st) {
  __shared__ __attribute__((aligned(16))) unsigned char img[C2D_EVT_BLOCK * C2D_EVT_RECORD + 16];
  /* ambiguous / multi-limb values of the workgroup: one global atomic each per
   * workgroup (a quarter of the values are ambiguous where escapes sit on
   * round boundaries; one atomic per value on one address took 14 ms of a
   * 1.1e7-event launch) */
  __shared__ unsigned int wg_cnt[2];
  if (threadIdx.x < 2) wg_cnt[threadIdx.x] = 0u;
  __syncthreads();
  unsigned int n_amb = 0u, n_ml = 0u;
  int64_t e0;
  int cnt;
  const int s = evt_locate(S, &e0, &cnt);
  const double* src = S.ev[s] + e0 * 7;
  const int nval = cnt * 7;
  char* dst = out + (S.rec0[s] + e0) * C2D_EVT_RECORD;
  const int pad = (int)(reinterpret_cast<uintptr_t>(dst) & 15u);
  const int tid = (int)threadIdx.x;
  /* one value formatted per pass, the next one's load already in flight */
  double xn = tid < nval ? __builtin_nontemporal_load(src + tid) : 0.0;
#pragma unroll 1
  for (int j = 0; j < 7; j++) {
    const int i = tid + C2D_EVT_BLOCK * j;
    if (i >= nval) break;
    const double x = xn;
    if (i + C2D_EVT_BLOCK < nval) xn = __builtin_nontemporal_load(src + i + C2D_EVT_BLOCK);
    uint64_t w0 = 0x2020202020202020ull, w1 = 0x202020202020ull;   /* a non-finite value: blanks */
    const int rc = c2d_fmt_e14_7_pack(tab, x, &w0, &w1);
    n_amb += rc > 0;
    n_ml += rc == C2D_FMT_MULTILIMB;
    if (rc == C2D_FMT_NONFINITE)
      evt_bad(st, (unsigned long long)(S.rec0[s] + e0) * 7ull + (unsigned long long)i);
    const int ev = i / 7, f = i - 7 * ev;
    /* 15 bytes V[0..15) at o: h = (4 - o) mod 4 single bytes up to the next
     * dword, three dwords, 3 - h single bytes */
    const unsigned __int128 V = (unsigned __int128)w0 | (unsigned __int128)(w1 | (uint64_t)(f == 6 ? '\n' : ' ') << 48) << 64;
    const int o = pad + ev * C2D_EVT_RECORD + f * 15;
    const int h = (4 - o) & 3;
    const unsigned __int128 M = V >> (8 * h);
    uint32_t* d = reinterpret_cast<uint32_t*>(img + o + h);
    d[0] = (uint32_t)M;
    d[1] = (uint32_t)(M >> 32);
    d[2] = (uint32_t)(M >> 64);
#pragma unroll
    for (int b = 0; b < 3; b++) {
      const int idx = b < h ? b : 12 + b;
      img[o + idx] = (unsigned char)(V >> (8 * idx));
    }
  }
  if (n_amb) atomicAdd(&wg_cnt[0], n_amb);
  if (n_ml) atomicAdd(&wg_cnt[1], n_ml);
  __syncthreads();
  if (tid == 0 && wg_cnt[0]) atomicAdd(&st->ambiguous, (unsigned long long)wg_cnt[0]);
  if (tid == 1 && wg_cnt[1]) atomicAdd(&st->multilimb, (unsigned long long)wg_cnt[1]);
  const int len = cnt * C2D_EVT_RECORD;
  const int head = min(len, (16 - pad) & 15);
  const int nvec = (len - head) >> 4;
  const int tail = len - head - 16 * nvec;
  if (tid < head) dst[tid] = (char)img[pad + tid];
  const uint4* iv = reinterpret_cast<const uint4*>(img + pad + head);
  uint4* ov = reinterpret_cast<uint4*>(dst + head);
  /* pad + head is a multiple of 16 (or the text ends inside the head and nvec = 0) */
  for (int v = tid; v < nvec; v += C2D_EVT_BLOCK) ov[v] = iv[v];
  if (tid < tail) dst[head + 16 * nvec + tid] = (char)img[pad + head + 16 * nvec + tid];
}

/* n doubles -> 14 bytes each (c2d_selftest_fmt) */
__global__ void c2d_fmt_selftest_kernel(const c2d_fmt_tab* __restrict__ tab, const double* x, int64_t n, char* out,
                                        EvtStat* st, int shortcut) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t w0 = 0, w1 = 0;
  const int rc = c2d_fmt_e14_7_pack_opt(tab, x[i], &w0, &w1, shortcut);
  if (rc == C2D_FMT_NONFINITE) {
    evt_bad(st, (unsigned long long)i);
    return;
  }
  char* o = out + 14 * i;
#pragma unroll
  for (int b = 0; b < 8; b++) o[b] = (char)(w0 >> (8 * b));
#pragma unroll
  for (int b = 0; b < 6; b++) o[8 + b] = (char)(w1 >> (8 * b));
}

}  // namespace c2d

using namespace c2d;

struct c2d_evt_writer {
  TextStage<EvtStat> st;              /* the text buffer has no pad: the kernel stores the exact bytes */
  double* stage_d = nullptr;          /* host-supplied events, one chunk */
  int64_t stage_cap = 0;
};

namespace {

constexpr EvtStat EVT_STAT0 = {0ull, ~0ull, 0ull, 0ull};   /* nothing met yet */

/* the segments of records [c0, c1) of the concatenation */
void chunk_segments(const double* const* seg, const int64_t* cnt, int nseg, int64_t c0, int64_t c1, bool rec_global,
                    EvtSegs* S) {
  memset(S, 0, sizeof *S);
  int64_t base = 0;
  int k = 0;
  for (int s = 0; s < nseg; s++) {
    const int64_t a = std::max(c0, base), b = std::min(c1, base + cnt[s]);
    if (b > a) {
      S->ev[k] = seg[s] + (a - base) * 7;
      S->n[k] = b - a;
      S->rec0[k] = rec_global ? a : a - c0;
      S->blk0[k + 1] = S->blk0[k] + (int32_t)((b - a + C2D_EVT_BLOCK - 1) / C2D_EVT_BLOCK);
      k++;
    }
    base += cnt[s];
  }
  S->nseg = k;
}

int ensure(c2d_evt_writer* w, int64_t events, int64_t stage_events, char* err, size_t errlen) {
  { const int rc = w->st.ensure(events, C2D_EVT_RECORD, false, [](int64_t) { return C2D_OK; }, err, errlen);
    if (rc) return rc; }
  if (stage_events > w->stage_cap) {
    if (w->stage_d) (void)hipFree(w->stage_d);
    w->stage_d = nullptr;
    w->stage_cap = 0;
    C2D_TXCHK(hipMalloc((void**)&w->stage_d, (size_t)stage_events * 7 * sizeof(double)));
    w->stage_cap = stage_events;
  }
  return C2D_OK;
}

int nonfinite_error(unsigned long long count, unsigned long long first, char* err, size_t errlen) {
  return efail(err, errlen, C2D_E_NONFINITE,
               "events: %llu non-finite value(s); the first in record %llu (counted from 1), field %llu; "
               "the file was not touched", count, first / 7ull + 1ull, first % 7ull + 1ull);
}

/* the chunks of [0, n) through the two pinned buffers into f */
int write_events(c2d_evt_writer* w, hipStream_t stream, const double* const* seg, const int64_t* cnt, int nseg,
                 int on_device, int64_t n, int64_t chunk, FILE* f, const char* path, c2d_evt_times* T, char* err,
                 size_t errlen) {
  TextStage<EvtStat>& st = w->st;
  auto produce = [&](int b, int64_t c0, int64_t m) {
    EvtSegs S;
    if (on_device) {
      chunk_segments(seg, cnt, nseg, c0, c0 + m, false, &S);
    } else {
      C2D_TXCHK(hipMemcpyAsync(w->stage_d, seg[0] + c0 * 7, (size_t)m * 7 * sizeof(double), hipMemcpyHostToDevice,
                               stream));
      const double* sd = w->stage_d;
      chunk_segments(&sd, &m, 1, 0, m, false, &S);
    }
    return st.timed(stream, b, [&] {
      hipLaunchKernelGGL(c2d_evtext_kernel, dim3((unsigned)S.blk0[S.nseg]), dim3(C2D_EVT_BLOCK), 0, stream, S,
                         st.tab_d, (char*)st.text_d, st.stat_d);
    }, err, errlen);
  };
  auto counts = [&](int b) {
    T->ambiguous = (int64_t)st.stat_h[b].ambiguous;
    T->multilimb = (int64_t)st.stat_h[b].multilimb;
  };
  auto nothing = [](int, int64_t) { return C2D_OK; };
  return write_chunks(st, stream, f, "events", path, C2D_EVT_RECORD, n, chunk, EVT_STAT0, T, produce, nothing, counts,
                      nothing, err, errlen);
}

}  // namespace

extern "C" int c2d_evtext_write(c2d_evt_writer** pw, int device, hipStream_t stream, const double* const* seg,
                                const int64_t* cnt, int nseg, int on_device, const char* path, int append,
                                int64_t* n_written, c2d_evt_times* times, char* err, size_t errlen) {
  c2d_evt_times T = {};
  int64_t n = 0;
  for (int s = 0; s < nseg; s++) n += cnt[s];
  if (nseg < 1 || nseg > C2D_EVT_MAXSEG || (!on_device && nseg != 1))
    return efail(err, errlen, C2D_E_ARG, "events: bad segment list");
  if (n > 0) {
    if (!*pw) {
      *pw = new c2d_evt_writer;
      (*pw)->st.device = device;
    }
    c2d_evt_writer* w = *pw;
    TextStage<EvtStat>& st = w->st;
    const int64_t chunk = chunk_env("C2D_EVTEXT_CHUNK", 0);
    const int64_t m = std::min(chunk, n);
    { const int rc = ensure(w, m, on_device ? 0 : m, err, errlen); if (rc) return rc; }
    /* non-finite values first: the file is opened only once there is none */
    if (on_device) {
      EvtStat init = EVT_STAT0;
      EvtSegs S;
      int64_t done = 0;
      C2D_TXCHK(hipMemcpyAsync(st.stat_d, &init, sizeof init, hipMemcpyHostToDevice, stream));
      C2D_TXCHK(hipEventRecord(st.ka[0], stream));
      while (done < n) {   /* launches of at most 2^30 events (the workgroup index is an int32) */
        const int64_t c1 = std::min(n, done + ((int64_t)1 << 30));
        chunk_segments(seg, cnt, nseg, done, c1, true, &S);
        hipLaunchKernelGGL(c2d_evscan_kernel, dim3((unsigned)S.blk0[S.nseg]), dim3(C2D_EVT_BLOCK), 0, stream, S,
                           st.stat_d);
        C2D_TXCHK(hipGetLastError());
        done = c1;
      }
      C2D_TXCHK(hipEventRecord(st.kb[0], stream));
      C2D_TXCHK(hipMemcpyAsync(&st.stat_h[0], st.stat_d, sizeof(EvtStat), hipMemcpyDeviceToHost, stream));
      C2D_TXCHK(hipStreamSynchronize(stream));
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, st.ka[0], st.kb[0]);
      T.scan_ms = ms;
      if (st.stat_h[0].nonfinite) return nonfinite_error(st.stat_h[0].nonfinite, st.stat_h[0].first_bad, err, errlen);
    } else {
      const double t0 = now_ms();
      const uint64_t* u = reinterpret_cast<const uint64_t*>(seg[0]);
      unsigned long long bad = 0, first = 0;
      for (int64_t i = 0; i < 7 * n; i++)
        if (((u[i] >> 52) & 0x7ffu) == 0x7ffu && bad++ == 0) first = (unsigned long long)i;
      T.scan_ms = now_ms() - t0;
      if (bad) return nonfinite_error(bad, first, err, errlen);
    }
    FILE* f = fopen(path, append ? "ab" : "wb");
    if (!f) return efail(err, errlen, C2D_E_IO, "events: cannot open '%s': %s", path, strerror(errno));
    setvbuf(f, nullptr, _IONBF, 0);   /* the chunks are the buffer */
    int rc = write_events(w, stream, seg, cnt, nseg, on_device, n, chunk, f, path, &T, err, errlen);
    if (rc) (void)hipStreamSynchronize(stream);   /* nothing in flight into the staging buffers */
    if (fclose(f) != 0 && !rc) rc = efail(err, errlen, C2D_E_IO, "events: cannot close '%s': %s", path, strerror(errno));
    if (rc) return rc;
  } else if (!append) {
    FILE* f = fopen(path, "wb");
    if (!f) return efail(err, errlen, C2D_E_IO, "events: cannot open '%s': %s", path, strerror(errno));
    if (fclose(f) != 0) return efail(err, errlen, C2D_E_IO, "events: cannot close '%s': %s", path, strerror(errno));
  }
  if (n_written) *n_written = n;
  if (times) *times = T;
  return C2D_OK;
}

extern "C" void c2d_evtext_free(c2d_evt_writer* w) {
  if (!w) return;
  (void)hipSetDevice(w->st.device);
  w->st.release();
  if (w->stage_d) (void)hipFree(w->stage_d);
  delete w;
}

extern "C" int c2d_selftest_fmt(int device, const double* x_host, int64_t n, char* out_host) {
  if (n < 0 || (n > 0 && (!x_host || !out_host))) return C2D_E_ARG;
  if (n == 0) return C2D_OK;
  if (hipSetDevice(device) != hipSuccess) return C2D_E_HIP;
  c2d_fmt_tab* tab = nullptr;
  double* x = nullptr;
  char* out = nullptr;
  EvtStat* st = nullptr;
  EvtStat h = {0ull, ~0ull, 0ull, 0ull};
  int rc = C2D_OK;
  if (hipMalloc((void**)&tab, sizeof(c2d_fmt_tab)) != hipSuccess || hipMalloc((void**)&x, n * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&out, (size_t)n * 14) != hipSuccess || hipMalloc((void**)&st, sizeof(EvtStat)) != hipSuccess)
    rc = C2D_E_HIP;
  if (!rc && (hipMemcpy(tab, fmt_tab(), sizeof(c2d_fmt_tab), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(x, x_host, n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(st, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemset(out, '#', (size_t)n * 14) != hipSuccess))
    rc = C2D_E_HIP;
  if (!rc) {
    /* C2D_FMT_SELFTEST_MULTILIMB=1 (read at every call): every ambiguous
     * value through the multi-limb path, which the events hardly ever reach */
    const char* e = getenv("C2D_FMT_SELFTEST_MULTILIMB");
    const int shortcut = !(e && e[0] == '1');
    hipLaunchKernelGGL(c2d_fmt_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, tab, x, n, out, st,
                       shortcut);
    if (hipDeviceSynchronize() != hipSuccess) rc = C2D_E_HIP;
  }
  if (!rc && (hipMemcpy(out_host, out, (size_t)n * 14, hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemcpy(&h, st, sizeof h, hipMemcpyDeviceToHost) != hipSuccess))
    rc = C2D_E_HIP;
  if (!rc && h.nonfinite) rc = C2D_E_NONFINITE;
  (void)hipFree(tab);
  (void)hipFree(x);
  (void)hipFree(out);
  (void)hipFree(st);
  return rc;
}
