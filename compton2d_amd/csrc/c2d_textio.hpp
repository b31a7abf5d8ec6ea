/*
 * c2d_textio.hpp — the streaming layer of the event and census text files
 * (evtext.hip, evparse.hip, censtext.hip): the staging buffers of a route and
 * the two double-buffered loops.  A file moves in chunks of records through
 * two pinned host buffers: while chunk k is copied and formatted or parsed on
 * the stream, the host writes chunk k - 1 to the file or reads chunk k + 1
 * from it.  The formats supply their steps as callables.
 */
#ifndef C2D_TEXTIO_HPP
#define C2D_TEXTIO_HPP

#include <hip/hip_runtime.h>

#include "c2d_textparse.hpp"

#define C2D_TXCHK(x)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess)                                                                     \
      return c2d::efail(err, errlen, C2D_E_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
  } while (0)

namespace c2d {

/* `records` of text on the device; padded: rounded up to 16 bytes and 16 beyond */
inline size_t text_bytes(int64_t records, int record, bool pad) {
  const size_t n = (size_t)records * (size_t)record;
  return pad ? ((n + 15) & ~(size_t)15) + 16 : n;
}

/* What every route stages through; Stat is the route's status struct (the
 * kernels' word on the device, pinned copies on the host). */
template <class Stat>
struct TextStage {
  int device = 0;
  c2d_fmt_tab* tab_d = nullptr;
  Stat* stat_d = nullptr;
  Stat* stat_h = nullptr;                       /* pinned: [3], one per buffer and the initial value */
  unsigned char* text_d = nullptr;              /* cap records of text */
  unsigned char* pin[2] = {nullptr, nullptr};   /* pinned host staging, cap records each */
  int64_t cap = 0;
  hipEvent_t done[2] = {nullptr, nullptr}, ka[2] = {nullptr, nullptr}, kb[2] = {nullptr, nullptr};

  /* Room for `records` of `record` bytes.  own(records) frees and allocates
   * what the route keeps per record beside the text. */
  template <class Own>
  int ensure(int64_t records, int record, bool pad, Own&& own, char* err, size_t errlen) {
    if (!tab_d) {
      C2D_TXCHK(hipMalloc((void**)&tab_d, sizeof(c2d_fmt_tab)));
      C2D_TXCHK(hipMemcpy(tab_d, fmt_tab(), sizeof(c2d_fmt_tab), hipMemcpyHostToDevice));
      C2D_TXCHK(hipMalloc((void**)&stat_d, sizeof(Stat)));
      C2D_TXCHK(hipHostMalloc((void**)&stat_h, 3 * sizeof(Stat), hipHostMallocDefault));
      for (int b = 0; b < 2; b++) {
        C2D_TXCHK(hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
        C2D_TXCHK(hipEventCreate(&ka[b]));
        C2D_TXCHK(hipEventCreate(&kb[b]));
      }
    }
    if (records <= cap) return C2D_OK;
    if (text_d) (void)hipFree(text_d);
    for (int b = 0; b < 2; b++)
      if (pin[b]) (void)hipHostFree(pin[b]);
    text_d = pin[0] = pin[1] = nullptr;
    cap = 0;
    C2D_TXCHK(hipMalloc((void**)&text_d, text_bytes(records, record, pad)));
    if (pad)   /* the pad is never parsed; keep it defined */
      C2D_TXCHK(hipMemset(text_d, ' ', text_bytes(records, record, pad)));
    { const int rc = own(records); if (rc) return rc; }
    for (int b = 0; b < 2; b++)
      C2D_TXCHK(hipHostMalloc((void**)&pin[b], (size_t)records * (size_t)record, hipHostMallocDefault));
    cap = records;
    return C2D_OK;
  }

  void release() {
    if (tab_d) (void)hipFree(tab_d);
    if (stat_d) (void)hipFree(stat_d);
    if (stat_h) (void)hipHostFree(stat_h);
    if (text_d) (void)hipFree(text_d);
    for (int b = 0; b < 2; b++) {
      if (pin[b]) (void)hipHostFree(pin[b]);
      if (done[b]) (void)hipEventDestroy(done[b]);
      if (ka[b]) (void)hipEventDestroy(ka[b]);
      if (kb[b]) (void)hipEventDestroy(kb[b]);
    }
  }

  /* the status word on the device to `init`, through the third pinned slot */
  int reset(hipStream_t stream, const Stat& init, char* err, size_t errlen) {
    stat_h[2] = init;
    C2D_TXCHK(hipMemcpyAsync(stat_d, &stat_h[2], sizeof(Stat), hipMemcpyHostToDevice, stream));
    return C2D_OK;
  }

  /* launch() between the events ka[b] and kb[b]: the kernel time of buffer b's chunk */
  template <class Launch>
  int timed(hipStream_t stream, int b, Launch&& launch, char* err, size_t errlen) {
    C2D_TXCHK(hipEventRecord(ka[b], stream));
    launch();
    C2D_TXCHK(hipGetLastError());
    C2D_TXCHK(hipEventRecord(kb[b], stream));
    return C2D_OK;
  }

  /* the status of buffer b's chunk to its pinned slot, and the chunk's end */
  int finish(hipStream_t stream, int b, char* err, size_t errlen) {
    C2D_TXCHK(hipMemcpyAsync(&stat_h[b], stat_d, sizeof(Stat), hipMemcpyDeviceToHost, stream));
    C2D_TXCHK(hipEventRecord(done[b], stream));
    return C2D_OK;
  }
};

/*
 * The file `fd` of `record`-byte records to the device, a chunk at a time:
 * chunk k is read into pinned buffer k & 1 while chunk k - 1 is copied and
 * parsed; then chunk k - 1 is retired.  `what` names the format in the
 * messages ("events", "census").  A chunk is `head` bytes (the checkpoint's
 * chunk head; 0 in the text files) and then whole records; offsets count
 * from where fd stands at the call.
 *   want(k)           bytes of chunk k, head included; 0: no further chunk
 *   side(b, n)        reads what lies beside the n records of buffer b (inside io_ms)
 *   enqueue(b, n, k)  queues the parse of chunk k, n records, whose text is on the device
 *   deliver(b, good)  hands over the canonical prefix of buffer b's chunk
 *   host(off)         parses from byte `off` to the end of the file on the host
 * The kernels lower Stat::first_bad to the first record that is not canonical.
 */
template <class Stat, class Times, class Want, class Side, class Enqueue, class Deliver, class Host>
int read_chunks_sized(TextStage<Stat>& r, hipStream_t stream, int fd, const char* what, const char* path, int record,
                      int head, Want&& want, const Stat& init, Times* T, Side&& side, Enqueue&& enqueue,
                      Deliver&& deliver, Host&& host, char* err, size_t errlen) {
  { const int rc = r.reset(stream, init, err, errlen); if (rc) return rc; }
  bool eof = false;
  int64_t prev_n = 0, prev_base = 0;   /* the chunk in flight: its records and its byte offset */
  int64_t file_off = 0;                /* bytes taken from fd so far */
  int prev_b = 0;
  int64_t host_off = -1;               /* where the host parser takes over */
  for (int64_t k = 0;; k++) {
    const int b = (int)(k & 1);
    int64_t cur_n = 0;
    const int64_t cur_base = file_off;
    const int64_t need = eof ? 0 : want(k);
    if (need == 0) eof = true;
    if (!eof) {   /* chunk k into pinned buffer b while chunk k - 1 is copied and parsed */
      const double t0 = now_ms();
      const int64_t got = read_full(fd, r.pin[b], need);
      if (got < 0) {
        T->io_ms += now_ms() - t0;
        return efail(err, errlen, C2D_E_IO, "%s: cannot read '%s': %s", what, path, strerror(errno));
      }
      cur_n = got > head ? (got - head) / record : 0;
      eof = got < need;
      file_off += got;
      if (got != (cur_n ? head + cur_n * record : 0))   /* a tail shorter than a record */
        host_off = cur_base + (cur_n ? head + cur_n * record : 0);
      if (cur_n > 0) { const int rc = side(b, cur_n); if (rc) return rc; }
      T->io_ms += now_ms() - t0;
    }
    if (prev_n > 0) {   /* chunk k - 1 to the sink */
      const double t0 = now_ms();
      C2D_TXCHK(hipEventSynchronize(r.done[prev_b]));
      T->wait_ms += now_ms() - t0;
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, r.ka[prev_b], r.kb[prev_b]);
      T->kernel_ms += ms;
      T->chunks++;
      const unsigned long long fb = r.stat_h[prev_b].first_bad;
      const int64_t good = fb < (unsigned long long)prev_n ? (int64_t)fb : prev_n;
      { const int rc = deliver(prev_b, good); if (rc) return rc; }
      if (good < prev_n) {   /* not canonical from here on: the host parser's */
        host_off = prev_base + head + good * record;
        break;
      }
      prev_n = 0;
    }
    if (cur_n > 0) {
      C2D_TXCHK(hipMemcpyAsync(r.text_d, r.pin[b], (size_t)(head + cur_n * record), hipMemcpyHostToDevice, stream));
      { const int rc = enqueue(b, cur_n, k); if (rc) return rc; }
      { const int rc = r.finish(stream, b, err, errlen); if (rc) return rc; }
      prev_n = cur_n;
      prev_b = b;
      prev_base = cur_base;
    }
    if (eof && prev_n == 0) break;
  }
  return host_off >= 0 ? host(host_off) : C2D_OK;
}

/* a text file: every chunk is `chunk` records with nothing before them, to the end of the file */
template <class Stat, class Times, class Side, class Enqueue, class Deliver, class Host>
int read_chunks(TextStage<Stat>& r, hipStream_t stream, int fd, const char* what, const char* path, int record,
                int64_t chunk, const Stat& init, Times* T, Side&& side, Enqueue&& enqueue, Deliver&& deliver,
                Host&& host, char* err, size_t errlen) {
  const int64_t chunk_bytes = chunk * record;
  return read_chunks_sized(r, stream, fd, what, path, record, 0, [&](int64_t) { return chunk_bytes; }, init, T, side,
                           enqueue, deliver, host, err, errlen);
}

/*
 * n records of `record` bytes to the file f, `chunk` at a time: chunk k is
 * formatted and copied to pinned buffer k & 1 while chunk k - 1 goes to the
 * file.  `head` bytes before a chunk's records travel with them (the
 * checkpoint's chunk head, filled on the device; 0 in the text files).
 *   produce(b, c0, m)   queues the format of records [c0, c0 + m) into the device text
 *   copy_out(b, m)      queues the copies beside the text's
 *   counts(b)           takes the route's counters of buffer b's chunk
 *   write_side(b, m)    writes what goes beside the text (inside io_ms)
 * The format kernels count Stat::nonfinite; the caller's scan found none, so
 * one here means the records changed under the call.
 */
template <class Stat, class Times, class Produce, class CopyOut, class Counts, class WriteSide>
int write_chunks_headed(TextStage<Stat>& w, hipStream_t stream, FILE* f, const char* what, const char* path,
                        int record, int head, int64_t n, int64_t chunk, const Stat& init, Times* T, Produce&& produce,
                        CopyOut&& copy_out, Counts&& counts, WriteSide&& write_side, char* err, size_t errlen) {
  const int64_t nchunks = (n + chunk - 1) / chunk;
  { const int rc = w.reset(stream, init, err, errlen); if (rc) return rc; }
  for (int64_t k = 0; k <= nchunks; k++) {
    if (k < nchunks) {   /* chunk k: format, copy to the pinned buffers k % 2 */
      const int b = (int)(k & 1);
      const int64_t c0 = k * chunk, m = std::min(n, c0 + chunk) - c0;
      { const int rc = produce(b, c0, m); if (rc) return rc; }
      C2D_TXCHK(hipMemcpyAsync(w.pin[b], w.text_d, (size_t)(head + m * record), hipMemcpyDeviceToHost, stream));
      { const int rc = copy_out(b, m); if (rc) return rc; }
      { const int rc = w.finish(stream, b, err, errlen); if (rc) return rc; }
    }
    if (k > 0) {   /* chunk k - 1: to the file while chunk k is formatted and copied */
      const int b = (int)((k - 1) & 1);
      const int64_t c0 = (k - 1) * chunk, m = std::min(n, c0 + chunk) - c0;
      const double t0 = now_ms();
      C2D_TXCHK(hipEventSynchronize(w.done[b]));
      const double t1 = now_ms();
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, w.ka[b], w.kb[b]);
      T->kernel_ms += ms;
      T->wait_ms += t1 - t0;
      T->chunks++;
      counts(b);
      if (w.stat_h[b].nonfinite)
        return efail(err, errlen, C2D_E_STATE, "%s: a non-finite value appeared while '%s' was written", what, path);
      const size_t bytes = (size_t)(head + m * record);
      if (fwrite(w.pin[b], 1, bytes, f) != bytes)
        return efail(err, errlen, C2D_E_IO, "%s: cannot write '%s': %s", what, path, strerror(errno));
      { const int rc = write_side(b, m); if (rc) return rc; }
      T->io_ms += now_ms() - t1;
    }
  }
  return C2D_OK;
}

/* a text file: nothing before a chunk's records */
template <class Stat, class Times, class Produce, class CopyOut, class Counts, class WriteSide>
int write_chunks(TextStage<Stat>& w, hipStream_t stream, FILE* f, const char* what, const char* path, int record,
                 int64_t n, int64_t chunk, const Stat& init, Times* T, Produce&& produce, CopyOut&& copy_out,
                 Counts&& counts, WriteSide&& write_side, char* err, size_t errlen) {
  return write_chunks_headed(w, stream, f, what, path, record, 0, n, chunk, init, T, produce, copy_out, counts,
                             write_side, err, errlen);
}

}  // namespace c2d

#endif
