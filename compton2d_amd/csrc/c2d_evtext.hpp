/*
 * c2d_evtext.hpp — the escape-event text writer (evtext.hip) as capi.cpp
 * sees it: event segments in, p###_evb.dat text out.
 */
#ifndef C2D_EVTEXT_HPP
#define C2D_EVTEXT_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#define C2D_EVT_MAXSEG 32     /* C2D_EV_SHARDS */
#define C2D_EVT_RECORD 105    /* 7 x 14 bytes, 6 blanks, newline */
#define C2D_EVT_BLOCK 256     /* events per workgroup (26 880 B of text, a multiple of 16) */

struct c2d_evt_writer;   /* staging buffers, the powers-of-ten table on the device */

/* device times and host I/O time of the last c2d_evtext_write */
struct c2d_evt_times {
  double kernel_ms, scan_ms, io_ms, wait_ms;
  int64_t ambiguous; /* values the kernel's fast path could not decide ... */
  int64_t multilimb; /* ... and of them, those decided by the multi-limb path */
  int32_t chunks;
};

/* Write `nseg` segments of events (seg[s]: cnt[s] events of 7 f64, all in
 * device memory, or nseg == 1 in host memory with on_device == 0) to `path`
 * in order.  Returns a C2D_* code with its text in err.  *w is created on
 * first use and freed by c2d_evtext_free. */
extern "C" int c2d_evtext_write(c2d_evt_writer** w, int device, hipStream_t stream, const double* const* seg,
                                const int64_t* cnt, int nseg, int on_device, const char* path, int append,
                                int64_t* n_written, c2d_evt_times* times, char* err, size_t errlen);
extern "C" void c2d_evtext_free(c2d_evt_writer* w);

#endif
