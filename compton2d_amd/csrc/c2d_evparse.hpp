/*
 * c2d_evparse.hpp — the escape-event text reader (evparse.hip) as capi.cpp
 * sees it: p###_evb.dat text in, events (7 x f64) out, chunk by chunk.
 */
#ifndef C2D_EVPARSE_HPP
#define C2D_EVPARSE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

struct c2d_evt_reader;   /* staging buffers, the powers-of-ten table on the device */

/* times and counts of the last c2d_evparse_file */
struct c2d_evr_times {
  double io_ms;            /* read() of the text                                 */
  double wait_ms;          /* host waiting for a chunk's copy and parse kernel   */
  double kernel_ms;        /* the parse kernels                                  */
  double host_parse_ms;    /* the host parser of what is not canonical           */
  int64_t canonical;       /* records parsed on the device                       */
  int64_t host_parsed;     /* records parsed on the host                         */
  int64_t exact_fields;    /* fields the device decided by the multi-limb path   */
  int32_t chunks;          /* device chunks                                      */
};

/* Takes n events in file order: in device memory (on_device != 0; valid
 * until the sink returns, and until work the sink queues on the reader's
 * stream has run) or in host memory.  A non-zero return ends the read and
 * is passed on. */
typedef int (*c2d_evr_sink)(void* user, const double* events, int64_t n, int on_device);

/* Parse `path` and hand its records to `sink` in order (sink == NULL only
 * counts).  *n_records = the records delivered, also when the call fails.
 * Returns a C2D_* code with its text in err.  *r is created on first use and
 * freed by c2d_evparse_free. */
extern "C" int c2d_evparse_file(c2d_evt_reader** r, int device, hipStream_t stream, const char* path,
                                c2d_evr_sink sink, void* user, int64_t* n_records, c2d_evr_times* times,
                                char* err, size_t errlen);
extern "C" void c2d_evparse_free(c2d_evt_reader* r);

#endif
