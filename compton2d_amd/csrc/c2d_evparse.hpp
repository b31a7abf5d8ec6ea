/*
 * c2d_evparse.hpp — the escape-event text reader (evparse.hip) as capi.cpp
 * sees it: p###_evb.dat text in, events (7 x f64) out, chunk by chunk.
 */
#ifndef C2D_EVPARSE_HPP
#define C2D_EVPARSE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "c2d_textparse.hpp"   /* c2d_evr_times, c2d_evr_sink */

struct c2d_evt_reader;   /* staging buffers, the powers-of-ten table on the device */

/* Parse `path` and hand its records to `sink` in order (sink == NULL only
 * counts).  *n_records = the records delivered, also when the call fails.
 * Returns a C2D_* code with its text in err.  *r is created on first use and
 * freed by c2d_evparse_free. */
extern "C" int c2d_evparse_file(c2d_evt_reader** r, int device, hipStream_t stream, const char* path,
                                c2d_evr_sink sink, void* user, int64_t* n_records, c2d_evr_times* times,
                                char* err, size_t errlen);
extern "C" void c2d_evparse_free(c2d_evt_reader* r);

#endif
