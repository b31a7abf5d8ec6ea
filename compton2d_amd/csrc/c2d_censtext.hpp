/*
 * c2d_censtext.hpp — the census record file (censtext.hip) as capi.cpp sees
 * it: plain records (d6, i5, key: the c2d_census_export layout) to the text
 * of write_cens and `<path>.keys`, and back.  Nothing here knows the grid or
 * the context's census; capi.cpp converts on either side.
 */
#ifndef C2D_CENSTEXT_HPP
#define C2D_CENSTEXT_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "c2d_textparse.hpp"   /* c2d_cens_times, c2d_cens_sink */

#define C2D_CENS_BLOCK 256   /* records per workgroup (29 696 B of text = 1 856 x 16 B) */

struct c2d_cens_file;   /* staging buffers of both directions, the powers-of-ten table on the device */

/* Queues, on the writer's stream, the work that fills records [first,
 * first + n) into the device arrays d6 [n][6], i5 [n][5], keys [n]. */
typedef int (*c2d_cens_source)(void* user, int64_t first, int64_t n, double* d6, int32_t* i5, uint64_t* keys);
/* n records to `path` and `path`.keys.  src != NULL: it supplies them chunk by
 * chunk (twice: the non-finite scan runs before either file is opened);
 * src == NULL: they are the host arrays h_d6, h_i5, h_keys. */
extern "C" int c2d_censtext_write(c2d_cens_file** w, int device, hipStream_t stream, c2d_cens_source src, void* user,
                                  const double* h_d6, const int32_t* h_i5, const uint64_t* h_keys, int64_t n,
                                  const char* path, c2d_cens_times* times, char* err, size_t errlen);
/* Parse `path` (keys from `path`.keys if it exists, else derived) and hand the
 * records to `sink` in order (NULL only counts).  *n_records = the records
 * delivered, also when the call fails. */
extern "C" int c2d_censtext_read(c2d_cens_file** r, int device, hipStream_t stream, const char* path,
                                 c2d_cens_sink sink, void* user, int64_t* n_records, c2d_cens_times* times,
                                 char* err, size_t errlen);
extern "C" void c2d_censtext_free(c2d_cens_file* f);

#endif
