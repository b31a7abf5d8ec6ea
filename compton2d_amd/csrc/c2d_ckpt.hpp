/*
 * c2d_ckpt.hpp — the checkpoint file (ckpt.hip) as capi.cpp sees it: the
 * census through its chunk list into the file's chunks with their digests,
 * and a file's chunks verified and handed back as packed records.  Nothing
 * here knows the context; capi.cpp decides what a header must say, owns the
 * tables' staging and stores the records (c2d_census_append).
 */
#ifndef C2D_CKPT_HPP
#define C2D_CKPT_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "c2d_ckpt_host.h"
#include "c2d_device.hpp"

struct c2d_ckpt_stage;   /* the staging buffers of both directions */

/* times and counts of the last c2d_ckpt_write / c2d_ckpt_read */
struct c2d_ckpt_times {
  double io_ms;       /* host: fwrite / read                      */
  double wait_ms;     /* host: waiting for a chunk                */
  double kernel_ms;   /* device: the chunks' gather or verify kernels (not the scan before a write, not the tables) */
  int64_t bytes;      /* file bytes moved                         */
  int32_t chunks;     /* census chunks                            */
};

/* a table section: `words` f64 in device memory (read: where they are staged) */
struct c2d_ckpt_table {
  double* d;
  int64_t words;
};

/* n verified packed records in device memory, in file order; valid until the
 * sink returns and work it queued on the reader's stream has run */
typedef int (*c2d_ckpt_sink)(void* user, const uint64_t* d_rec, int64_t n);

/* The census cs[clist][0, n), the tables and the blob to `path` (through
 * `path`.tmp).  h: every field but chunk, the blob's and the header's digest
 * set by the caller.  Census records and tables are scanned for NaN/Inf
 * before the file is opened. */
extern "C" int c2d_ckpt_write(c2d_ckpt_stage** ps, int device, hipStream_t stream, c2d::CensusSoA cs,
                              const int32_t* clist, c2d_ckpt_header* h, const c2d_ckpt_table* tabs, int ntabs,
                              const void* user, const char* path, c2d_ckpt_times* times, char* err, size_t errlen);
/* The file of header h (c2d_ckpt_info_file's): the blob into user (NULL:
 * skipped; written only when the whole call has succeeded); the tables into tabs (ntabs = 0: skipped; else c2d_ckpt_tables'
 * count and sizes); census records [first, last) to the sink, chunk by chunk,
 * each chunk only after its digest and every record of it have passed.
 * *n_records = records handed over, also when the call fails. */
extern "C" int c2d_ckpt_read(c2d_ckpt_stage** ps, int device, hipStream_t stream, const char* path,
                             const c2d_ckpt_header* h, int64_t first, int64_t last, void* user, int64_t user_cap,
                             const c2d_ckpt_table* tabs, int ntabs, c2d_ckpt_sink sink, void* sink_user,
                             int64_t* n_records, c2d_ckpt_times* times, char* err, size_t errlen);
extern "C" void c2d_ckpt_free(c2d_ckpt_stage* s);

#endif
