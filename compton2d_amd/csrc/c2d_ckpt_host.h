/*
 * c2d_ckpt_host.h — the checkpoint file (include/compton2d.h "Checkpoints",
 * DESIGN.md §4i) on the host: the header and trailer, the digest, and
 * c2d_checkpoint_info.  Plain C++17, no HIP: capi.cpp and ckpt.hip include
 * it, and so does a stand-alone program (tests/c/ckpt_main.cpp).  The
 * digest's two functions are also the kernels' (ckpt.hip).
 *
 * Everything in the file is little-endian and 8-byte aligned:
 *
 *   header    128 B   c2d_ckpt_header
 *   user blob         user_bytes, zero-padded to a multiple of 8
 *   kappa_prev        (C2D_CKPT_HAS_KAPPA)  a table section, ncell * 400 f64
 *   f_nt, Pnt         (C2D_CKPT_HAS_ELECTRONS) two table sections, ncell * 200 f64 each
 *   census            ceil(n_records / chunk) chunks, all of `chunk` records but the last
 *   trailer    24 B   c2d_ckpt_trailer
 *
 * A table section and a census chunk begin with the same 24 bytes, (count,
 * digest_sum, digest_xor): count is the section's f64 words or the chunk's
 * records; the words follow, 8 u64 a record (c2d_census_pack's).
 */
#ifndef C2D_CKPT_HOST_H
#define C2D_CKPT_HOST_H

#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/compton2d.h"
#include "c2d_rng.h"   /* c2d_mix64: SplitMix64's finaliser */

#define C2D_CKPT_MAGIC 0x0054504b43443243ull    /* "C2DCKPT\0" */
#define C2D_CKPT_TRAILER_MAGIC 0x00444e4543443243ull   /* "C2DCEND\0" */
#define C2D_CKPT_HEADER_BYTES 128
#define C2D_CKPT_HEAD_BYTES 24   /* (count, digest_sum, digest_xor) of a section or chunk */
#define C2D_CKPT_GOLDEN 0x9E3779B97F4A7C15ull
#define C2D_CKPT_CHUNK_MAX ((int64_t)1 << 24)   /* records per chunk: the writer's bound, and the reader's */

typedef struct c2d_ckpt_header {
  uint64_t magic;
  uint32_t version, header_bytes;
  int32_t nz, nr;
  int32_t nmu, encoded;          /* encoded: the census azimuth column is cos(phi) + C2D_CENS_ESW */
  uint64_t grid_digest;          /* digest_sum of z[nz] r[nr] rmin zmin E_ph[400] E_field[400] */
  uint64_t seed;
  int32_t rank, world;
  int32_t ncycle;                /* the clock of the last step (informational) */
  uint32_t sections;             /* C2D_CKPT_HAS_* */
  double time, dt;
  int64_t n_records, chunk;
  int32_t fp_auto_known, fp_auto_exact;
  int64_t user_bytes;
  uint64_t user_digest;          /* digest_sum of the padded blob */
  uint64_t header_digest;        /* digest_sum of the 15 words before this one */
} c2d_ckpt_header;

typedef struct c2d_ckpt_trailer {
  uint64_t magic;
  int64_t n_records;
  uint64_t digest;               /* c2d_ckpt_fold over the chunks' (sum, xor), in order */
} c2d_ckpt_trailer;

typedef struct c2d_ckpt_digest { uint64_t sum, x; } c2d_ckpt_digest;

#ifdef __cplusplus
static_assert(sizeof(c2d_ckpt_header) == C2D_CKPT_HEADER_BYTES, "the header is 16 words");
static_assert(sizeof(c2d_ckpt_trailer) == 24, "the trailer is 3 words");
#endif

/* the hash of group g (a census record, or 8 words of a table): a =
 * mix(g + golden), then a = mix(a ^ w_k) for the 8 words */
C2D_RHD uint64_t c2d_ckpt_hash_begin(uint64_t g) { return c2d_mix64(g + C2D_CKPT_GOLDEN); }
C2D_RHD uint64_t c2d_ckpt_hash_word(uint64_t a, uint64_t w) { return c2d_mix64(a ^ w); }

/* (sum, xor) of the hashes of n words in groups of 8 from group g0 on, the
 * last group zero-padded */
C2D_RHD c2d_ckpt_digest c2d_ckpt_digest_words(const uint64_t* w, int64_t n, uint64_t g0) {
  c2d_ckpt_digest d = {0ull, 0ull};
  for (int64_t i = 0; i < n; i += 8) {
    uint64_t a = c2d_ckpt_hash_begin(g0 + (uint64_t)(i >> 3));
    for (int k = 0; k < 8; k++) a = c2d_ckpt_hash_word(a, i + k < n ? w[i + k] : 0ull);
    d.sum += a;
    d.x ^= a;
  }
  return d;
}

/* the trailer's digest: t = mix(n_records + golden), then per chunk
 * t = mix(t ^ sum), t = mix(t ^ xor) */
C2D_RHD uint64_t c2d_ckpt_fold_begin(int64_t n_records) { return c2d_mix64((uint64_t)n_records + C2D_CKPT_GOLDEN); }
C2D_RHD uint64_t c2d_ckpt_fold(uint64_t t, uint64_t sum, uint64_t x) { return c2d_mix64(c2d_mix64(t ^ sum) ^ x); }

C2D_RHD uint64_t c2d_ckpt_header_digest(const c2d_ckpt_header* h) {
  uint64_t w[16];
  memcpy(w, h, sizeof w);
  return c2d_ckpt_digest_words(w, 15, 0ull).sum;
}

C2D_RHD int64_t c2d_ckpt_pad8(int64_t n) { return (n + 7) & ~(int64_t)7; }
C2D_RHD int64_t c2d_ckpt_nchunks(const c2d_ckpt_header* h) {
  return h->n_records > 0 ? (h->n_records + h->chunk - 1) / h->chunk : 0;
}
/* f64 words of the table sections, in file order; returns how many there are */
C2D_RHD int c2d_ckpt_tables(const c2d_ckpt_header* h, int64_t words[3]) {
  const int64_t nc = (int64_t)h->nz * h->nr;
  int n = 0;
  if (h->sections & C2D_CKPT_HAS_KAPPA) words[n++] = nc * C2D_N_VOL;
  if (h->sections & C2D_CKPT_HAS_ELECTRONS) {
    words[n++] = nc * C2D_NUM_NT;
    words[n++] = nc * C2D_NUM_NT;
  }
  return n;
}
/* byte offset of census chunk k */
C2D_RHD int64_t c2d_ckpt_chunk_offset(const c2d_ckpt_header* h, int64_t k) {
  int64_t words[3], off = C2D_CKPT_HEADER_BYTES + c2d_ckpt_pad8(h->user_bytes);
  const int nt = c2d_ckpt_tables(h, words);
  for (int i = 0; i < nt; i++) off += C2D_CKPT_HEAD_BYTES + 8 * words[i];
  return off + k * (C2D_CKPT_HEAD_BYTES + 8 * C2D_CENSUS_REC_WORDS * h->chunk);
}
/* the file's size: where the trailer ends */
C2D_RHD int64_t c2d_ckpt_file_bytes(const c2d_ckpt_header* h) {
  const int64_t nk = c2d_ckpt_nchunks(h);
  return c2d_ckpt_chunk_offset(h, 0) + nk * C2D_CKPT_HEAD_BYTES + 8 * C2D_CENSUS_REC_WORDS * h->n_records +
         (int64_t)sizeof(c2d_ckpt_trailer);
}

/* Why `bytes` bytes at p are not a header this version reads: NULL if they are */
C2D_RHD const char* c2d_ckpt_header_check(const void* p, int64_t bytes, c2d_ckpt_header* h) {
  if (bytes < C2D_CKPT_HEADER_BYTES) return "shorter than a header";
  memcpy(h, p, sizeof *h);
  if (h->magic != C2D_CKPT_MAGIC) return "not a checkpoint (magic)";
  if (h->version != C2D_CKPT_VERSION || h->header_bytes != C2D_CKPT_HEADER_BYTES) return "another format version";
  if (h->header_digest != c2d_ckpt_header_digest(h)) return "the header's digest does not match";
  if (h->nz < 1 || h->nz > C2D_MAXZONE || h->nr < 1 || h->nr > C2D_MAXZONE || h->nmu < 1 || h->nmu > C2D_NMUMAX ||
      h->n_records < 0 || h->chunk < 1 || h->chunk > C2D_CKPT_CHUNK_MAX || h->user_bytes < 0 ||
      (h->sections & ~(uint32_t)(C2D_CKPT_HAS_KAPPA | C2D_CKPT_HAS_ELECTRONS)) || h->n_records > ((int64_t)1 << 48) ||
      h->user_bytes > ((int64_t)1 << 48))
    return "a header field out of range";
  return NULL;
}

C2D_RHD void c2d_ckpt_info_from(const c2d_ckpt_header* h, c2d_ckpt_info* o) {
  memset(o, 0, sizeof *o);
  o->version = (int32_t)h->version;
  o->nz = h->nz; o->nr = h->nr; o->nmu = h->nmu;
  o->encoded = h->encoded;
  o->rank = h->rank; o->world = h->world;
  o->ncycle = h->ncycle;
  o->sections = (int32_t)h->sections;
  o->fp_auto_known = h->fp_auto_known; o->fp_auto_exact = h->fp_auto_exact;
  o->grid_digest = h->grid_digest;
  o->seed = h->seed;
  o->time = h->time; o->dt = h->dt;
  o->n_records = h->n_records; o->chunk = h->chunk;
  o->user_bytes = h->user_bytes;
  o->file_bytes = c2d_ckpt_file_bytes(h);
}

/* c2d_checkpoint_info's work: the header, the file's size against it and the
 * trailer.  msg (msglen > 0) takes why a file is refused. */
static inline int c2d_ckpt_info_file(const char* path, c2d_ckpt_info* out, c2d_ckpt_header* hdr, char* msg,
                                     size_t msglen) {
  if (msg && msglen) msg[0] = 0;
  FILE* f = fopen(path, "rb");
  if (!f) {
    if (msg) snprintf(msg, msglen, "checkpoint: cannot open '%s': %s", path, strerror(errno));
    return C2D_E_IO;
  }
  unsigned char buf[C2D_CKPT_HEADER_BYTES];
  const size_t got = fread(buf, 1, sizeof buf, f);
  c2d_ckpt_header h;
  const char* why = c2d_ckpt_header_check(buf, (int64_t)got, &h);
  c2d_ckpt_trailer t;
  if (!why) {
    const int64_t size = c2d_ckpt_file_bytes(&h);
    if (fseek(f, 0, SEEK_END) != 0 || (int64_t)ftell(f) != size)
      why = "the file's size is not what its header says (truncated?)";
    else if (fseek(f, (long)(size - (int64_t)sizeof t), SEEK_SET) != 0 || fread(&t, 1, sizeof t, f) != sizeof t)
      why = "the trailer cannot be read";
    else if (t.magic != C2D_CKPT_TRAILER_MAGIC)
      why = "the trailer's magic is wrong";
    else if (t.n_records != h.n_records)
      why = "the trailer's record count disagrees with the header's";
    else {   /* every chunk's head: its count, and the trailer's digest over them */
      uint64_t fold = c2d_ckpt_fold_begin(h.n_records);
      const int64_t nk = c2d_ckpt_nchunks(&h);
      for (int64_t k = 0; k < nk && !why; k++) {
        uint64_t head[3];
        const int64_t m = k + 1 < nk ? h.chunk : h.n_records - k * h.chunk;
        if (fseek(f, (long)c2d_ckpt_chunk_offset(&h, k), SEEK_SET) != 0 || fread(head, 1, sizeof head, f) != sizeof head)
          why = "a chunk's head cannot be read";
        else if ((int64_t)head[0] != m)
          why = "a chunk's record count is not what the header says";
        else
          fold = c2d_ckpt_fold(fold, head[1], head[2]);
      }
      if (!why && fold != t.digest) why = "the trailer's digest disagrees with the chunks' digests";
    }
  }
  fclose(f);
  if (why) {
    if (msg) snprintf(msg, msglen, "checkpoint '%s': %s", path, why);
    return C2D_E_IO;
  }
  if (out) c2d_ckpt_info_from(&h, out);
  if (hdr) *hdr = h;
  return C2D_OK;
}

#endif
