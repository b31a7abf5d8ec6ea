/*
 * ckpt.hip — the checkpoint file (include/compton2d.h "Checkpoints",
 * c2d_ckpt_host.h) on the device: the census gathered through its chunk list
 * into contiguous packed records with the chunk's digest in the same pass,
 * and a file's chunk verified (digest and every record) before anything is
 * stored.  Both directions stream through c2d_textio.hpp's two pinned host
 * buffers, a chunk of C2D_CKPT_CHUNK records at a time: a chunk's 24-byte
 * head (count, digest_sum, digest_xor) travels in front of its records, so
 * the staged bytes are the file's.
 *
 * The digest is a sum and an xor of per-record hashes (c2d_ckpt_host.h): a
 * lane hashes its records, a wave reduces its lanes' sums and xors with
 * shuffles, the workgroup's waves meet in LDS, and the workgroup stores its
 * two words in its own slot of a partials array; a one-workgroup kernel
 * folds the slots into the chunk's head (write) or compares them with it
 * (read).  No atomics: 16 384 waves adding to the same two words cost
 * 0.35 ms a launch, more than the records themselves.  The
 * order does not matter; numpy recomputes it (compton2d_amd/checkpoint.py).
 *
 * Nothing is indexed by what a file says: the verify kernel's addresses are
 * functions of the record count alone, and a record reaches the census only
 * after its cell, its bins and its doubles have been checked.
 */
#include "c2d_ckpt.hpp"

#include <fcntl.h>
#include <sys/stat.h>

#include <string>
#include <vector>

#include "c2d_textio.hpp"

namespace c2d {

struct CkptStat {
  unsigned long long nonfinite;    /* NaN/Inf values met                                              */
  unsigned long long first_bad;    /* write: the smallest 6 * record + field (tables: word) among them;
                                      read: the first record of the chunk that fails (~0: none)       */
  unsigned long long sum, x;       /* the digest of the table in work (c2d_ckpt_sum_kernel)           */
  unsigned long long digest_bad;   /* read: a chunk's digest or count was not its head's              */
};

constexpr int CKPT_BLOCK = 256;
constexpr int CKPT_MAXGRID = 4096;   /* workgroups of a digesting launch = slots of the partials array */
constexpr int CKPT_REC = 8 * C2D_CENSUS_REC_WORDS;   /* 64 bytes */

__device__ __forceinline__ bool ckpt_nonfinite(uint64_t w) { return ((w >> 52) & 0x7ffu) == 0x7ffu; }

/* the workgroup's (sum, xor) of its lanes' values, valid in thread 0: shuffles
 * within a wave, then the waves' words through LDS.  Every thread calls it. */
__device__ __forceinline__ void ckpt_block_reduce(unsigned long long& s, unsigned long long& x) {
  __shared__ unsigned long long red[2 * (CKPT_BLOCK / 64)];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    x ^= __shfl_xor(x, o, 64);
  }
  const int wv = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[2 * wv] = s;
    red[2 * wv + 1] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = 0ull;
    x = 0ull;
#pragma unroll
    for (int w = 0; w < CKPT_BLOCK / 64; w++) {
      s += red[2 * w];
      x ^= red[2 * w + 1];
    }
  }
}

/* the workgroup's digest into its slot of the partials array (every workgroup of the launch writes its own) */
__device__ __forceinline__ void ckpt_block_digest(unsigned long long s, unsigned long long x,
                                                  unsigned long long* __restrict__ part) {
  ckpt_block_reduce(s, x);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = s;
    part[2 * blockIdx.x + 1] = x;
  }
}

/* one workgroup: the digest of a launch of nblocks workgroups from their slots, valid in thread 0 */
__device__ __forceinline__ void ckpt_fold_partials(const unsigned long long* __restrict__ part, int nblocks,
                                                   unsigned long long& s, unsigned long long& x) {
  s = 0ull;
  x = 0ull;
  for (int i = (int)threadIdx.x; i < nblocks; i += CKPT_BLOCK) {
    s += part[2 * i];
    x ^= part[2 * i + 1];
  }
  ckpt_block_reduce(s, x);
}

/* Census records [first, first + m) through the chunk list, the census read
 * once with the census stream's non-temporal loads; NaN/Inf counted in st.
 * STORE: their packed words to out and the workgroup's digest to its slot of
 * part.  !STORE is the scan before the file is opened: no hash, no store.
 * Every thread stays in the loop to its end, so the reduction is over whole
 * workgroups. */
template <bool STORE>
__global__ void __launch_bounds__(CKPT_BLOCK)
c2d_ckpt_gather_kernel(CensusSoA cs, const int32_t* __restrict__ clist, int64_t first, int64_t m,
                       uint64_t* __restrict__ out, unsigned long long* __restrict__ part, CkptStat* st) {
  unsigned long long s = 0ull, x = 0ull;
  for (int64_t b0 = (int64_t)blockIdx.x * CKPT_BLOCK; b0 < m; b0 += (int64_t)gridDim.x * CKPT_BLOCK) {
    const int64_t i = b0 + threadIdx.x;
    if (i >= m) continue;
    const int64_t g = first + i;
    const int64_t slot = cens_slot(clist, g);
    const c2d_d2 rz = cld2_nt(cs.rz + slot), wp = cld2_nt(cs.wp + slot), ex = cld2_nt(cs.ex + slot);
    const c2d_u4 tg = cld4_nt(cs.tg + slot);
    uint64_t w[C2D_CENSUS_REC_WORDS];
    w[0] = (uint64_t)__double_as_longlong(rz.x);
    w[1] = (uint64_t)__double_as_longlong(rz.y);
    w[2] = (uint64_t)__double_as_longlong(wp.x);
    w[3] = (uint64_t)__double_as_longlong(wp.y);
    w[4] = (uint64_t)__double_as_longlong(ex.x);
    w[5] = (uint64_t)__double_as_longlong(ex.y);
    w[6] = (uint64_t)tg.x | ((uint64_t)tg.y << 32);
    w[7] = c2d_tg_key(tg);
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (ckpt_nonfinite(w[k])) {
        atomicAdd(&st->nonfinite, 1ull);
        atomicMin(&st->first_bad, (unsigned long long)(6 * g + k));
      }
    if (STORE) {
      uint64_t a = c2d_ckpt_hash_begin((uint64_t)g);
#pragma unroll
      for (int k = 0; k < C2D_CENSUS_REC_WORDS; k++) a = c2d_ckpt_hash_word(a, w[k]);
      s += a;
      x ^= a;
      uint64_t* o = out + i * C2D_CENSUS_REC_WORDS;
#pragma unroll
      for (int k = 0; k < C2D_CENSUS_REC_WORDS; k++) o[k] = w[k];   /* plain: a lane's 64 bytes meet in L2 */
    }
  }
  if (STORE) ckpt_block_digest(s, x, part);
}

/* n f64 words in groups of 8 (group g0 first, the last zero-padded): their
 * digest, and the NaN/Inf among them */
__global__ void __launch_bounds__(CKPT_BLOCK)
c2d_ckpt_words_kernel(const uint64_t* __restrict__ w, int64_t n, unsigned long long* __restrict__ part,
                      CkptStat* st) {
  const int64_t ngroups = (n + 7) >> 3;
  unsigned long long s = 0ull, x = 0ull;
  for (int64_t b0 = (int64_t)blockIdx.x * CKPT_BLOCK; b0 < ngroups; b0 += (int64_t)gridDim.x * CKPT_BLOCK) {
    const int64_t g = b0 + threadIdx.x;
    if (g >= ngroups) continue;
    uint64_t a = c2d_ckpt_hash_begin((uint64_t)g);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int64_t i = 8 * g + k;
      const uint64_t v = i < n ? w[i] : 0ull;
      a = c2d_ckpt_hash_word(a, v);
      if (ckpt_nonfinite(v)) {
        atomicAdd(&st->nonfinite, 1ull);
        atomicMin(&st->first_bad, (unsigned long long)i);
      }
    }
    s += a;
    x ^= a;
  }
  ckpt_block_digest(s, x, part);
}

/* The m staged records of a file's chunk (the first is record g0 of the
 * census): their digest, and each record as a file must be checked before a
 * kernel indexes tables with what it holds.  Lowers first_bad to the first
 * record of the chunk that fails. */
__global__ void __launch_bounds__(CKPT_BLOCK)
c2d_ckpt_verify_kernel(const uint64_t* __restrict__ rec, int64_t g0, int64_t m, int nz, int nr, int nmu,
                       unsigned long long* __restrict__ part, CkptStat* st) {
  unsigned long long s = 0ull, x = 0ull;
  for (int64_t b0 = (int64_t)blockIdx.x * CKPT_BLOCK; b0 < m; b0 += (int64_t)gridDim.x * CKPT_BLOCK) {
    const int64_t i = b0 + threadIdx.x;
    if (i >= m) continue;
    const uint64_t* r = rec + i * C2D_CENSUS_REC_WORDS;
    uint64_t w[C2D_CENSUS_REC_WORDS];
#pragma unroll
    for (int k = 0; k < C2D_CENSUS_REC_WORDS; k++) w[k] = r[k];
    uint64_t a = c2d_ckpt_hash_begin((uint64_t)(g0 + i));
    bool ok = true;
#pragma unroll
    for (int k = 0; k < C2D_CENSUS_REC_WORDS; k++) {
      a = c2d_ckpt_hash_word(a, w[k]);
      if (k < 6) ok = ok && !ckpt_nonfinite(w[k]);
    }
    s += a;
    x ^= a;
    const uint32_t jk = (uint32_t)(w[6] & 0xffffffffull), bins = (uint32_t)(w[6] >> 32);
    const int ie = c2d_cens_ie(jk), efl = c2d_cens_efl(jk), j = c2d_cens_j(jk), kk = c2d_cens_k(jk);
    ok = ok && j >= 1 && j <= nz && kk >= 1 && kk <= nr && ie >= 1 && ie <= C2D_N_VOL && efl <= C2D_NPHFIELD;
    /* jgpsp, jgplc, jgpmu index fout(mu, jgpsp) and edout(mu, jgplc) at an escape; no dead slot */
    ok = ok && (bins & 0xffu) <= (uint32_t)C2D_NPHOMAX && ((bins >> 8) & 0xffu) <= (uint32_t)C2D_NPHLCMAX &&
         ((bins >> 16) & 0xffu) <= (uint32_t)nmu && !(bins & C2D_CENS_DEAD);
    if (!ok) atomicMin(&st->first_bad, (unsigned long long)i);
  }
  ckpt_block_digest(s, x, part);
}

/* The three below are one workgroup of CKPT_BLOCK threads each, after a launch of nblocks workgroups. */
/* write: the chunk's head in front of its records */
__global__ void __launch_bounds__(CKPT_BLOCK)
c2d_ckpt_head_kernel(uint64_t* head, int64_t m, const unsigned long long* __restrict__ part, int nblocks) {
  unsigned long long s, x;
  ckpt_fold_partials(part, nblocks, s, x);
  if (threadIdx.x != 0) return;
  head[0] = (uint64_t)m;
  head[1] = s;
  head[2] = x;
}

/* read: the chunk's digest against its head; a chunk that fails stores nothing */
__global__ void __launch_bounds__(CKPT_BLOCK)
c2d_ckpt_match_kernel(const uint64_t* head, int64_t m, const unsigned long long* __restrict__ part, int nblocks,
                      CkptStat* st) {
  unsigned long long s, x;
  ckpt_fold_partials(part, nblocks, s, x);
  if (threadIdx.x != 0) return;
  if (head[0] != (uint64_t)m || head[1] != s || head[2] != x) {
    st->digest_bad = 1ull;
    st->first_bad = 0ull;
  }
}

/* a table's digest into the status */
__global__ void __launch_bounds__(CKPT_BLOCK)
c2d_ckpt_sum_kernel(const unsigned long long* __restrict__ part, int nblocks, CkptStat* st) {
  unsigned long long s, x;
  ckpt_fold_partials(part, nblocks, s, x);
  if (threadIdx.x != 0) return;
  st->sum = s;
  st->x = x;
}

}  // namespace c2d

using namespace c2d;

struct c2d_ckpt_stage {
  TextStage<CkptStat> st;   /* "text": a chunk's head and records, the file's bytes */
  unsigned long long* part_d = nullptr;   /* [CKPT_MAXGRID][2]: the workgroups' digests of the launch in work */
};

namespace {

constexpr CkptStat CKPT_STAT0 = {0ull, ~0ull, 0ull, 0ull, 0ull};

unsigned ckpt_grid(int64_t items) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + CKPT_BLOCK - 1) / CKPT_BLOCK, CKPT_MAXGRID));
}

int ensure(c2d_ckpt_stage** ps, int device, int64_t records, char* err, size_t errlen) {
  if (!*ps) {
    *ps = new c2d_ckpt_stage;
    (*ps)->st.device = device;
  }
  if (!(*ps)->part_d) C2D_TXCHK(hipMalloc((void**)&(*ps)->part_d, sizeof(unsigned long long) * 2 * CKPT_MAXGRID));
  /* one record more: room for the chunk's head */
  return (*ps)->st.ensure(records + 1, CKPT_REC, false, [](int64_t) { return C2D_OK; }, err, errlen);
}

/* the status after the queued work, on the host */
int fetch_stat(TextStage<CkptStat>& st, hipStream_t stream, CkptStat* out, char* err, size_t errlen) {
  C2D_TXCHK(hipMemcpyAsync(&st.stat_h[0], st.stat_d, sizeof(CkptStat), hipMemcpyDeviceToHost, stream));
  C2D_TXCHK(hipStreamSynchronize(stream));
  *out = st.stat_h[0];
  return C2D_OK;
}

/* digest and NaN/Inf count of `words` f64 in device memory */
int table_digest(c2d_ckpt_stage* s, hipStream_t stream, const double* d, int64_t words, CkptStat* out, char* err,
                 size_t errlen) {
  TextStage<CkptStat>& st = s->st;
  { const int rc = st.reset(stream, CKPT_STAT0, err, errlen); if (rc) return rc; }
  { const int rc = st.timed(stream, 0, [&] {
      const unsigned grid = ckpt_grid((words + 7) / 8);
      hipLaunchKernelGGL(c2d_ckpt_words_kernel, dim3(grid), dim3(CKPT_BLOCK), 0, stream,
                         reinterpret_cast<const uint64_t*>(d), words, s->part_d, st.stat_d);
      hipLaunchKernelGGL(c2d_ckpt_sum_kernel, dim3(1), dim3(CKPT_BLOCK), 0, stream, s->part_d, (int)grid, st.stat_d);
    }, err, errlen); if (rc) return rc; }
  return fetch_stat(st, stream, out, err, errlen);
}

int write_body(c2d_ckpt_stage* s, hipStream_t stream, CensusSoA cs, const int32_t* clist, const c2d_ckpt_header* h,
               const c2d_ckpt_table* tabs, const CkptStat* tab_stat, int ntabs, const void* user, FILE* f,
               const char* path, c2d_ckpt_times* T, char* err, size_t errlen) {
  TextStage<CkptStat>& st = s->st;
  auto put = [&](const void* p, size_t bytes) {
    const double t0 = now_ms();
    const bool ok = bytes == 0 || fwrite(p, 1, bytes, f) == bytes;
    T->io_ms += now_ms() - t0;
    T->bytes += (int64_t)bytes;
    return ok ? C2D_OK : efail(err, errlen, C2D_E_IO, "checkpoint: cannot write '%s': %s", path, strerror(errno));
  };
  { const int rc = put(h, sizeof *h); if (rc) return rc; }
  {
    std::vector<unsigned char> blob((size_t)c2d_ckpt_pad8(h->user_bytes), 0);
    if (h->user_bytes) memcpy(blob.data(), user, (size_t)h->user_bytes);
    const int rc = put(blob.data(), blob.size());
    if (rc) return rc;
  }
  std::vector<double> host;
  for (int i = 0; i < ntabs; i++) {
    host.resize((size_t)tabs[i].words);
    C2D_TXCHK(hipMemcpyAsync(host.data(), tabs[i].d, sizeof(double) * host.size(), hipMemcpyDeviceToHost, stream));
    C2D_TXCHK(hipStreamSynchronize(stream));
    const uint64_t head[3] = {(uint64_t)tabs[i].words, tab_stat[i].sum, tab_stat[i].x};
    if (c2d_ckpt_digest_words(reinterpret_cast<const uint64_t*>(host.data()), tabs[i].words, 0ull).sum != head[1])
      return efail(err, errlen, C2D_E_STATE, "checkpoint: a table changed while '%s' was written", path);
    { const int rc = put(head, sizeof head); if (rc) return rc; }
    { const int rc = put(host.data(), sizeof(double) * host.size()); if (rc) return rc; }
  }
  uint64_t fold = c2d_ckpt_fold_begin(h->n_records);
  if (h->n_records > 0) {
    uint64_t* head_d = reinterpret_cast<uint64_t*>(st.text_d);
    auto produce = [&](int b, int64_t c0, int64_t m) {
      return st.timed(stream, b, [&] {
        const unsigned grid = ckpt_grid(m);
        hipLaunchKernelGGL(c2d_ckpt_gather_kernel<true>, dim3(grid), dim3(CKPT_BLOCK), 0, stream, cs, clist, c0, m,
                           head_d + 3, s->part_d, st.stat_d);
        hipLaunchKernelGGL(c2d_ckpt_head_kernel, dim3(1), dim3(CKPT_BLOCK), 0, stream, head_d, m, s->part_d,
                           (int)grid);
      }, err, errlen);
    };
    auto copy_out = [&](int, int64_t) { return C2D_OK; };
    auto counts = [&](int b) {   /* the chunk's head is in the pinned buffer: the trailer's digest takes it */
      const uint64_t* head = reinterpret_cast<const uint64_t*>(st.pin[b]);
      fold = c2d_ckpt_fold(fold, head[1], head[2]);
    };
    auto write_side = [&](int, int64_t m) {
      T->bytes += C2D_CKPT_HEAD_BYTES + m * CKPT_REC;
      return C2D_OK;
    };
    const int rc = write_chunks_headed(st, stream, f, "checkpoint", path, CKPT_REC, C2D_CKPT_HEAD_BYTES, h->n_records,
                                       h->chunk, CKPT_STAT0, T, produce, copy_out, counts, write_side, err, errlen);
    if (rc) return rc;
  }
  const c2d_ckpt_trailer t = {C2D_CKPT_TRAILER_MAGIC, h->n_records, fold};
  return put(&t, sizeof t);
}

}  // namespace

extern "C" int c2d_ckpt_write(c2d_ckpt_stage** ps, int device, hipStream_t stream, CensusSoA cs, const int32_t* clist,
                              c2d_ckpt_header* h, const c2d_ckpt_table* tabs, int ntabs, const void* user,
                              const char* path, c2d_ckpt_times* times, char* err, size_t errlen) {
  c2d_ckpt_times T = {};
  const int64_t n = h->n_records;
  h->chunk = chunk_env("C2D_CKPT_CHUNK", (long long)C2D_CKPT_CHUNK_MAX);
  { const int rc = ensure(ps, device, std::max<int64_t>(1, std::min(h->chunk, n)), err, errlen); if (rc) return rc; }
  TextStage<CkptStat>& st = (*ps)->st;
  /* before the file is opened: NaN/Inf in the tables (their digests on the way) and in the census */
  CkptStat tab_stat[3] = {};
  if (ntabs > 3) return efail(err, errlen, C2D_E_ARG, "checkpoint: %d table sections", ntabs);
  for (int i = 0; i < ntabs; i++) {
    const int rc = table_digest(*ps, stream, tabs[i].d, tabs[i].words, &tab_stat[i], err, errlen);
    if (rc) return rc;
    if (tab_stat[i].nonfinite)
      return efail(err, errlen, C2D_E_NONFINITE, "checkpoint: %llu non-finite value(s) in table section %d; the first "
                   "at word %llu; the file was not touched", tab_stat[i].nonfinite, i, tab_stat[i].first_bad);
  }
  if (n > 0) {
    { const int rc = st.reset(stream, CKPT_STAT0, err, errlen); if (rc) return rc; }
    { const int rc = st.timed(stream, 0, [&] {
        for (int64_t c0 = 0; c0 < n; c0 += h->chunk) {
          const int64_t m = std::min(h->chunk, n - c0);
          hipLaunchKernelGGL(c2d_ckpt_gather_kernel<false>, dim3(ckpt_grid(m)), dim3(CKPT_BLOCK), 0, stream, cs, clist,
                             c0, m, (uint64_t*)nullptr, (unsigned long long*)nullptr, st.stat_d);
        }
      }, err, errlen); if (rc) return rc; }
    CkptStat scan;
    { const int rc = fetch_stat(st, stream, &scan, err, errlen); if (rc) return rc; }
    if (scan.nonfinite)
      return efail(err, errlen, C2D_E_NONFINITE, "checkpoint: %llu non-finite value(s) in the census; the first in "
                   "record %llu (counted from 1), field %llu; the file was not touched", scan.nonfinite,
                   scan.first_bad / 6ull + 1ull, scan.first_bad % 6ull + 1ull);
  }
  h->user_digest = 0ull;
  {
    std::vector<uint64_t> blob((size_t)(c2d_ckpt_pad8(h->user_bytes) / 8), 0ull);
    if (h->user_bytes) memcpy(blob.data(), user, (size_t)h->user_bytes);
    h->user_digest = c2d_ckpt_digest_words(blob.data(), (int64_t)blob.size(), 0ull).sum;
  }
  h->header_digest = c2d_ckpt_header_digest(h);
  struct stat sb;
  const bool in_place = stat(path, &sb) == 0 && !S_ISREG(sb.st_mode);   /* a device: nothing to rename over */
  const std::string tmp = in_place ? std::string(path) : std::string(path) + ".tmp";
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) return efail(err, errlen, C2D_E_IO, "checkpoint: cannot open '%s': %s", tmp.c_str(), strerror(errno));
  setvbuf(f, nullptr, _IONBF, 0);   /* the chunks are the buffer */
  int rc = write_body(*ps, stream, cs, clist, h, tabs, tab_stat, ntabs, user, f, tmp.c_str(), &T, err, errlen);
  if (rc) (void)hipStreamSynchronize(stream);   /* nothing in flight into the staging buffers */
  /* on the disk before it takes the older file's name: a machine that goes down keeps one of the two whole */
  if (!rc && !in_place && (fflush(f) != 0 || fsync(fileno(f)) != 0))
    rc = efail(err, errlen, C2D_E_IO, "checkpoint: cannot flush '%s': %s", tmp.c_str(), strerror(errno));
  if (fclose(f) != 0 && !rc)
    rc = efail(err, errlen, C2D_E_IO, "checkpoint: cannot close '%s': %s", tmp.c_str(), strerror(errno));
  if (!rc && !in_place && rename(tmp.c_str(), path) != 0)
    rc = efail(err, errlen, C2D_E_IO, "checkpoint: cannot rename '%s' to '%s': %s", tmp.c_str(), path,
               strerror(errno));
  if (rc && !in_place) (void)remove(tmp.c_str());
  if (times) *times = T;
  return rc;
}

extern "C" int c2d_ckpt_read(c2d_ckpt_stage** ps, int device, hipStream_t stream, const char* path,
                             const c2d_ckpt_header* h, int64_t first, int64_t last, void* user, int64_t user_cap,
                             const c2d_ckpt_table* tabs, int ntabs, c2d_ckpt_sink sink, void* sink_user,
                             int64_t* n_records, c2d_ckpt_times* times, char* err, size_t errlen) {
  c2d_ckpt_times T = {};
  int64_t delivered = 0;
  if (n_records) *n_records = 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return efail(err, errlen, C2D_E_IO, "checkpoint: cannot open '%s': %s", path, strerror(errno));
  std::vector<uint64_t> blob;   /* handed to the caller only when the whole call has succeeded */
  auto finish = [&](int rc) {
    (void)close(fd);
    if (!rc && user && user_cap > 0 && h->user_bytes > 0)
      memcpy(user, blob.data(), (size_t)std::min(user_cap, h->user_bytes));
    if (n_records) *n_records = delivered;
    if (times) *times = T;
    return rc;
  };
  auto get = [&](void* p, int64_t bytes, int64_t off, const char* what) {
    const double t0 = now_ms();
    const bool ok = lseek(fd, (off_t)off, SEEK_SET) == (off_t)off && read_full(fd, p, bytes) == bytes;
    T.io_ms += now_ms() - t0;
    T.bytes += bytes;
    return ok ? C2D_OK
              : efail(err, errlen, C2D_E_IO, "checkpoint '%s': cannot read %s (%lld bytes at offset %lld)", path, what,
                      (long long)bytes, (long long)off);
  };
  const int64_t chunk = h->chunk, nk = c2d_ckpt_nchunks(h);
  const bool some = first < last;
  const int64_t k0 = some ? first / chunk : 0, k1 = some ? (last - 1) / chunk + 1 : 0;   /* the chunks that cover it */
  { const int rc = ensure(ps, device, std::max<int64_t>(1, std::min(chunk, h->n_records)), err, errlen);
    if (rc) return finish(rc); }
  TextStage<CkptStat>& st = (*ps)->st;
  int64_t off = C2D_CKPT_HEADER_BYTES;
  {   /* the blob */
    blob.assign((size_t)(c2d_ckpt_pad8(h->user_bytes) / 8), 0ull);
    if (!blob.empty()) {
      const int rc = get(blob.data(), 8 * (int64_t)blob.size(), off, "the user blob");
      if (rc) return finish(rc);
    }
    if (c2d_ckpt_digest_words(blob.data(), (int64_t)blob.size(), 0ull).sum != h->user_digest)
      return finish(efail(err, errlen, C2D_E_IO, "checkpoint '%s': the user blob's digest does not match (offset %lld)",
                          path, (long long)off));
    off += 8 * (int64_t)blob.size();
  }
  {   /* the tables into the caller's staging, each against its head */
    int64_t words[3];
    const int nt = c2d_ckpt_tables(h, words);
    std::vector<double> host;
    for (int i = 0; i < nt; i++) {
      if (ntabs) {
        if (ntabs != nt || tabs[i].words != words[i])
          return finish(efail(err, errlen, C2D_E_ARG, "checkpoint: table section %d of %lld words, %lld expected", i,
                              (long long)(ntabs == nt ? tabs[i].words : -1), (long long)words[i]));
        uint64_t head[3];
        { const int rc = get(head, sizeof head, off, "a table's head"); if (rc) return finish(rc); }
        host.resize((size_t)words[i]);
        { const int rc = get(host.data(), 8 * words[i], off + C2D_CKPT_HEAD_BYTES, "a table");
          if (rc) return finish(rc); }
        hipError_t e = hipMemcpyAsync(tabs[i].d, host.data(), 8 * (size_t)words[i], hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess)
          return finish(efail(err, errlen, C2D_E_HIP, "checkpoint: staging a table: %s", hipGetErrorString(e)));
        CkptStat ts;
        { const int rc = table_digest(*ps, stream, tabs[i].d, words[i], &ts, err, errlen);
          if (rc) return finish(rc); }
        if ((int64_t)head[0] != words[i] || head[1] != ts.sum || head[2] != ts.x || ts.nonfinite)
          return finish(efail(err, errlen, C2D_E_IO, "checkpoint '%s': table section %d at offset %lld fails its "
                              "check (%s)", path, i, (long long)off,
                              ts.nonfinite ? "a non-finite value" : "digest or size"));
      }
      off += C2D_CKPT_HEAD_BYTES + 8 * words[i];
    }
  }
  int rc = C2D_OK;
  if (k1 > k0) {
    const int64_t base = c2d_ckpt_chunk_offset(h, k0);
    if (lseek(fd, (off_t)base, SEEK_SET) != (off_t)base)
      return finish(efail(err, errlen, C2D_E_IO, "checkpoint: cannot seek in '%s': %s", path, strerror(errno)));
    auto records_of = [&](int64_t k) { return k + 1 < nk ? chunk : h->n_records - k * chunk; };
    int64_t k_side = k0, k_done = k0;   /* the chunk read last, and the one retired next */
    auto bad_chunk = [&](int64_t k, const char* why) {
      return efail(err, errlen, C2D_E_IO, "checkpoint '%s': chunk %lld at byte offset %lld %s; nothing of it was "
                   "stored", path, (long long)k, (long long)c2d_ckpt_chunk_offset(h, k), why);
    };
    auto want = [&](int64_t k) { return k0 + k < k1 ? C2D_CKPT_HEAD_BYTES + CKPT_REC * records_of(k0 + k) : 0; };
    auto side = [&](int b, int64_t n) {   /* the head's count is the header's, or nothing of it is touched */
      const int64_t k = k_side++;
      T.bytes += C2D_CKPT_HEAD_BYTES + n * CKPT_REC;
      if (n != records_of(k) || reinterpret_cast<const uint64_t*>(st.pin[b])[0] != (uint64_t)n)
        return bad_chunk(k, "is truncated or holds another count than its header says");
      return C2D_OK;
    };
    const uint64_t* head_d = reinterpret_cast<const uint64_t*>(st.text_d);
    unsigned long long* part_d = (*ps)->part_d;
    auto enqueue = [&](int b, int64_t n, int64_t k) {
      return st.timed(stream, b, [&] {
        const unsigned grid = ckpt_grid(n);
        hipLaunchKernelGGL(c2d_ckpt_verify_kernel, dim3(grid), dim3(CKPT_BLOCK), 0, stream, head_d + 3,
                           (k0 + k) * chunk, n, (int)h->nz, (int)h->nr, (int)h->nmu, part_d, st.stat_d);
        hipLaunchKernelGGL(c2d_ckpt_match_kernel, dim3(1), dim3(CKPT_BLOCK), 0, stream, head_d, n, part_d, (int)grid,
                           st.stat_d);
      }, err, errlen);
    };
    auto deliver = [&](int b, int64_t good) {
      const int64_t k = k_done++, n = records_of(k), c0 = k * chunk;
      if (good < n) {
        char why[96];
        if (st.stat_h[b].digest_bad) snprintf(why, sizeof why, "fails its digest");
        else snprintf(why, sizeof why, "holds a record out of range or not finite (record %lld of it)", (long long)good);
        return bad_chunk(k, why);
      }
      const int64_t lo = std::max(first, c0) - c0, hi = std::min(last, c0 + n) - c0;
      if (hi > lo && sink) {
        const int rc = sink(sink_user, head_d + 3 + lo * C2D_CENSUS_REC_WORDS, hi - lo);
        if (rc) return rc;
      }
      delivered += hi - lo;
      return C2D_OK;
    };
    auto host = [&](int64_t) { return bad_chunk(k_side, "is truncated"); };
    rc = read_chunks_sized(st, stream, fd, "checkpoint", path, CKPT_REC, C2D_CKPT_HEAD_BYTES, want, CKPT_STAT0, &T,
                           side, enqueue, deliver, host, err, errlen);
    if (rc) (void)hipStreamSynchronize(stream);   /* nothing in flight out of the staging buffers */
  }
  return finish(rc);
}

extern "C" void c2d_ckpt_free(c2d_ckpt_stage* s) {
  if (!s) return;
  (void)hipSetDevice(s->st.device);
  s->st.release();
  if (s->part_d) (void)hipFree(s->part_d);
  delete s;
}
