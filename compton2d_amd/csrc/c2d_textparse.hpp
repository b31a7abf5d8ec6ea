/*
 * c2d_textparse.hpp — the host side of the event and census text files that
 * needs no GPU: the small helpers the three routes share (evtext.hip,
 * evparse.hip, censtext.hip), the process-wide powers-of-ten table, and the
 * two host parsers that take what the device does not (the first record that
 * is not canonical and everything after it, or a tail shorter than a record).
 * Plain C++17 with no HIP include: tests/c/textparse_wrap.cpp compiles it
 * with g++, also under the host sanitizers.
 */
#ifndef C2D_TEXTPARSE_HPP
#define C2D_TEXTPARSE_HPP

#include <errno.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/compton2d.h"
#include "c2d_censfmt.h"

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

/* times and counts of the last c2d_censtext_write / c2d_censtext_read */
struct c2d_cens_times {
  double io_ms;       /* host: fwrite / read of the text and the keys                     */
  double wait_ms;     /* host: waiting for a chunk                                        */
  double kernel_ms;   /* device: the format or parse kernels                              */
  double conv_ms;     /* device: the record conversion (write: the source, both passes, and
                         the non-finite scan; read: added by the sink's owner)            */
  int64_t device_records, host_records;   /* read: parsed by the kernel / by the host parser */
  int32_t chunks;
};

/* Takes n records in file order, in device memory (on_device != 0: valid until
 * the sink returns and work it queued on the reader's stream has run) or in
 * host memory.  A non-zero return ends the read and is passed on. */
typedef int (*c2d_cens_sink)(void* user, const double* d6, const int32_t* i5, const uint64_t* keys, int64_t n,
                             int on_device);

namespace c2d {

inline int efail(char* err, size_t n, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (err && n) vsnprintf(err, n, fmt, ap);
  va_end(ap);
  return code;
}

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* up to `want` bytes, short only at the end of the file; -1 on error */
inline int64_t read_full(int fd, void* buf, int64_t want) {
  int64_t got = 0;
  while (got < want) {
    const ssize_t k = read(fd, (unsigned char*)buf + got, (size_t)std::min<int64_t>(want - got, (int64_t)1 << 30));
    if (k < 0) {
      if (errno == EINTR) continue;
      return -1;
    }
    if (k == 0) break;
    got += k;
  }
  return got;
}

inline bool is_blank(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

/* records per chunk: the environment variable `name`, read at every call (a
 * test knob), at most `bound` (0: no bound) */
inline int64_t chunk_env(const char* name, long long bound) {
  const char* e = getenv(name);
  if (e && *e) {
    const long long v = atoll(e);
    if (v >= 1) return (int64_t)(bound ? std::min(v, bound) : v);
  }
  return (int64_t)1 << 20;
}

/* the powers-of-ten table, built once per process */
inline const c2d_fmt_tab* fmt_tab() {
  static c2d_fmt_tab tab;
  static std::once_flag once;
  std::call_once(once, [] { c2d_fmt_tab_build(&tab); });
  return &tab;
}

/* the canonical E14.7 field with its pad restored: 14 bytes with the sign, or 13 without */
inline bool canonical_field(const char* t, int len, double* v) {
  char f[14];
  if (len == 14 && t[0] == '-') {
    memcpy(f, t, 14);
  } else if (len == 13) {
    f[0] = ' ';
    memcpy(f + 1, t, 13);
  } else {
    return false;
  }
  return c2d_scan_e14_7(fmt_tab(), f, v) >= 0;
}

/* ------------------------------------------------------------------------
 * Events: blank-separated tokens, each the canonical field, else strtod of
 * the whole token; groups of seven.
 * ---------------------------------------------------------------------- */
inline bool token_value(const char* t, int len, double* v) {
  if (canonical_field(t, len, v)) return true;
  char* end = nullptr;
  *v = strtod(t, &end);
  return len > 0 && end == t + len;
}

struct EvrHostParse {
  std::vector<double> ev;
  int64_t cap;                 /* events per delivery */
  c2d_evr_sink sink;
  void* user;
  int64_t* delivered;
  c2d_evr_times* T;
  /* the complete records gathered so far to the sink; an incomplete one stays */
  int flush() {
    const int64_t n = (int64_t)(ev.size() / 7);
    if (n == 0) return C2D_OK;
    const int rc = sink ? sink(user, ev.data(), n, 0) : C2D_OK;
    if (rc) return rc;
    *delivered += n;
    T->host_parsed += n;
    ev.erase(ev.begin(), ev.begin() + 7 * n);
    return C2D_OK;
  }
};

/* the event host parser from byte `off` to the end of the file */
inline int evr_host_parse(int fd, int64_t off, int64_t chunk, c2d_evr_sink sink, void* user, int64_t* delivered,
                          c2d_evr_times* T, const char* path, char* err, size_t errlen) {
  const double t0 = now_ms();
  if (lseek(fd, (off_t)off, SEEK_SET) < 0)
    return efail(err, errlen, C2D_E_IO, "events: cannot seek in '%s': %s", path, strerror(errno));
  EvrHostParse H{{}, chunk, sink, user, delivered, T};
  std::vector<unsigned char> buf((size_t)1 << 20);
  char tok[64];
  int tl = 0;
  bool too_long = false;
  int64_t pos = off, tok_off = off;
  int rc = C2D_OK;
  for (bool eof = false; !eof && !rc;) {
    const int64_t got = read_full(fd, buf.data(), (int64_t)buf.size());
    if (got < 0) {
      rc = efail(err, errlen, C2D_E_IO, "events: cannot read '%s': %s", path, strerror(errno));
      break;
    }
    eof = got < (int64_t)buf.size();
    for (int64_t i = 0; i <= got && !rc; i++) {
      const bool end_of_text = i == got;
      if (end_of_text && !eof) break;
      const unsigned char c = end_of_text ? ' ' : buf[(size_t)i];
      if (!is_blank(c)) {
        if (tl == 0) tok_off = pos + i;
        if (tl < (int)sizeof tok - 1) tok[tl++] = (char)c; else too_long = true;
        continue;
      }
      if (tl == 0) continue;
      tok[tl] = 0;
      double v = 0.0;
      if (too_long || !token_value(tok, tl, &v)) {
        rc = H.flush();   /* the records before it are delivered */
        if (!rc)
          rc = efail(err, errlen, C2D_E_IO, "events: '%s': token '%s%s' at byte offset %lld is not a number; "
                     "%lld record(s) before it were delivered", path, tok, too_long ? "..." : "", (long long)tok_off,
                     (long long)*delivered);
        break;
      }
      tl = 0;
      H.ev.push_back(v);
      if ((int64_t)H.ev.size() >= 7 * H.cap) rc = H.flush();
    }
    pos += got;
  }
  if (!rc) rc = H.flush();   /* a trailing group of fewer than seven values is dropped */
  T->host_parse_ms += now_ms() - t0;
  return rc;
}

/* ------------------------------------------------------------------------
 * Census: read_census's rules (compton2d_amd/census_io.py): CR stripped,
 * blank lines skipped, fixed 14- and 5-column fields, the E-less three-digit
 * exponent repaired, D or a lower-case e as the exponent letter, a missing
 * final newline.
 * ---------------------------------------------------------------------- */
/* columns [a, a + width) of the line without the blanks around them */
inline void columns(const std::string& s, size_t a, size_t width, const char** t, int* len) {
  size_t lo = std::min(a, s.size()), hi = std::min(a + width, s.size());
  while (lo < hi && is_blank((unsigned char)s[lo])) lo++;
  while (hi > lo && is_blank((unsigned char)s[hi - 1])) hi--;
  *t = s.data() + lo;
  *len = (int)(hi - lo);
}

/* one E field: the canonical field, else the E-less exponent repaired, D or d
 * as the exponent letter, and strtod of all of it */
inline bool double_field(const char* t, int len, double* v) {
  char f[24];
  if (len < 1 || len > 14) return false;
  if (canonical_field(t, len, v)) return true;
  int n = 0, last_sign = -1;
  bool has_e = false;
  for (int i = 0; i < len; i++) {
    char c = t[i];
    if (c == 'D' || c == 'd') c = 'E';
    if (c == 'E' || c == 'e') has_e = true;
    if ((c == '+' || c == '-') && i > 0) last_sign = n;
    f[n++] = c;
  }
  if (!has_e && last_sign > 0) {
    memmove(f + last_sign + 1, f + last_sign, (size_t)(n - last_sign));
    f[last_sign] = 'E';
    n++;
  }
  f[n] = 0;
  char* end = nullptr;
  *v = strtod(f, &end);
  return end == f + n;
}

/* one I5 field: an optional sign and digits */
inline bool int_field(const char* t, int len, int32_t* v) {
  int i = 0;
  bool neg = false;
  if (len > 0 && (t[0] == '-' || t[0] == '+')) { neg = t[0] == '-'; i = 1; }
  if (i >= len || len > 10) return false;
  int64_t a = 0;
  for (; i < len; i++) {
    if (t[i] < '0' || t[i] > '9') return false;
    a = a * 10 + (t[i] - '0');
  }
  *v = (int32_t)(neg ? -a : a);
  return true;
}

struct CensHostParse {
  std::vector<double> d6;
  std::vector<int32_t> i5;
  std::vector<int64_t> seed;
  std::vector<uint64_t> keys;
  int64_t cap;          /* records per delivery */
  int kfd;              /* the keys file, or -1 */
  c2d_cens_sink sink;
  void* user;
  int64_t* delivered;
  c2d_cens_times* T;
  const char* path;
  int flush(char* err, size_t errlen) {
    const int64_t n = (int64_t)seed.size();
    if (n == 0) return C2D_OK;
    keys.resize((size_t)n);
    if (kfd >= 0) {
      int64_t got = 0;
      while (got < 8 * n) {
        const ssize_t k = pread(kfd, (unsigned char*)keys.data() + got, (size_t)(8 * n - got),
                                (off_t)(8 * *delivered + got));
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) break;
        got += k;
      }
      if (got != 8 * n)
        return efail(err, errlen, C2D_E_IO, "census: '%s.keys' holds fewer keys than '%s' has records", path, path);
    } else {
      for (int64_t r = 0; r < n; r++) keys[(size_t)r] = c2d_cens_derive_key(seed[(size_t)r], *delivered + r);
    }
    const int rc = sink ? sink(user, d6.data(), i5.data(), keys.data(), n, 0) : C2D_OK;
    if (rc) return rc;
    *delivered += n;
    T->host_records += n;
    d6.clear();
    i5.clear();
    seed.clear();
    return C2D_OK;
  }
};

/* the census host parser from byte `off` (the start of a record) to the end of the file */
inline int cens_host_parse(int fd, int kfd, int64_t off, int64_t chunk, c2d_cens_sink sink, void* user,
                           int64_t* delivered, c2d_cens_times* T, const char* path, char* err, size_t errlen) {
  if (lseek(fd, (off_t)off, SEEK_SET) < 0)
    return efail(err, errlen, C2D_E_IO, "census: cannot seek in '%s': %s", path, strerror(errno));
  CensHostParse H{{}, {}, {}, {}, chunk, kfd, sink, user, delivered, T, path};
  std::vector<unsigned char> buf((size_t)1 << 20);
  std::string line, first;
  int64_t pos = off, line_off = off, first_off = 0;
  bool have_first = false;
  int rc = C2D_OK;
  for (bool eof = false; !eof && !rc;) {
    const int64_t got = read_full(fd, buf.data(), (int64_t)buf.size());
    if (got < 0) return efail(err, errlen, C2D_E_IO, "census: cannot read '%s': %s", path, strerror(errno));
    eof = got < (int64_t)buf.size();
    for (int64_t i = 0; i <= got && !rc; i++) {
      const bool end_of_text = i == got;
      if (end_of_text && !eof) break;
      if (!end_of_text && buf[(size_t)i] != '\n') {
        if (line.empty()) line_off = pos + i;
        if (line.size() < 4096) line.push_back((char)buf[(size_t)i]);
        continue;
      }
      /* a line ends here (or the text does: a missing final newline) */
      bool blank = true;
      for (char c : line) blank = blank && is_blank((unsigned char)c);
      if (blank) { line.clear(); continue; }
      if (!have_first) {
        first.swap(line);
        first_off = line_off;
        have_first = true;
        line.clear();
        continue;
      }
      have_first = false;
      const char* t;
      int len;
      for (int c = 0; c < 6 && !rc; c++) {
        double v = 0.0;
        columns(first, 14 * (size_t)c, 14, &t, &len);
        if (!double_field(t, len, &v))
          rc = efail(err, errlen, C2D_E_IO, "census: '%s': field '%.*s' at byte offset %lld is not a number", path, len,
                     t, (long long)(first_off + 14 * c));
        H.d6.push_back(v);
      }
      for (int c = 0; c < 6 && !rc; c++) {
        int32_t v = 0;
        columns(line, 5 * (size_t)c, 5, &t, &len);
        if (!int_field(t, len, &v))
          rc = efail(err, errlen, C2D_E_IO, "census: '%s': field '%.*s' at byte offset %lld is not an integer", path,
                     len, t, (long long)(line_off + 5 * c));
        if (c < 5) H.i5.push_back(v); else H.seed.push_back(v);
      }
      line.clear();
      if (!rc && (int64_t)H.seed.size() >= H.cap) rc = H.flush(err, errlen);
    }
    pos += got;
  }
  if (!rc && have_first)
    rc = efail(err, errlen, C2D_E_IO, "census: '%s': an odd number of lines: the record at byte offset %lld has no "
               "integer line", path, (long long)first_off);
  if (!rc) rc = H.flush(err, errlen);
  return rc;
}

}  // namespace c2d

#endif
