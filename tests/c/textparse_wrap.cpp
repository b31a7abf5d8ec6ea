/* Host harness of compton2d_amd/csrc/c2d_textparse.hpp (C++17, g++, no HIP):
 * the host parsers of the event and census text files over a file path, for
 * tests/test_textparse_host.py.  The sinks append to the caller's arrays and
 * record the size of each delivery.  With -DTEXTPARSE_WRAP_MAIN it is a
 * stand-alone program over a list of files (the build the test runs under
 * -fsanitize=address,undefined): one line per file,
 *     E|C  chunk  base  want_rc  want_records  path
 * and it prints how many files gave another code or record count. */
#include <fcntl.h>

#include "../../compton2d_amd/csrc/c2d_textparse.hpp"

namespace {

struct Dst {
  double* d;            /* events [cap][7], or d6 [cap][6] */
  int32_t* i5;
  uint64_t* keys;
  int64_t cap, n;
  int64_t* sizes;       /* the size of each delivery, the first max_sizes of them */
  int32_t max_sizes, n_sizes;
  bool note(int64_t m) {
    if (n_sizes < max_sizes) sizes[n_sizes] = m;
    n_sizes++;
    return n + m <= cap;
  }
};

int ev_sink(void* user, const double* ev, int64_t m, int on_device) {
  Dst* d = static_cast<Dst*>(user);
  if (on_device || !d->note(m)) return C2D_E_ARG;
  memcpy(d->d + 7 * d->n, ev, (size_t)m * 7 * sizeof(double));
  d->n += m;
  return C2D_OK;
}

int cens_sink(void* user, const double* d6, const int32_t* i5, const uint64_t* keys, int64_t m, int on_device) {
  Dst* d = static_cast<Dst*>(user);
  if (on_device || !d->note(m)) return C2D_E_ARG;
  memcpy(d->d + 6 * d->n, d6, (size_t)m * 6 * sizeof(double));
  memcpy(d->i5 + 5 * d->n, i5, (size_t)m * 5 * sizeof(int32_t));
  memcpy(d->keys + d->n, keys, (size_t)m * sizeof(uint64_t));
  d->n += m;
  return C2D_OK;
}

}  // namespace

/* The event file from byte `off`, `chunk` records a delivery, into ev [cap][7].
 * *delivered = the parser's count, *n_sizes = the deliveries. */
extern "C" int tw_events(const char* path, int64_t off, int64_t chunk, double* ev, int64_t cap, int64_t* delivered,
                         int64_t* sizes, int32_t max_sizes, int32_t* n_sizes, char* err, int64_t errlen) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return C2D_E_ARG;
  Dst d = {ev, nullptr, nullptr, cap, 0, sizes, max_sizes, 0};
  c2d_evr_times T = {};
  *delivered = 0;
  const int rc = c2d::evr_host_parse(fd, off, chunk, ev_sink, &d, delivered, &T, path, err, (size_t)errlen);
  (void)close(fd);
  *n_sizes = d.n_sizes;
  if (!rc && (T.host_parsed != *delivered || d.n != *delivered)) return C2D_E_STATE;
  return rc;
}

/* The census file (keys from `path`.keys if it exists, else derived from the
 * record index, which starts at `base`) into d6 [cap][6], i5 [cap][5],
 * keys [cap].  *delivered - base = the records delivered. */
extern "C" int tw_census(const char* path, int64_t base, int64_t chunk, double* d6, int32_t* i5, uint64_t* keys,
                         int64_t cap, int64_t* delivered, int64_t* sizes, int32_t max_sizes, int32_t* n_sizes,
                         char* err, int64_t errlen) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return C2D_E_ARG;
  const int kfd = open((std::string(path) + ".keys").c_str(), O_RDONLY);
  Dst d = {d6, i5, keys, cap, 0, sizes, max_sizes, 0};
  c2d_cens_times T = {};
  *delivered = base;
  const int rc = c2d::cens_host_parse(fd, kfd, 0, chunk, cens_sink, &d, delivered, &T, path, err, (size_t)errlen);
  (void)close(fd);
  if (kfd >= 0) (void)close(kfd);
  *n_sizes = d.n_sizes;
  if (!rc && (T.host_records != *delivered - base || d.n != *delivered - base)) return C2D_E_STATE;
  return rc;
}

#ifdef TEXTPARSE_WRAP_MAIN
int main(int argc, char** argv) {
  FILE* list = argc == 2 ? fopen(argv[1], "r") : nullptr;
  if (!list) {
    printf("usage: %s LIST\n", argv[0]);
    return 2;
  }
  const int64_t cap = 4096;
  std::vector<double> d((size_t)cap * 7);
  std::vector<int32_t> i5((size_t)cap * 5);
  std::vector<uint64_t> keys((size_t)cap);
  int64_t sizes[8];
  int fails = 0, files = 0;
  char kind, path[1024], err[256];
  long long chunk, base, want_rc, want_n;
  while (fscanf(list, " %c %lld %lld %lld %lld %1023[^\n]", &kind, &chunk, &base, &want_rc, &want_n, path) == 6) {
    int64_t delivered = 0;
    int32_t n_sizes = 0;
    err[0] = 0;
    const int rc = kind == 'E' ? tw_events(path, base, chunk, d.data(), cap, &delivered, sizes, 8, &n_sizes, err, sizeof err)
                               : tw_census(path, base, chunk, d.data(), i5.data(), keys.data(), cap, &delivered, sizes,
                                           8, &n_sizes, err, sizeof err);
    const int64_t n = kind == 'E' ? delivered : delivered - base;
    files++;
    if (rc != want_rc || n != want_n) {
      printf("%s: code %d, %lld records; want %lld, %lld (%s)\n", path, rc, (long long)n, want_rc, want_n, err);
      fails++;
    }
  }
  (void)fclose(list);
  printf("%d files, %d failures\n", files, fails);
  return fails != 0;
}
#endif
