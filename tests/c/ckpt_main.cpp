/*
 * ckpt_main.cpp — the host side of the checkpoint file
 * (compton2d_amd/csrc/c2d_ckpt_host.h) as a stand-alone program, for a build
 * with -fsanitize=address,undefined (tests/test_checkpoint_host.py).
 *
 *   ckpt_main info <file>
 *       one line: code, then the header's fields (code 0 only)
 *   ckpt_main list <list file>
 *       lines of "<expected code> <expected n_records> <path>": every file
 *       through c2d_ckpt_info_file; prints "<n> files, <k> failures"
 *   ckpt_main digest <g0> <word> ...
 *       "sum xor" of the words' digest (hex words)
 */
#include <inttypes.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../compton2d_amd/csrc/c2d_ckpt_host.h"

static int info(const char* path) {
  c2d_ckpt_info o;
  char msg[512];
  const int rc = c2d_ckpt_info_file(path, &o, nullptr, msg, sizeof msg);
  if (rc) {
    printf("%d %s\n", rc, msg);
    return 0;
  }
  printf("0 version=%d nz=%d nr=%d nmu=%d encoded=%d rank=%d world=%d ncycle=%d sections=%d fp_auto_known=%d "
         "fp_auto_exact=%d grid_digest=%" PRIu64 " seed=%" PRIu64 " time=%.17g dt=%.17g n_records=%" PRId64
         " chunk=%" PRId64 " user_bytes=%" PRId64 " file_bytes=%" PRId64 "\n",
         o.version, o.nz, o.nr, o.nmu, o.encoded, o.rank, o.world, o.ncycle, o.sections, o.fp_auto_known,
         o.fp_auto_exact, o.grid_digest, o.seed, o.time, o.dt, o.n_records, o.chunk, o.user_bytes, o.file_bytes);
  return 0;
}

static int list(const char* lst) {
  FILE* f = fopen(lst, "r");
  if (!f) return 2;
  int files = 0, failures = 0, want;
  long long want_n;
  char path[4096];
  while (fscanf(f, "%d %lld %4095s", &want, &want_n, path) == 3) {
    c2d_ckpt_info o;
    char msg[512];
    const int rc = c2d_ckpt_info_file(path, &o, nullptr, msg, sizeof msg);
    files++;
    if (rc != want || (rc == 0 && o.n_records != want_n) || (rc != 0 && !msg[0])) {
      failures++;
      printf("FAIL %s: code %d (expected %d) %s\n", path, rc, want, msg);
    }
  }
  fclose(f);
  printf("%d files, %d failures\n", files, failures);
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && std::string(argv[1]) == "info") return info(argv[2]);
  if (argc == 3 && std::string(argv[1]) == "list") return list(argv[2]);
  if (argc >= 3 && std::string(argv[1]) == "digest") {
    std::vector<uint64_t> w;
    for (int i = 3; i < argc; i++) w.push_back(strtoull(argv[i], nullptr, 16));
    const c2d_ckpt_digest d = c2d_ckpt_digest_words(w.data(), (int64_t)w.size(), strtoull(argv[2], nullptr, 0));
    printf("%" PRIu64 " %" PRIu64 "\n", d.sum, d.x);
    return 0;
  }
  fprintf(stderr, "usage: ckpt_main info <file> | list <list file> | digest <g0> <hex word> ...\n");
  return 2;
}
