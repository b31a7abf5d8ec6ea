/* Test harness (tests/test_plcm_host.py): the product's plcm dialogue and
 * file code (compton2d_amd/csrc/plcm_host.h, used by c2d_obs_set_add_plcm /
 * c2d_obs_set_write) exported for a CPU check against compton2d_amd/
 * observer.py and the reference plcm's own output files. */
#include "../../compton2d_amd/csrc/plcm_host.h"

int lw_sizeof(void) { return (int)sizeof(c2d_plcm_deck); }
int lw_parse(const char* text, c2d_plcm_deck* d) { return c2d_plcm_parse(text, d); }
int lw_write(const char* dir, const c2d_plcm_deck* d, const double* F, const double* F2, const double* cnt,
             int factor) {
  return c2d_plcm_write(dir, d, F, F2, cnt, factor);
}
