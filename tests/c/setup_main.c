/* csrc/setup_host.h as plain C99 with its own main (host sanitizers): prints
 * the bits of a small F_IC and of one zone's electrons in both flavours, which
 * tests/test_setup_host.py holds against the library's build of the same header.
 *   setup_main tea amxwl gmin gmax p_nth */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../compton2d_amd/csrc/setup_host.h"

static void put(double v) {
  uint64_t u;
  memcpy(&u, &v, sizeof u);
  printf("%016" PRIx64 "\n", u);
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  double gnt[C2D_SU_NUM_NT], E_field[C2D_SU_NGRID], E_ph[C2D_SU_NGRID];
  c2d_su_grids(gnt, E_field, E_ph);
  const int rows[3] = {0, 120, 199};
  double g3[3], e8[8], F[24];
  for (int i = 0; i < 3; i++) g3[i] = gnt[rows[i]];
  for (int p = 0; p < 8; p++) e8[p] = E_field[150 + 30 * p];
  for (int libm = 1; libm >= 0; libm--) {
    if (c2d_su_ic_loss(g3, 3, e8, 8, F, 8, 1, libm)) return 3;
    for (int k = 0; k < 24; k++) put(F[k]);
    double gmin, N_nth, gbar, f[C2D_SU_NUM_NT], P[C2D_SU_NUM_NT];
    if (c2d_su_electrons_zone(atof(argv[1]), atof(argv[2]), atof(argv[3]), atof(argv[4]), atof(argv[5]), gnt,
                              libm, &gmin, &N_nth, &gbar, f, P))
      return 4;
    put(gmin);
    put(N_nth);
    put(gbar);
    for (int i = 0; i < C2D_SU_NUM_NT; i++) put(f[i]);
    for (int i = 0; i < C2D_SU_NUM_NT; i++) put(P[i]);
  }
  return 0;
}
