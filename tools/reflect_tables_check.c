/* Stand-alone run of the host code behind c2d_reflect_tables_host
 * (compton2d_amd/csrc/reflect_host.h c2d_reflect_build) for the sanitizers:
 *
 *   cc -std=gnu11 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
 *      -Icompton2d_amd/csrc tools/reflect_tables_check.c -lm -o /tmp/reflect_tables_check
 *   /tmp/reflect_tables_check
 *
 * The tables go to heap blocks of exactly their size, so an index past
 * [500][500] is an error; it also runs the calls with null pointers.  Prints
 * a few values and exits 0. */
#include <stdio.h>
#include <stdlib.h>

#include "reflect_host.h"

int main(void) {
  const size_t N = C2D_NREF;
  double* E = (double*)malloc(N * sizeof(double));
  double* P = (double*)malloc(N * N * sizeof(double));
  double* W = (double*)malloc(N * N * sizeof(double));
  if (!E || !P || !W) return 2;
  int rc = c2d_reflect_build(E, P, W);
  if (rc) { printf("P_ref column %d is not non-decreasing\n", rc - 1); return 1; }
  if (c2d_reflect_build(E, NULL, NULL) || c2d_reflect_build(NULL, P, NULL) || c2d_reflect_build(NULL, NULL, W))
    return 1;
  for (size_t ni = 0; ni < N; ni++) {
    if (P[ni * N + N - 1] != 1.0 || W[ni * N + ni] < 0.0 || W[ni * N + ni] > 1.0) {
      printf("bad column %zu\n", ni);
      return 1;
    }
  }
  printf("E_ref[0] %.17g E_ref[499] %.17g P_ref[499][250] %.17g W_abs[0][0] %.17g W_abs[499][250] %.17g\n",
         E[0], E[N - 1], P[(N - 1) * N + 250], W[0], W[(N - 1) * N + 250]);
  free(E); free(P); free(W);
  return 0;
}
