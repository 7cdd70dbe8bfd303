// Host program over csrc/k1_consts.h: the band constants and the admission test of the K1 filter's X / Y formulation
// (k1c::consts_xy), evaluated by the SAME code the device runs.
// usage: k1_xy_consts_main <beta> <shift> <r2 float bits> [...more triples]
// one line per triple: C K2 K0 eps_y eps_x (hex floats) kexp use_mfma ra rb pa pb (k1c::xy_shifts of kexp)
#include <cstdio>
#include <cstdlib>

#include "k1_consts.h"

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3) return 2;
  for (int k = 1; k + 2 < argc; k += 3) {
    const double beta = strtod(argv[k], nullptr);
    const int s = atoi(argv[k + 1]);
    const unsigned int r2 = (unsigned int)strtoul(argv[k + 2], nullptr, 10);
    const k1c::ConstsXY c = k1c::consts_xy(beta, s, r2);
    int ra, rb, pa, pb;
    k1c::xy_shifts(c.kexp, &ra, &rb, &pa, &pb);
    printf("%a %a %a %a %a %d %d %d %d %d %d\n", c.C, c.K2, c.K0, c.eps_y, c.eps_x, c.kexp, c.use_mfma, ra, rb, pa, pb);
  }
  return 0;
}
