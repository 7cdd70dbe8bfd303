// Host program over csrc/k1_consts.h: the band constants and the admission test of the K1 filter, evaluated by the
// SAME code the device runs.  usage: k1_f16_consts_main <beta> <shift> <r2 float bits> [...more triples]
// one line per triple: C K2 K0 eps_u eps_w (hex floats) kexp use_mfma;   `shift <H>` prints norm_shift(H) instead.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "k1_consts.h"

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "shift")) {
    printf("%d\n", k1c::norm_shift(strtod(argv[2], nullptr)));
    return 0;
  }
  if (argc < 4 || (argc - 1) % 3) return 2;
  for (int k = 1; k + 2 < argc; k += 3) {
    const double beta = strtod(argv[k], nullptr);
    const int s = atoi(argv[k + 1]);
    const unsigned int r2 = (unsigned int)strtoul(argv[k + 2], nullptr, 10);
    const k1c::Consts c = k1c::consts(beta, s, r2);
    printf("%a %a %a %a %a %d %d\n", c.C, c.K2, c.K0, c.eps_u, c.eps_w, c.kexp, c.use_mfma);
  }
  return 0;
}
