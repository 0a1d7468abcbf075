// Stand-alone driver of nk_poly_plant.h for tests/test_poly_plant_host.py: nothing of the GPU is included.  Standard input:
// one case after another,
//   "d p n_terms k4_at_k1 Ts n_lines"  then n_lines (<= 32) lines  "row ex0 ex1 ex2 ex3 eu0 eu1 eu2 eu3 coef"  then one line
//   "x0 x1 x2 x3 u0 u1 u2 u3"
// (floating-point numbers as strtod reads them: hexadecimal floats, "nan", "inf").  n_terms is the field of the description
// and may be out of range; n_lines is how many term lines follow.  Every case goes through the validation and, when the
// description is valid, through one step.  Output, one line per case:  "ok x_next ..." (d hexadecimal floats) or "bad <message>".
#include <cstdio>
#include <cstdlib>

#include "nk_poly_plant.h"

static bool read_double(double* v) {
  char tok[64];
  if (std::scanf("%63s", tok) != 1) return false;
  *v = std::strtod(tok, nullptr);
  return true;
}

int main() {
  int d = 0, p = 0, n_terms = 0, k4 = 0, n_lines = 0;
  while (std::scanf("%d %d %d %d", &d, &p, &n_terms, &k4) == 4) {
    nk_poly_plant pl = {};
    pl.d = d; pl.p = p; pl.n_terms = n_terms; pl.k4_at_k1 = k4;
    if (!read_double(&pl.Ts) || std::scanf("%d", &n_lines) != 1 || n_lines < 0 || n_lines > NK_POLY_MAX_TERMS) return 2;
    for (int i = 0; i < n_lines; ++i) {
      int row = 0, e[8];
      if (std::scanf("%d %d %d %d %d %d %d %d %d", &row, e, e + 1, e + 2, e + 3, e + 4, e + 5, e + 6, e + 7) != 9) return 2;
      nk_poly_term& t = pl.terms[i];
      t.row = row;
      for (int k = 0; k < 4; ++k) {
        t.ex[k] = (uint8_t)e[k];
        t.eu[k] = (uint8_t)e[4 + k];
      }
      if (!read_double(&t.coef)) return 2;
    }
    double xu[8];
    for (double& v : xu)
      if (!read_double(&v)) return 2;
    char msg[160];
    if (!nk::poly_plant_check(&pl, msg, sizeof msg)) {
      std::printf("bad %s\n", msg);
      continue;
    }
    double xn[NK_POLY_MAX_D];
    nk::poly_plant_step_host(pl, xu, xu + 4, xn);
    std::printf("ok");
    for (int k = 0; k < pl.d; ++k) std::printf(" %a", xn[k]);
    std::printf("\n");
  }
  return 0;
}
