// halocheck.cpp -- TEST TOOL ONLY (tests/test_halo_host.py): a host compile of art_halo.h, the halo
// velocity model's three formulas, so a CPU test can hold them to numpy without a GPU. The product
// never runs this.
//
//   halocheck speed|asymptote|factor < cases > results      (raw float64, native byte order)
//
// speed:     records of 2 (U, vp)                          -> 1 (s)
// asymptote: records of 8 (x[3], d[3], s, GM)              -> 3 (u[3])
// factor:    records of 9 (u[3], s, v0, v_ns[3], vp)       -> 1 (F)
// Exit status 2: unknown mode; 3: the input is no whole number of records.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../adiabatic_raytracer_amd/csrc/art_halo.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  int nin = 0, nout = 0, mode = -1;
  if (!std::strcmp(argv[1], "speed")) { mode = 0; nin = 2; nout = 1; }
  if (!std::strcmp(argv[1], "asymptote")) { mode = 1; nin = 8; nout = 3; }
  if (!std::strcmp(argv[1], "factor")) { mode = 2; nin = 9; nout = 1; }
  if (mode < 0) return 2;
  std::vector<double> in;
  double buf[4096];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
  if (in.size() % (size_t)nin != 0) return 3;
  const size_t n = in.size() / (size_t)nin;
  std::vector<double> out(n * (size_t)nout);
  for (size_t i = 0; i < n; ++i) {
    const double* c = in.data() + i * (size_t)nin;
    double* o = out.data() + i * (size_t)nout;
    if (mode == 0) o[0] = art::halo_speed(c[0], c[1]);
    if (mode == 1) art::halo_asymptote(c, c + 3, c[6], c[7], o);
    if (mode == 2) o[0] = art::halo_factor(c, c[3], c[4], c + 5, c[8]);
  }
  if (!out.empty() && std::fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size()) return 1;
  return 0;
}
