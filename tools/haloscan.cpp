// haloscan.cpp -- TEST TOOL ONLY (tests/test_halo_scan.py): a host compile of art_halo.h's halo_ratio,
// the one formula of the halo scan, so a CPU test can hold it to numpy without a GPU. The product
// never runs this.
//
//   haloscan ratio < cases > results      (raw float64, native byte order)
//
// ratio: records of 11 (u[3], base v0, base v_ns[3], target v0, target v_ns[3])   -> 1 (R)
// Exit status 2: unknown mode; 3: the input is no whole number of records.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../adiabatic_raytracer_amd/csrc/art_halo.h"

int main(int argc, char** argv) {
  if (argc != 2 || std::strcmp(argv[1], "ratio")) return 2;
  const size_t nin = 11;
  std::vector<double> in;
  double buf[4096];
  size_t got;
  while ((got = std::fread(buf, sizeof(double), 4096, stdin)) > 0) in.insert(in.end(), buf, buf + got);
  if (in.size() % nin != 0) return 3;
  const size_t n = in.size() / nin;
  std::vector<double> out(n);
  for (size_t i = 0; i < n; ++i) {
    const double* c = in.data() + i * nin;
    const art::HaloK base{c[3], {c[4], c[5], c[6]}, 0.0}, target{c[7], {c[8], c[9], c[10]}, 0.0};  // (vp plays no part)
    out[i] = art::halo_ratio(c, base, target);
  }
  if (!out.empty() && std::fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size()) return 1;
  return 0;
}
