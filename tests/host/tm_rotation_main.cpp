// Stand-alone host check of csrc/tm_rotation.h: the header is __host__ __device__, so the very C++ the kernels compile runs here
// on the CPU.  tests/test_rotation_host.py builds this file (host side only), feeds it moments and holds the answers against an SVD.
//
//   tm_rotation_main IN OUT
// IN:  records of int64 n followed by 15 fp64 moments (sum p, sum q, sum p q^T row-major), native byte order.
// OUT: 12 fp64 per record, R row-major then t.
// Exit status 0 on success, 2 on a usage or file error, 3 on a truncated record.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "tm_rotation.h"

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  std::FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<double> out;
  for (;;) {
    int64_t n;
    double m[tm_rotation::NMOM], x[12];
    if (std::fread(&n, sizeof n, 1, in) != 1) break;
    if (std::fread(m, sizeof(double), tm_rotation::NMOM, in) != (size_t)tm_rotation::NMOM) {
      std::fclose(in);
      return 3;
    }
    tm_rotation::solve(m, (int)n, x);
    out.insert(out.end(), x, x + 12);
  }
  std::fclose(in);
  std::FILE *o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const bool ok = std::fwrite(out.data(), sizeof(double), out.size(), o) == out.size();
  return std::fclose(o) == 0 && ok ? 0 : 2;
}
