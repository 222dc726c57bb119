// The text the kernel of csrc/report.hip compiles (eogs2_amd/csrc/report_cc.h) on the host, with a main of its own.
// Reads cases from the file named by argv[1]: per line 24 hexadecimal words, the bits of Ai[9], bi[3], A1[9], b1[3];
// prints per case "OUT" and 12 hexadecimal words, the bits of Ai'[9] then bi'[3].
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "report_cc.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s CASES\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  int cases = 0;
  for (;;) {
    uint32_t w[24];
    int got = 0;
    for (; got < 24; got++)
      if (std::fscanf(f, "%x", &w[got]) != 1) break;
    if (got == 0) break;
    if (got != 24) {
      std::fprintf(stderr, "case %d: %d words\n", cases, got);
      std::fclose(f);
      return 2;
    }
    float Ai[9], bi[3], A1[9], b1[3], oA[9], ob[3];
    std::memcpy(Ai, w, sizeof Ai);
    std::memcpy(bi, w + 9, sizeof bi);
    std::memcpy(A1, w + 12, sizeof A1);
    std::memcpy(b1, w + 21, sizeof b1);
    report_recompose(Ai, bi, A1, b1, oA, ob);
    uint32_t o[12];
    std::memcpy(o, oA, sizeof oA);
    std::memcpy(o + 9, ob, sizeof ob);
    std::printf("OUT");
    for (int i = 0; i < 12; i++) std::printf(" %08x", o[i]);
    std::printf("\n");
    cases++;
  }
  std::fclose(f);
  std::printf("CASES %d\n", cases);
  return 0;
}
