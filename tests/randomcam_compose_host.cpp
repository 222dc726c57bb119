// The text the kernel of csrc/randomcam.hip compiles (eogs2_amd/csrc/randomcam_compose.h) on the host, with a main of its own.
// Reads cases from the file named by argv[1]: per line 18 hexadecimal words, the bits of cam2virt[9] then camera_to_sun[9];
// prints per case "OUT" and 18 hexadecimal words, the bits of virt_to_sun[9] then K[9].
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "randomcam_compose.h"

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
    uint32_t w[18];
    int got = 0;
    for (; got < 18; got++)
      if (std::fscanf(f, "%x", &w[got]) != 1) break;
    if (got == 0) break;
    if (got != 18) {
      std::fprintf(stderr, "case %d: %d words\n", cases, got);
      std::fclose(f);
      return 2;
    }
    float c[9], s[9], out[18];
    std::memcpy(c, w, sizeof c);
    std::memcpy(s, w + 9, sizeof s);
    randomcam_compose(c, s, out);
    uint32_t o[18];
    std::memcpy(o, out, sizeof o);
    std::printf("OUT");
    for (int i = 0; i < 18; i++) std::printf(" %08x", o[i]);
    std::printf("\n");
    cases++;
  }
  std::fclose(f);
  std::printf("CASES %d\n", cases);
  return 0;
}
