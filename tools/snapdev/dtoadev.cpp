// Development harness (tooling, never shipped): ygm_dtoa.hpp on the host -- the arithmetic the kernels run -- so that
// Number::toString can be checked against V8's strings and against an independent shortest-round-trip reference
// without a GPU.  Reads raw 8-byte doubles (the machine's byte order) on stdin and prints one decimal string per line;
// a value that is not finite prints as JavaScript names it (the walkers never pass one on).
//     dtoadev < doubles.bin > strings.txt
//     dtoadev --f32 < floats.bin > strings.txt     (raw 4-byte floats, each widened as the float32 tag of an Any is)
// A sanitizer build of this program (g++ -fsanitize=address,undefined) over the same input is where the table index,
// the shifts and the 25-byte bound are checked: every string goes through a writer of exactly 25 bytes.
#define YGM_HOST_BUILD 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../hocuspocus_amd/csrc/ygm_dtoa.hpp"

struct Out25 {
  uint8_t* p; uint32_t n;
  void b(uint8_t c) { if (n >= 25u) { fprintf(stderr, "more than 25 bytes\n"); exit(1); } p[n++] = c; }
};

int main(int argc, char** argv) {
  const bool f32 = argc > 1 && !strcmp(argv[1], "--f32");
  const size_t w = f32 ? 4 : 8;
  uint8_t raw[8];
  while (fread(raw, 1, w, stdin) == w) {
    uint64_t bits;
    if (f32) { uint32_t u; memcpy(&u, raw, 4); bits = ygm::dtoa::widen_f32(u); } else memcpy(&bits, raw, 8);
    if (!ygm::dtoa::finite(bits)) { puts(bits << 12 ? "NaN" : bits >> 63 ? "-Infinity" : "Infinity"); continue; }
    std::vector<uint8_t> buf(25);   // (an allocation of exactly the bound: a 26th byte is a sanitizer's finding)
    Out25 o{buf.data(), 0};
    ygm::dtoa::write(o, bits);
    fwrite(buf.data(), 1, o.n, stdout); fputc('\n', stdout);
  }
  return 0;
}
