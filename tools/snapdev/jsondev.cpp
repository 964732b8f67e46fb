// Development harness (tooling, never shipped): the host twin of ygm_json_v1 (ygm_json.hpp: the sequential code of
// k_json) over a file of asks, so the JSON can be checked against the yjs bundle without a GPU.  Input: u32 count,
// then per ask (u32 len, state bytes), (u32 len, root name bytes).  Output per ask: i32 status, u32 reran, u32 len,
// bytes.  The overflow protocol is the engine's: a first run into an output region of Caps::out bytes (an allocation
// of its own, of exactly that size: a store one byte past the cap is a sanitizer's finding, not a write into slack);
// a document whose JSON does not fit (ST_JSON_MORE) runs again over a fresh workspace into a region of exactly the
// recorded length (reran = 1), and must then give that length.
//     jsondev [--floats] in.bin out.bin [flags]       (flags: 1 = 13.5 compat; the JSON does not depend on it.
//                                          --floats: the walk as a context opened with YGM_F_FLOATS runs it)
// A sanitizer build of this program (g++ -fsanitize=address,undefined) over the whole fixture is where the walk's
// bounds are checked.
#define YGM_HOST_BUILD 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>
#include "../../hocuspocus_amd/csrc/ygm_json.hpp"

static bool rd(FILE* f, std::vector<uint8_t>& v, uint32_t pad) {
  uint32_t len;
  if (fread(&len, 4, 1, f) != 1) return false;
  v.assign((size_t)len + pad, 0);
  if (len && fread(v.data(), 1, len, f) != len) return false;
  return true;
}

int main(int argc, char** argv) {
  bool floats = false;   // --floats, anywhere: the FLOATS instantiation (a context opened with YGM_F_FLOATS)
  for (int i = 1; i < argc; i++)
    if (!strcmp(argv[i], "--floats")) { floats = true; for (int j = i; j + 1 < argc; j++) argv[j] = argv[j + 1]; argc--; i--; }
  if (argc < 3) { fprintf(stderr, "usage: jsondev in.bin out.bin [flags]\n"); return 2; }
  const uint32_t flags = argc > 3 ? (uint32_t)atoi(argv[3]) : 0u;
  FILE* f = fopen(argv[1], "rb"); FILE* g = fopen(argv[2], "wb");
  if (!f || !g) return 1;
  uint32_t n = 0; if (fread(&n, 4, 1, f) != 1) return 1;
  std::vector<uint8_t> st, name;
  for (uint32_t i = 0; i < n; i++) {
    if (!rd(f, st, 64) || !rd(f, name, 0)) return 1;
    const uint32_t len = (uint32_t)st.size() - 64u, nl = (uint32_t)name.size();
    int32_t gs = 1; uint32_t ol = 0, reran = 0;   // (an empty update: ST_MALFORMED, as k_json)
    std::vector<uint8_t> res;
    if (len) {
      uint32_t S, Dn, C; ygm::snap::count_doc(st.data(), len, flags, S, Dn, C);
      const ygm::snap::Caps k = ygm::snap::caps_of(S, Dn, C, len);
      // (fresh allocations per ask, each of its exact size: no capacity left over from a larger document)
      std::vector<uint8_t> ws((size_t)ygm::snap::ws_core_bytes(k), 0), first((size_t)k.out, 0), big;
      gs = (floats ? ygm::json::json_run<false, true> : ygm::json::json_run<false, false>)(st.data(), len, flags, ws.data(), k, name.data(), nl, 0u, first.data(), k.out, ol);
      if (gs == 0) res.assign(first.begin(), first.begin() + ol);
      if (gs == ygm::json::ST_JSON_MORE) {
        const uint32_t need = ol;
        reran = 1;
        big.assign((size_t)need, 0);   // (exactly the recorded length: a sanitizer sees one byte more)
        std::fill(ws.begin(), ws.end(), 0);
        gs = (floats ? ygm::json::json_run<false, true> : ygm::json::json_run<false, false>)(st.data(), len, flags, ws.data(), k, name.data(), nl, 0u, big.data(), need, ol);
        if (gs != 0 || ol != need) { fprintf(stderr, "ask %u: the rerun gave status %d, %u bytes for %u recorded\n", i, gs, ol, need); return 1; }
        res = big;
      }
    }
    const uint32_t gl = gs == 0 ? ol : 0u;
    fwrite(&gs, 4, 1, g); fwrite(&reran, 4, 1, g); fwrite(&gl, 4, 1, g);
    if (gl) fwrite(res.data(), 1, gl, g);
  }
  fclose(f); fclose(g);
  return 0;
}
