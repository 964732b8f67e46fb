// Development harness (tooling, never shipped): the host twin of both tiers of ygm_text_v1 (ygm_text.hpp: the
// sequential code of k_text_flat and k_text) over a file of asks, so the text can be checked against the yjs bundle
// without a GPU.  Input: u32 count, then per ask (u32 len, state bytes), (u32 len, root name bytes), u32 mode
// (0 flat, 1 deep).  Output per ask: i32 flat tier (0: not taken, 1: the 6 KiB launch, 2: the 24 KiB launch), u32
// len, bytes; then the general tier's i32 status, u32 len, bytes -- every ask goes through the general twin, and
// through the flat twin at both workspace sizes as the kernel's two launches would offer it.
//     textdev in.bin out.bin [flags]       (flags: 1 = 13.5 compat; the text does not depend on it)
#define YGM_HOST_BUILD 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../hocuspocus_amd/csrc/ygm_text.hpp"

static bool rd(FILE* f, std::vector<uint8_t>& v, uint32_t pad) {
  uint32_t len;
  if (fread(&len, 4, 1, f) != 1) return false;
  v.assign((size_t)len + pad, 0);
  if (len && fread(v.data(), 1, len, f) != len) return false;
  v.resize((size_t)len + pad);
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: textdev in.bin out.bin [flags]\n"); return 2; }
  const uint32_t flags = argc > 3 ? (uint32_t)atoi(argv[3]) : 0u;
  FILE* f = fopen(argv[1], "rb"); FILE* g = fopen(argv[2], "wb");
  if (!f || !g) return 1;
  uint32_t n = 0; if (fread(&n, 4, 1, f) != 1) return 1;
  std::vector<uint8_t> st, name, ws, tws;
  static const uint32_t LB[2] = {6144u, 24576u};
  for (uint32_t i = 0; i < n; i++) {
    uint32_t mode;
    if (!rd(f, st, 64) || !rd(f, name, 0) || fread(&mode, 4, 1, f) != 1) return 1;
    const uint32_t len = (uint32_t)st.size() - 64u, nl = (uint32_t)name.size();
    // the flat tier: the kernel's claim conditions, then lane 0's code and the sequential emit
    int32_t tier = 0; uint32_t fl = 0;
    std::vector<uint8_t> fo(len + 16u, 0);
    for (int a = 0; a < 2 && !tier && len && len < 0xFFFFu && nl < 0xFFFFu; a++) {
      tws.assign(LB[a] + 64u, 0xA5);
      ygm::snapt::TDoc D;
      if (!ygm::text::flat_init(D, st.data(), len, flags, tws.data(), LB[a])) continue;
      const int32_t cnt = ygm::text::flat_prepare(D, name.data(), nl);
      if (cnt < 0) continue;
      ygm::snap::OutCap o{fo.data(), 0, len};
      ygm::text::flat_emit_seq(D, (uint32_t)cnt, o);
      if (o.n > o.cap) { fprintf(stderr, "ask %u: flat text longer than its input\n", i); return 1; }
      tier = a + 1; fl = o.n;
    }
    fwrite(&tier, 4, 1, g); fwrite(&fl, 4, 1, g);
    if (fl) fwrite(fo.data(), 1, fl, g);
    // the general tier
    int32_t gs = 1; uint32_t oo = 0, ol = 0;   // (an empty update: ST_MALFORMED, as k_text)
    if (len) {
      uint32_t S, Dn, C; ygm::snap::count_doc(st.data(), len, flags, S, Dn, C);
      const ygm::snap::Caps k = ygm::snap::caps_of(S, Dn, C, len);
      ws.assign(ygm::snap::ws_bytes(k) + 64, 0);
      gs = ygm::text::text_doc(st.data(), len, flags, ws.data(), k, name.data(), nl, mode, oo, ol);
    }
    const uint32_t gl = gs == 0 ? ol : 0u;
    fwrite(&gs, 4, 1, g); fwrite(&gl, 4, 1, g);
    if (gl) fwrite(ws.data() + oo, 1, gl, g);
  }
  fclose(f); fclose(g);
  return 0;
}
