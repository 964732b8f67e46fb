// Development harness (tooling, never shipped): version history on the host -- the device code of ygm_version.hpp
// (the cut) and ygm_snapshot.hpp (take, and the snapshots before and after the cut) over a file of (state, version)
// rows, the steps of ygm_version_take_v1 / ygm_version_restore_v1 in order.
// Input: u32 rows, then per row (u32 len, state) (u32 len, version).  Output per row four results (i32 status, u32 len,
// bytes): take, the cut update, restored into a gc document, restored into a gc: false document.  A restored document
// left pending (status 64) writes its PendHdr and three updates, as tools/snapdev/snapdev.cpp does.
// flags: 1 = yjs 13.5 compat.
#define YGM_HOST_BUILD 1
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../hocuspocus_amd/csrc/ygm_snapshot.hpp"
#include "../../hocuspocus_amd/csrc/ygm_version.hpp"

using namespace ygm;

static int snap_run(const std::vector<uint8_t>& in, uint32_t len, uint32_t flags, std::vector<uint8_t>& out) {
  out.clear();
  if (!len) return ST_MALFORMED;
  std::vector<uint8_t> u(in.begin(), in.begin() + len);
  u.resize(len + 64, 0);
  uint32_t S, D, C; snap::count_doc(u.data(), len, flags, S, D, C);
  const snap::Caps k = snap::caps_of(S, D, C, len);
  std::vector<uint8_t> ws(snap::ws_bytes(k) + 64, 0);
  uint32_t oo = 0, ol = 0;
  const int st = snap::snapshot_doc(u.data(), len, flags, ws.data(), k, oo, ol);
  if (st == 0 || st == snap::ST_PEND) out.assign(ws.begin() + oo, ws.begin() + oo + ol);
  return st;
}
static void put(FILE* g, int st, const std::vector<uint8_t>& b) {
  const int32_t s32 = st; const uint32_t l32 = (st == 0 || st == snap::ST_PEND) ? (uint32_t)b.size() : 0u;
  fwrite(&s32, 4, 1, g); fwrite(&l32, 4, 1, g);
  if (l32) fwrite(b.data(), 1, l32, g);
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: versiondev in.bin out.bin [flags]\n"); return 2; }
  const uint32_t flags = argc > 3 ? (uint32_t)atoi(argv[3]) : 0u;
  FILE* f = fopen(argv[1], "rb"); FILE* g = fopen(argv[2], "wb");
  if (!f || !g) return 1;
  uint32_t n = 0; if (fread(&n, 4, 1, f) != 1) return 1;
  std::vector<ver::SvEnt> tbl(ver::MAX_SV);
  for (uint32_t i = 0; i < n; i++) {
    std::vector<uint8_t> part[2];
    for (auto& p : part) {
      uint32_t len; if (fread(&len, 4, 1, f) != 1) return 1;
      p.assign(len, 0);
      if (len && fread(p.data(), 1, len, f) != len) return 1;
    }
    const std::vector<uint8_t>&state = part[0], &version = part[1];
    std::vector<uint8_t> take, S, X, r0, r1;
    put(g, snap_run(state, (uint32_t)state.size(), flags | snap::F_SNAP_STATE | snap::F_SNAP_VERSION, take), take);
    int st = snap_run(state, (uint32_t)state.size(), flags | snap::F_SNAP_STATE | snap::F_SNAP_NOGC, S);
    if (!st) {
      std::vector<uint8_t> v(version); v.resize(version.size() + 64, 0);
      const uint32_t sn = (uint32_t)S.size(), cap = sn + (uint32_t)version.size() + 16u;
      S.resize(sn + 64, 0);
      X.assign(cap, 0);
      uint32_t xl = 0;
      st = ver::cut_doc(ver::HostW{}, S.data(), sn, v.data(), (uint32_t)version.size(), flags, tbl.data(), X.data(), cap, xl);
      X.resize(st ? 0 : xl);
    }
    put(g, st, X);
    if (st) { put(g, st, r0); put(g, st, r1); continue; }
    const int s0 = snap_run(X, (uint32_t)X.size(), flags, r0); put(g, s0, r0);
    const int s1 = snap_run(X, (uint32_t)X.size(), flags | snap::F_SNAP_NOGC, r1); put(g, s1, r1);
  }
  fclose(f); fclose(g);
  return 0;
}
