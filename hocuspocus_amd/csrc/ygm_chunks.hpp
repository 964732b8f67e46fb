// ygm_chunks.hpp -- how the host API cuts a batch into chunks.  Plain C++ with no HIP dependency: the host runtime
// (ygm_engine.cpp) includes it, and tools/hostdev/chunks.cpp checks both planners on the CPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace ygm {

// One chunk: the results [r0, r1) and the primary inputs [p0, p1) they are computed from.  Results are documents, or
// the asks of a shared-state call; primary inputs are what the first arena holds -- the documents themselves (then
// p = r), a merge's updates, a shared call's states.
struct ChunkRange {
  uint32_t r0 = 0, r1 = 0, p0 = 0, p1 = 0;
};

// Chunks of whole documents: each the longest run of documents whose input bytes fit `budget`, and at least one
// document.  by_update false: off[n_docs + 1] are the documents' offsets, the documents are the primary inputs.
// by_update true (merge): off[n_upd + 1] are the updates' offsets and upd_doc[n_upd] each update's document,
// non-decreasing; a document may have no updates (upd_doc may be null when n_upd is 0).  Always at least one chunk (an
// empty one for an empty batch).
inline std::vector<ChunkRange> plan_doc_chunks(const uint64_t* off, uint32_t n_docs, bool by_update, const uint32_t* upd_doc, uint32_t n_upd,
                                               uint64_t budget) {
  std::vector<ChunkRange> ch;
  // the first primary input of document x: binary searches over the ascending upd_doc / offsets (a walk over every
  // update took milliseconds per call on batches of millions of updates)
  auto first_pri = [&](uint32_t x) { return by_update ? (uint32_t)(std::lower_bound(upd_doc, upd_doc + n_upd, x) - upd_doc) : x; };
  uint32_t d = 0, p = 0;
  while (d < n_docs) {
    ChunkRange C;
    C.r0 = d; C.p0 = p;
    const uint64_t base = off[p];
    auto fits = [&](uint32_t x) { return off[first_pri(x)] - base <= budget; };   // documents [d, x)
    uint32_t lo = d + 1, hi = n_docs;   // the last x in [d + 1, n_docs] that fits (at least one document)
    if (fits(n_docs)) lo = n_docs;
    else while (lo < hi) { const uint32_t mid = lo + (hi - lo + 1) / 2; if (fits(mid)) lo = mid; else hi = mid - 1; }
    d = lo; p = first_pri(d);
    C.r1 = d; C.p1 = p;
    ch.push_back(C);
  }
  if (ch.empty()) ch.push_back(ChunkRange{});
  return ch;
}

// Shared states: n_states states, n_asks asks (ask_state non-decreasing).  A chunk is a range of states [p0, p1) with
// its contiguous asks [r0, r1) (results and the second arena are indexed by ask); its budget counts virtual bytes, the
// states' bytes plus, over its asks, the ask's state length -- what bounds the slot region.  A state whose virtual
// bytes fit the budget, or that has at most one ask, is never split and joins the open chunk unless that would pass
// the budget.  A state whose asks alone exceed the budget is split: chunks of that one state, each staging (and,
// step2, snapshotting) it again, with as many asks as fit beside the state (at least one).  Always at least one chunk.
inline std::vector<ChunkRange> plan_shared_chunks(const uint64_t* off, uint32_t n_states, const uint32_t* ask_state, uint32_t n_asks,
                                                  uint64_t budget) {
  std::vector<ChunkRange> ch;
  uint32_t a = 0;   // the first ask not yet placed
  ChunkRange C;
  uint64_t cur = 0;
  bool open = false;
  auto close = [&]() { if (open) { ch.push_back(C); open = false; cur = 0; } };
  for (uint32_t sd = 0; sd < n_states; sd++) {
    const uint64_t L = off[sd + 1] - off[sd];
    uint32_t a1 = a;
    while (a1 < n_asks && ask_state[a1] == sd) a1++;
    const uint64_t v = L + (uint64_t)(a1 - a) * L;
    if (open && cur + v > budget) close();
    if (v <= budget || a1 - a <= 1) {
      if (!open) { C = ChunkRange{}; C.p0 = sd; C.r0 = a; open = true; }
      C.p1 = sd + 1; C.r1 = a1; cur += v;
    } else {   // one state over several chunks
      const uint64_t per = budget > L ? (budget - L) / L : 1;
      const uint32_t m = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(per, 1), a1 - a);
      for (uint32_t x = a; x < a1; x += m) {
        C = ChunkRange{}; C.p0 = sd; C.p1 = sd + 1; C.r0 = x; C.r1 = std::min(a1, x + m);
        ch.push_back(C);
      }
    }
    a = a1;
  }
  close();
  if (ch.empty()) ch.push_back(ChunkRange{});
  return ch;
}

}  // namespace ygm
