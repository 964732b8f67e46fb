// chunks.cpp -- CPU check of the host API's chunk planners (hocuspocus_amd/csrc/ygm_chunks.hpp), stand-alone:
//   g++ -std=c++17 -fsanitize=address,undefined -o chunks tools/hostdev/chunks.cpp && ./chunks [rounds]
// A few thousand random offset tables per planner.  Every plan must partition the results in order (and the primary
// inputs it covers); the plain planner must take, chunk by chunk, what a linear scan takes -- the longest run of
// documents that fits the budget, at least one --; the shared planner must follow the rules its comment states.
// Prints one summary line and exits 0, or the first violation and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../hocuspocus_amd/csrc/ygm_chunks.hpp"

using ygm::ChunkRange;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // xorshift64*
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return rng_state * 0x2545f4914f6cdd1dull;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (!fails++) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } return; } } while (0)

// sizes with many zeros, small values and now and then one larger than any budget
static uint64_t some_size(uint64_t budget) {
  switch (below(8)) {
    case 0: return 0;
    case 1: return budget + 1 + below(budget + 5);
    case 2: return budget;
    default: return below(budget / 2 + 2);
  }
}

static size_t n_plain = 0, n_shared = 0, n_chunks = 0;

// documents as primary inputs (merge false), or updates with a document each (merge true; documents may have none)
static void check_plain(bool merge) {
  const uint64_t budget = 1 + below(200);
  const uint32_t n_docs = (uint32_t)below(below(4) ? 40 : 2);   // (often 0 or 1)
  std::vector<uint32_t> upd_doc;
  std::vector<uint64_t> off(1, 1000 + below(50));   // (the first offset need not be 0)
  uint32_t n_pri = n_docs;
  if (merge) {
    for (uint32_t d = 0; d < n_docs; d++)
      for (uint64_t k = below(4) ? below(5) : 0; k; k--) upd_doc.push_back(d);
    n_pri = (uint32_t)upd_doc.size();
  }
  for (uint32_t i = 0; i < n_pri; i++) off.push_back(off.back() + some_size(merge ? budget / 2 + 1 : budget));
  const std::vector<ChunkRange> ch = ygm::plan_doc_chunks(off.data(), n_docs, merge, upd_doc.empty() ? nullptr : upd_doc.data(), n_pri, budget);
  n_plain++; n_chunks += ch.size();
  CHECK(!ch.empty(), "no chunk");
  if (n_docs == 0) { CHECK(ch.size() == 1 && ch[0].r0 == 0 && ch[0].r1 == 0 && ch[0].p0 == 0 && ch[0].p1 == 0, "empty batch"); return; }
  // where each document's inputs end, by a walk
  std::vector<uint32_t> doc_end(n_docs);
  for (uint32_t d = 0, u = 0; d < n_docs; d++) {
    if (merge) { while (u < n_pri && upd_doc[u] == d) u++; doc_end[d] = u; } else doc_end[d] = d + 1;
  }
  uint32_t d = 0, p = 0;
  for (size_t i = 0; i < ch.size(); i++) {
    const ChunkRange& C = ch[i];
    CHECK(C.r0 == d && C.p0 == p, "chunk %zu starts at result %u input %u, expected %u %u", i, C.r0, C.p0, d, p);
    CHECK(d < n_docs, "chunk %zu after the last document", i);
    // the linear scan: the first document always, then every further one while the run still fits
    uint32_t x = d + 1;
    while (x < n_docs && off[doc_end[x]] - off[p] <= budget) x++;
    CHECK(C.r1 == x && C.p1 == doc_end[x - 1], "chunk %zu ends at result %u input %u, the scan at %u %u (budget %llu)", i, C.r1, C.p1, x,
          doc_end[x - 1], (unsigned long long)budget);
    d = C.r1; p = C.p1;
  }
  CHECK(d == n_docs && p == n_pri, "the chunks end at result %u input %u of %u %u", d, p, n_docs, n_pri);
}

static void check_shared() {
  const uint64_t budget = 1 + below(300);
  const uint32_t n_states = (uint32_t)below(below(4) ? 30 : 2);
  std::vector<uint64_t> off(1, below(50));
  std::vector<uint32_t> ask_state;
  for (uint32_t s = 0; s < n_states; s++) {
    off.push_back(off.back() + some_size(budget));
    for (uint64_t k = below(3) ? below(4) : below(2) ? 0 : below(40); k; k--) ask_state.push_back(s);   // (often none, now and then many)
  }
  const uint32_t n_asks = (uint32_t)ask_state.size();
  const std::vector<ChunkRange> ch = ygm::plan_shared_chunks(off.data(), n_states, ask_state.empty() ? nullptr : ask_state.data(), n_asks, budget);
  n_shared++; n_chunks += ch.size();
  CHECK(!ch.empty(), "no chunk");
  if (n_states == 0) { CHECK(ch.size() == 1 && ch[0].r1 == 0 && ch[0].p1 == 0 && ch[0].r0 == 0 && ch[0].p0 == 0, "empty batch"); return; }
  std::vector<uint32_t> first_ask(n_states + 1, n_asks);   // the asks of state s: [first_ask[s], first_ask[s + 1])
  for (uint32_t s = n_states, a = n_asks; s-- > 0;) { while (a && ask_state[a - 1] >= s) a--; first_ask[s] = a; }
  uint32_t a = 0, s = 0;   // the first ask / state not yet covered (a split state counts as covered with its last ask)
  for (size_t i = 0; i < ch.size(); i++) {
    const ChunkRange& C = ch[i];
    CHECK(C.p0 < C.p1 && C.p1 <= n_states && C.r0 <= C.r1 && C.r1 <= n_asks, "chunk %zu: ranges [%u, %u) [%u, %u)", i, C.r0, C.r1, C.p0, C.p1);
    CHECK(C.r0 == a, "chunk %zu starts at ask %u, expected %u", i, C.r0, a);
    const bool piece = C.p1 - C.p0 == 1 && (C.r0 != first_ask[C.p0] || C.r1 != first_ask[C.p1]);   // some, not all, of one state's asks
    CHECK(C.p0 == (piece && C.r0 != first_ask[C.p0] ? s - 1 : s), "chunk %zu starts at state %u, expected %u", i, C.p0, s);
    uint64_t v = 0;
    for (uint32_t x = C.p0; x < C.p1; x++) v += off[x + 1] - off[x];
    for (uint32_t x = C.r0; x < C.r1; x++) {
      CHECK(ask_state[x] >= C.p0 && ask_state[x] < C.p1, "chunk %zu: ask %u names state %u outside [%u, %u)", i, x, ask_state[x], C.p0, C.p1);
      v += off[ask_state[x] + 1] - off[ask_state[x]];
    }
    // over the budget only alone: one state with at most one ask, or one ask of a split state
    CHECK(v <= budget || (C.p1 - C.p0 == 1 && C.r1 - C.r0 <= 1), "chunk %zu: %llu virtual bytes over the budget %llu", i,
          (unsigned long long)v, (unsigned long long)budget);
    if (piece) {   // of a split state: its virtual bytes exceed the budget; as many asks as fit beside it, at least one
      const uint64_t L = off[C.p0 + 1] - off[C.p0], asks = first_ask[C.p0 + 1] - first_ask[C.p0];
      CHECK(L + asks * L > budget && asks > 1, "chunk %zu splits a state that fits", i);
      const uint64_t m = budget >= 2 * L ? (budget - L) / L : 1;
      const bool last = C.r1 == first_ask[C.p0 + 1];
      CHECK(C.r1 > C.r0 && (last ? C.r1 - C.r0 <= m : C.r1 - C.r0 == m), "chunk %zu: a piece of %u asks, %llu fit", i, C.r1 - C.r0,
            (unsigned long long)m);
    } else {   // whole states, each with all of its asks; closed only because the next state did not fit beside them
      CHECK(C.r0 == first_ask[C.p0] && C.r1 == first_ask[C.p1], "chunk %zu: asks [%u, %u) of states [%u, %u)", i, C.r0, C.r1, C.p0, C.p1);
      if (C.p1 < n_states) {
        const uint64_t L = off[C.p1 + 1] - off[C.p1], nv = L + (uint64_t)(first_ask[C.p1 + 1] - first_ask[C.p1]) * L;
        CHECK(v + nv > budget, "chunk %zu closed although state %u fits beside it", i, C.p1);
      }
    }
    a = C.r1;
    s = C.p1;
  }
  CHECK(a == n_asks && s == n_states, "the chunks end at ask %u state %u of %u %u", a, s, n_asks, n_states);
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 4000;
  for (int r = 0; r < rounds && !fails; r++) {
    check_plain(false);
    check_plain(true);
    check_shared();
  }
  if (fails) return 1;
  printf("chunks ok: %zu plain plans, %zu shared plans, %zu chunks\n", n_plain, n_shared, n_chunks);
  return 0;
}
