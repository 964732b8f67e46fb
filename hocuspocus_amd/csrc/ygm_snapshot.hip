// ygm_snapshot.hip -- doc-normalized snapshot kernels:
//   k_snap_text  : flat-text documents (ygm_snap_text.hpp), one per wave, input + workspace in LDS, into slots;
//                  the documents it leaves take the general path below
//   k_snap_count : per document, the struct / delete-range / client-block counts -> workspace bytes
//   k_snap_scan* : exclusive scan of the workspace sizes (three launches, 256 documents per block)
//   k_snap       : per document, integrate + gc + merge + encode into its workspace's output region
//   k_pend_*     : documents left pending (ST_PEND): their [state, pendingDs, pending structs] packed as three-update
//                  documents for the merge kernels (plan, copy), then the merged bytes' places written back (fix);
//                  k_pend_split* / k_pend_join*: their three parts diffed and merged for SyncStep2
//   k_cont_count, k_cont : read-only SyncStep2 (snapshotContainsUpdate), a thread per document
// A thread per document keeps the reference's sequential algorithm (YATA integration order matters)
// while up to 64 documents share a wave; the workspace is per document, so nothing is shared.  The staging into LDS,
// the lane prologue and the epilogue of k_snap_count and k_snap are ygm_docstage.hpp's, shared with k_text and k_json.
// k_snap_text and k_snap take a nullable per-document option array (one byte each; bit 0, YGM_DOC_NO_GC: the document
// is a Y.Doc({gc: false}), snap::F_SNAP_NOGC for that document alone; any other bit: ST_INVAL for that document, the
// byte not used otherwise).  The count pass does not depend on it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "ygm_common.hpp"
#include "ygm_snapshot.hpp"
#include "ygm_snap_text.hpp"
#include "ygm_docstage.hpp"
#include "ygm_launch.hpp"

namespace ygm {

using docstage::Lane;

// k_snap_text: one document per workgroup (one wave): lane 0 runs the flat-text snapshot (ygm_snap_text.hpp) with
// its workspace in the workgroup's LB bytes of LDS and its input read through the scalar cache (aligned dwords from
// the constant address space: the kernel never writes the arena) -- the integration's dependent chain as LDS round
// trips instead of global ones, the document index wave-uniform so the control flow stays on scalar branches.
// Documents outside the envelope or the workspace are left unclaimed (a second launch with a larger LB, then the
// count / scan / k_snap path).  Outputs go to per-document slots at align16(2 * doc_off[d] + 64 * d), 2n + 48 bytes.
template <uint32_t LB>
__global__ __launch_bounds__(docstage::NT) void k_snap_text(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off, uint32_t n_docs,
                                                    uint32_t flags, uint8_t* __restrict__ out, uint64_t* __restrict__ out_off,
                                                    uint64_t* __restrict__ out_len, int32_t* __restrict__ status, uint8_t* __restrict__ claim,
                                                    unsigned long long* __restrict__ pay, uint32_t again, uint64_t slot_total,
                                                    const uint8_t* __restrict__ opt) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[LB];
  const uint32_t d = blockIdx.x;
  if (threadIdx.x != 0 || (again && claim[d])) return;   // (again: the first launch took it)
  const uint64_t a = doc_off[d], b = doc_off[d + 1];
  bool ok = false;
  // (a slot past the caller's region, slot_total = 2 * arena_bytes + 64 * n_docs: left to the general path, as is a
  // document with a bad option byte: k_snap gives it its status)
  if (snap::doc_flags(flags, opt, d, flags) && b > a && b - a < 0xFFFFu && snap::al16(2 * a + 64ull * d) + 2 * (b - a) + 48 <= slot_total) {
    const uint32_t n = (uint32_t)(b - a);
    const uint64_t slot = snap::al16(2 * a + 64ull * d);
    snap::OutCap o{out + slot, 0, 2u * n + 48u};
    ok = snapt::snapshot_text(arena + a, n, flags, lds, LB, o) && o.n <= o.cap;
    if (ok) {
      out_off[d] = slot; out_len[d] = o.n; status[d] = ST_OK;
      atomicAdd(pay, (unsigned long long)o.n);
      atomicAdd(pay + 1, 1ull);
    }
  }
  claim[d] = ok ? 1 : 0;
}

__global__ __launch_bounds__(docstage::NT) void k_snap_count(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off,
                                                     uint32_t n_docs, uint32_t flags, uint4* __restrict__ cnt,
                                                     uint64_t* __restrict__ need, const uint8_t* __restrict__ claim) {
  __shared__ __attribute__((aligned(16))) uint8_t stg[docstage::STAGE + 16];
  const Lane L = docstage::lane_doc(stg, arena, doc_off, n_docs, docstage::DPW);
  const uint32_t d = L.d;
  if (!L.on) return;
  if (claim && claim[d]) { cnt[d] = make_uint4(0, 0, 0, 0); need[d] = 0; return; }   // k_snap_text wrote it
  uint32_t S = 0, D = 0, C = 0;
  const uint32_t n = docstage::doc_len(doc_off[d], doc_off[d + 1]);
  if (n) snap::count_doc(L.in, n, flags, S, D, C);
  cnt[d] = make_uint4(S, D, C, n);
  need[d] = snap::al16(snap::ws_bytes(snap::caps_of(S, D, C, n)));
}

// exclusive scan of n u64 values in place, total at v[n]: block sums, one block scanning them, apply
__global__ __launch_bounds__(256) void k_snap_scan_sum(const uint64_t* __restrict__ v, uint32_t n, uint64_t* __restrict__ bs) {
  __shared__ uint64_t tmp[256 / WAVE + 1];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  uint64_t tot;
  (void)block_exscan<256>(i < n ? v[i] : (uint64_t)0, tmp, tot);
  if (threadIdx.x == 0) bs[blockIdx.x] = tot;
}
__global__ __launch_bounds__(1024) void k_snap_scan_top(uint64_t* __restrict__ bs, uint32_t nb) {
  __shared__ uint64_t tmp[1024 / WAVE + 1];
  __shared__ uint64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < nb; b0 += 1024) {
    const uint32_t i = b0 + threadIdx.x;
    uint64_t tot;
    const uint64_t pre = block_exscan<1024>(i < nb ? bs[i] : (uint64_t)0, tmp, tot);
    if (i < nb) bs[i] = carry + pre;
    __syncthreads();
    if (threadIdx.x == 0) carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) bs[nb] = carry;
}
__global__ __launch_bounds__(256) void k_snap_scan_apply(uint64_t* __restrict__ v, uint32_t n, const uint64_t* __restrict__ bs) {
  __shared__ uint64_t tmp[256 / WAVE + 1];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  uint64_t tot;
  const uint64_t pre = block_exscan<256>(i < n ? v[i] : (uint64_t)0, tmp, tot);
  if (i < n) v[i] = bs[blockIdx.x] + pre;
  if (i == n) v[n] = bs[gridDim.x];
}

__global__ __launch_bounds__(docstage::NT) void k_snap(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off, uint32_t n_docs,
                                               uint32_t flags, const uint4* __restrict__ cnt, const uint64_t* __restrict__ ws_off,
                                               uint8_t* __restrict__ ws, uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_len,
                                               int32_t* __restrict__ status, unsigned long long* __restrict__ payload, uint32_t dpw,
                                               const uint8_t* __restrict__ claim, uint64_t base, uint32_t* __restrict__ pend_list,
                                               unsigned int* __restrict__ pend_n, const uint8_t* __restrict__ opt) {
  __shared__ __attribute__((aligned(16))) uint8_t stg[docstage::STAGE + 16];
  const Lane L = docstage::lane_doc(stg, arena, doc_off, n_docs, dpw);
  const uint32_t d = L.d;
  uint64_t mine = 0;
  if (L.on && !(claim && claim[d])) {
    const uint4 c = cnt[d];
    const uint64_t a = doc_off[d], b = doc_off[d + 1];
    uint32_t oo = 0, ol = 0;
    uint32_t fl;
    snap::Caps k;
    int st = docstage::lane_caps(snap::doc_flags(flags, opt, d, fl), a, b, c, k);
    if (st == ST_OK) st = snap::snapshot_doc(L.in, c.w, fl, ws + base + ws_off[d], k, oo, ol);
    mine = docstage::put(d, out_off, out_len, status, base + ws_off[d] + oo, (st == ST_OK || st == snap::ST_PEND) ? ol : 0u, st);
    if (st == snap::ST_PEND) pend_list[atomicAdd(pend_n, 1u)] = d;   // (rare: one atomic per such document)
  }
  docstage::add_payload(mine, payload);
}

// ---- pending documents: [state, pendingDs, pending structs] (PendHdr) -> three-update documents for the merge kernels
// plan (one workgroup): document j of the list gets updates 3j .. 3j + 2 at the exclusive prefix of the three lengths
__global__ __launch_bounds__(1024) void k_pend_plan(const uint32_t* __restrict__ list, uint32_t P, const uint8_t* __restrict__ ws,
                                                    const uint64_t* __restrict__ out_off, uint64_t* __restrict__ upd_off,
                                                    uint32_t* __restrict__ doc_upd) {
  __shared__ uint64_t tmp[1024 / WAVE + 1];
  __shared__ uint64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t j0 = 0; j0 < P; j0 += 1024) {
    const uint32_t j = j0 + threadIdx.x;
    uint32_t l0 = 0, l1 = 0, l2 = 0;
    if (j < P) {
      const uint8_t* h = ws + out_off[list[j]];   // PendHdr, read by bytes (the region's base need not be aligned)
      auto u32at = [&](uint32_t o) { return (uint32_t)h[o] | ((uint32_t)h[o + 1] << 8) | ((uint32_t)h[o + 2] << 16) | ((uint32_t)h[o + 3] << 24); };
      l0 = u32at(0); l1 = u32at(4); l2 = u32at(8);
    }
    uint64_t tot;
    const uint64_t pre = carry + block_exscan<1024>(j < P ? (uint64_t)l0 + l1 + l2 : (uint64_t)0, tmp, tot);
    if (j < P) { upd_off[3ull * j] = pre; upd_off[3ull * j + 1] = pre + l0; upd_off[3ull * j + 2] = pre + l0 + l1; doc_upd[j] = 3u * j; }
    __syncthreads();
    if (threadIdx.x == 0) carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) { upd_off[3ull * P] = carry; doc_upd[P] = 3u * P; }
}
// copy (a workgroup per document): its three updates to their places in the packed arena
__global__ __launch_bounds__(256) void k_pend_copy(const uint32_t* __restrict__ list, const uint8_t* __restrict__ ws,
                                                   const uint64_t* __restrict__ out_off, const uint64_t* __restrict__ upd_off,
                                                   uint8_t* __restrict__ dst) {
  const uint32_t j = blockIdx.x;
  const uint8_t* src = ws + out_off[list[j]] + sizeof(snap::PendHdr);
  const uint64_t a = upd_off[3ull * j], n = upd_off[3ull * j + 3] - a;
  for (uint64_t i = threadIdx.x; i < n; i += 256) dst[a + i] = src[i];
}
// fix: the merged bytes were appended at `tail` of the output region: each document's place, length and status (pst:
// a status decided before the merge, which wins when non-zero)
__global__ __launch_bounds__(256) void k_pend_fix(const uint32_t* __restrict__ list, uint32_t P, const uint64_t* __restrict__ m_off,
                                                  const uint64_t* __restrict__ m_len, const int32_t* __restrict__ m_st,
                                                  const int32_t* __restrict__ pst, uint64_t tail, uint64_t* __restrict__ out_off,
                                                  uint64_t* __restrict__ out_len, int32_t* __restrict__ status) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= P) return;
  const uint32_t d = list[j];
  const int32_t st = pst && pst[j] ? pst[j] : m_st[j];
  out_off[d] = tail + m_off[j]; out_len[d] = st == ST_OK ? m_len[j] : 0u; status[d] = st;
}

// ---- SyncStep2 of pending documents: encodeStateAsUpdate(doc, sv) = mergeUpdates([writeStateAsUpdate(doc, sv),
// pendingDs, diffUpdate(pending structs, sv)]) (Y@23300).  split: each document's three parts and its state vector
// packed into four arenas (offsets k (P + 1) + j: k = state, pendingDs, pending structs, state vector), for the two
// diffs; join: [diff(state), pendingDs, diff(pending structs)] packed as three-update documents for the merge
YDEV uint32_t pend_len(const uint8_t* h, uint32_t k) {
  return (uint32_t)h[4 * k] | ((uint32_t)h[4 * k + 1] << 8) | ((uint32_t)h[4 * k + 2] << 16) | ((uint32_t)h[4 * k + 3] << 24);
}
__global__ __launch_bounds__(1024) void k_pend_split_plan(const uint32_t* __restrict__ list, uint32_t P, const uint8_t* __restrict__ ws,
                                                          const uint64_t* __restrict__ out_off, const uint64_t* __restrict__ sv_off,
                                                          uint64_t* __restrict__ offs) {
  __shared__ uint64_t tmp[1024 / WAVE + 1];
  __shared__ uint64_t carry[4];
  if (threadIdx.x < 4) carry[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t j0 = 0; j0 < P; j0 += 1024) {
    const uint32_t j = j0 + threadIdx.x;
    uint64_t l[4] = {0, 0, 0, 0};
    if (j < P) {
      const uint32_t d = list[j];
      const uint8_t* h = ws + out_off[d];
      l[0] = pend_len(h, 0); l[1] = pend_len(h, 1); l[2] = pend_len(h, 2); l[3] = sv_off[d + 1] - sv_off[d];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint64_t tot;
      const uint64_t pre = block_exscan<1024>(l[k], tmp, tot);
      if (j < P) offs[(uint64_t)k * (P + 1) + j] = carry[k] + pre;
      __syncthreads();
      if (threadIdx.x == 0) carry[k] += tot;
      __syncthreads();
    }
  }
  if (threadIdx.x < 4) offs[(uint64_t)threadIdx.x * (P + 1) + P] = carry[threadIdx.x];
}
__global__ __launch_bounds__(256) void k_pend_split_copy(const uint32_t* __restrict__ list, uint32_t P, const uint8_t* __restrict__ ws,
                                                         const uint64_t* __restrict__ out_off, const uint8_t* __restrict__ sv,
                                                         const uint64_t* __restrict__ sv_off, const uint64_t* __restrict__ offs,
                                                         uint8_t* __restrict__ da, uint8_t* __restrict__ db, uint8_t* __restrict__ dc,
                                                         uint8_t* __restrict__ dsv) {
  const uint32_t j = blockIdx.x, d = list[j];
  const uint8_t* src = ws + out_off[d] + sizeof(snap::PendHdr);
  uint8_t* const dst[3] = {da, db, dc};
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const uint64_t a = offs[(uint64_t)k * (P + 1) + j], n = offs[(uint64_t)k * (P + 1) + j + 1] - a;
    for (uint64_t i = threadIdx.x; i < n; i += 256) dst[k][a + i] = src[i];
    src += n;
  }
  const uint64_t a = offs[3ull * (P + 1) + j], n = offs[3ull * (P + 1) + j + 1] - a, s0 = sv_off[d];
  for (uint64_t i = threadIdx.x; i < n; i += 256) dsv[a + i] = sv[s0 + i];
}
// ---- the same split for asks that share states (ygm_sync_step2_shared_v1): `list` holds asks; ask a's parts come from
// the workspace record of its state ask_ix[a], its state vector from the ask.  The parts of a pending state are copied
// once per ask (such states are rare: lost updates); the state is not snapshotted again.
// the asks whose state the snapshot left pending (one atomic per such ask: rare; every use of the list is per entry)
__global__ __launch_bounds__(256) void k_ask_pending(const uint32_t* __restrict__ ask_ix, uint32_t n_asks, const int32_t* __restrict__ st_state,
                                                     uint32_t* __restrict__ list, unsigned int* __restrict__ n_out) {
  const uint32_t a = blockIdx.x * 256 + threadIdx.x;
  if (a >= n_asks) return;
  const uint32_t sd = ask_ix[a];
  if (sd != 0xFFFFFFFFu && st_state[sd] == snap::ST_PEND) list[atomicAdd(n_out, 1u)] = a;
}
__global__ __launch_bounds__(1024) void k_pend_split_plan_g(const uint32_t* __restrict__ list, uint32_t P, const uint32_t* __restrict__ ask_ix,
                                                            const uint8_t* __restrict__ ws, const uint64_t* __restrict__ out_off,
                                                            const uint64_t* __restrict__ sv_off, uint64_t* __restrict__ offs) {
  __shared__ uint64_t tmp[1024 / WAVE + 1];
  __shared__ uint64_t carry[4];
  if (threadIdx.x < 4) carry[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t j0 = 0; j0 < P; j0 += 1024) {
    const uint32_t j = j0 + threadIdx.x;
    uint64_t l[4] = {0, 0, 0, 0};
    if (j < P) {
      const uint32_t a = list[j];
      const uint8_t* h = ws + out_off[ask_ix[a]];
      l[0] = pend_len(h, 0); l[1] = pend_len(h, 1); l[2] = pend_len(h, 2); l[3] = sv_off[a + 1] > sv_off[a] ? sv_off[a + 1] - sv_off[a] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint64_t tot;
      const uint64_t pre = block_exscan<1024>(l[k], tmp, tot);
      if (j < P) offs[(uint64_t)k * (P + 1) + j] = carry[k] + pre;
      __syncthreads();
      if (threadIdx.x == 0) carry[k] += tot;
      __syncthreads();
    }
  }
  if (threadIdx.x < 4) offs[(uint64_t)threadIdx.x * (P + 1) + P] = carry[threadIdx.x];
}
__global__ __launch_bounds__(256) void k_pend_split_copy_g(const uint32_t* __restrict__ list, uint32_t P, const uint32_t* __restrict__ ask_ix,
                                                           const uint8_t* __restrict__ ws, const uint64_t* __restrict__ out_off,
                                                           const uint8_t* __restrict__ sv, const uint64_t* __restrict__ sv_off,
                                                           const uint64_t* __restrict__ offs, uint8_t* __restrict__ da,
                                                           uint8_t* __restrict__ db, uint8_t* __restrict__ dc, uint8_t* __restrict__ dsv) {
  const uint32_t j = blockIdx.x, a = list[j];
  const uint8_t* src = ws + out_off[ask_ix[a]] + sizeof(snap::PendHdr);
  uint8_t* const dst[3] = {da, db, dc};
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const uint64_t o = offs[(uint64_t)k * (P + 1) + j], n = offs[(uint64_t)k * (P + 1) + j + 1] - o;
    for (uint64_t i = threadIdx.x; i < n; i += 256) dst[k][o + i] = src[i];
    src += n;
  }
  const uint64_t o = offs[3ull * (P + 1) + j], n = offs[3ull * (P + 1) + j + 1] - o, s0 = sv_off[a];
  for (uint64_t i = threadIdx.x; i < n; i += 256) dsv[o + i] = sv[s0 + i];
}
__global__ __launch_bounds__(1024) void k_pend_join_plan(uint32_t P, const uint64_t* __restrict__ a_len, const int32_t* __restrict__ a_st,
                                                         const uint64_t* __restrict__ offs, const uint64_t* __restrict__ c_len,
                                                         const int32_t* __restrict__ c_st, uint64_t* __restrict__ upd_off,
                                                         uint32_t* __restrict__ doc_upd, int32_t* __restrict__ pst) {
  __shared__ uint64_t tmp[1024 / WAVE + 1];
  __shared__ uint64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t j0 = 0; j0 < P; j0 += 1024) {
    const uint32_t j = j0 + threadIdx.x;
    uint64_t l0 = 0, l1 = 0, l2 = 0;
    if (j < P) {
      l0 = a_st[j] == ST_OK ? a_len[j] : 0u;
      l1 = offs[(P + 1) + j + 1] - offs[(P + 1) + j];
      l2 = c_st[j] == ST_OK ? c_len[j] : 0u;
      pst[j] = a_st[j] != ST_OK ? a_st[j] : c_st[j];
    }
    uint64_t tot;
    const uint64_t pre = carry + block_exscan<1024>(l0 + l1 + l2, tmp, tot);
    if (j < P) { upd_off[3ull * j] = pre; upd_off[3ull * j + 1] = pre + l0; upd_off[3ull * j + 2] = pre + l0 + l1; doc_upd[j] = 3u * j; }
    __syncthreads();
    if (threadIdx.x == 0) carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) { upd_off[3ull * P] = carry; doc_upd[P] = 3u * P; }
}
__global__ __launch_bounds__(256) void k_pend_join_copy(uint32_t P, const uint8_t* __restrict__ ad, const uint64_t* __restrict__ a_off,
                                                        const uint8_t* __restrict__ bd, const uint64_t* __restrict__ offs,
                                                        const uint8_t* __restrict__ cd, const uint64_t* __restrict__ c_off,
                                                        const uint64_t* __restrict__ upd_off, uint8_t* __restrict__ dst) {
  const uint32_t j = blockIdx.x;
  const uint8_t* const src[3] = {ad + a_off[j], bd + offs[(P + 1) + j], cd + c_off[j]};
#pragma unroll
  for (uint32_t k = 0; k < 3; k++) {
    const uint64_t a = upd_off[3ull * j + k], n = upd_off[3ull * j + k + 1] - a;
    for (uint64_t i = threadIdx.x; i < n; i += 256) dst[a + i] = src[k][i];
  }
}

// ---------------------------------------------------------------------------------------------------
// Read-only SyncStep2 (MessageReceiver.ts:156-179): Y.snapshotContainsUpdate(Y.snapshot(doc), update),
// restated from yjs 13.6 (snapshotContainsUpdateV2 -- not in the 13.5.16 bundle): every struct of the
// update (Skips included, in order; the first one past the snapshot's state vector answers false) ends
// at or below the state vector, and merging the update's delete set into the snapshot's leaves it equal.
// The snapshot is given as the document's normalized state (ygm_snapshot_v1 output: its delete set is
// createDeleteSetFromStructStore's, sorted and merged), so the second test is: every update range
// [k, k + l) lies in one snapshot range [a, b) with a <= k and k + l <= b (sortAndMergeDeleteSet).
struct CtSv { uint32_t client, end; };
struct CtDs { uint32_t client, clock, end, pad; };
__global__ __launch_bounds__(docstage::NT) void k_cont_count(const uint8_t* __restrict__ st_arena, const uint64_t* __restrict__ st_off,
                                                     uint32_t n_docs, uint32_t flags, uint64_t* __restrict__ need) {
  const uint32_t d = blockIdx.x * docstage::NT + threadIdx.x;
  if (d >= n_docs) return;
  uint32_t S = 0, D = 0, C = 0;
  const uint32_t n = docstage::doc_len(st_off[d], st_off[d + 1]);
  if (n) snap::count_doc(st_arena + st_off[d], n, flags, S, D, C);
  need[d] = snap::al16((uint64_t)(C + 1) * sizeof(CtSv)) + snap::al16((uint64_t)(D + 1) * sizeof(CtDs));
}
// ws holds ws_bytes (k_cont_count's size for the document): a snapshot with more blocks or ranges than
// counted (count_doc zeroes its counts past 2^26 structs / ranges) is refused, never written past
YDEV_NI int contains_doc(const uint8_t* sp, uint32_t sn, const uint8_t* up, uint32_t un, uint32_t flags, uint8_t* ws, uint64_t ws_bytes,
                         uint32_t& res) {
  res = 0;
  // the snapshot: state vector (clients of the blocks) and delete set
  Cur c{sp, 0, sn, 0, 0};
  const uint64_t nb = c.vu();
  CtSv* sv = (CtSv*)ws;
  uint32_t nsv = 0;
  for (uint64_t b = 0; b < nb && !c.err; b++) {
    const uint64_t ns = c.vu(), cl = c.vu(); uint64_t ck = c.vu();
    for (uint64_t s = 0; s < ns && !c.err; s++) { SInfo si; read_struct_fast(c, si, flags); ck += si.len; }
    if (cl > 0xFFFFFFFFull || ck > 0xFFFFFFFFull) return snap::ST_UNSUP;
    if (snap::al16((uint64_t)(nsv + 2) * sizeof(CtSv)) + 16u > ws_bytes) return snap::ST_UNSUP;
    sv[nsv].client = (uint32_t)cl; sv[nsv].end = (uint32_t)ck; nsv++;
  }
  if (c.err) return c.err;
  CtDs* ds = (CtDs*)(ws + snap::al16((uint64_t)(nsv + 1) * sizeof(CtSv)));
  uint32_t nds = 0;
  const uint64_t ndc = c.vu();
  for (uint64_t q = 0; q < ndc && !c.err; q++) {
    const uint64_t cl = c.vu(), nr = c.vu();
    for (uint64_t r = 0; r < nr && !c.err; r++) {
      const uint64_t ck = c.vu(), ln = c.vu();
      if (cl > 0xFFFFFFFFull || ck + ln > 0xFFFFFFFFull) return snap::ST_UNSUP;
      if ((uint64_t)((uint8_t*)(ds + nds + 1) - ws) > ws_bytes) return snap::ST_UNSUP;
      ds[nds].client = (uint32_t)cl; ds[nds].clock = (uint32_t)ck; ds[nds].end = (uint32_t)(ck + ln); nds++;
    }
  }
  if (c.err) return c.err;
  // the update: structs in order, then its delete set
  Cur u{up, 0, un, 0, 0};
  const uint64_t ub = u.vu();
  for (uint64_t b = 0; b < ub && !u.err; b++) {
    const uint64_t ns = u.vu(), cl = u.vu(); uint64_t ck = u.vu();
    if (u.err) break;
    uint64_t have = 0;
    for (uint32_t i = 0; i < nsv; i++) if (sv[i].client == cl) have = sv[i].end;
    for (uint64_t s = 0; s < ns && !u.err; s++) {
      SInfo si; read_struct_fast(u, si, flags);
      if (u.err) break;
      ck += si.len;
      if (have < ck) return ST_OK;   // res = 0: a struct past the snapshot
    }
  }
  if (u.err) return u.err;
  const uint64_t udc = u.vu();
  for (uint64_t q = 0; q < udc && !u.err; q++) {
    const uint64_t cl = u.vu(), nr = u.vu();
    for (uint64_t r = 0; r < nr && !u.err; r++) {
      const uint64_t k = u.vu(), l = u.vu();
      if (u.err) break;
      bool cov = false;
      for (uint32_t i = 0; i < nds && !cov; i++) cov = ds[i].client == cl && ds[i].clock <= k && k + l <= ds[i].end;
      if (!cov) { res = 0; return ST_OK; }
    }
  }
  if (u.err) return u.err;
  res = 1;
  return ST_OK;
}
__global__ __launch_bounds__(docstage::NT) void k_cont(const uint8_t* __restrict__ st_arena, const uint64_t* __restrict__ st_off,
                                               const uint8_t* __restrict__ up_arena, const uint64_t* __restrict__ up_off, uint32_t n_docs,
                                               uint32_t flags, const uint64_t* __restrict__ ws_off, uint8_t* __restrict__ ws,
                                               uint8_t* __restrict__ out, uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_len,
                                               int32_t* __restrict__ status) {
  const uint32_t d = blockIdx.x * docstage::NT + threadIdx.x;
  if (d >= n_docs) return;
  const uint64_t a = st_off[d], b = st_off[d + 1], ua = up_off[d], ub = up_off[d + 1];
  uint32_t res = 0;
  int st;
  if (b < a || ub < ua || b - a >= (1ull << 30) || ub - ua >= (1ull << 30)) st = ST_INVAL;
  else st = contains_doc(st_arena + a, (uint32_t)(b - a), up_arena + ua, (uint32_t)(ub - ua), flags, ws + ws_off[d], ws_off[d + 1] - ws_off[d], res);
  out[d] = (uint8_t)res;
  out_off[d] = d; out_len[d] = st == ST_OK ? 1u : 0u; status[d] = st;
}

}  // namespace ygm

using namespace ygm;

// k_snap_text<LB> over every document of the batch (again: 0 / 1, the kernel's own argument)
template <uint32_t LB>
static void snap_text_launch(const ygm_docs* d, const ygm_results* r, uint8_t* claim, unsigned long long* pay, uint32_t again, hipStream_t s) {
  hipLaunchKernelGGL((k_snap_text<LB>), dim3(d->n_docs), dim3(docstage::NT), 0, s, d->arena, d->doc_off, d->n_docs, d->flags, r->out, r->out_off,
                     r->out_len, r->status, claim, pay, again, r->slot_total, d->opt);
}
// exclusive scan of v[0..n) in place, total at v[n] (bs: ceil((n + 1) / 256) + 1 scratch entries)
static void scan_launch(uint64_t* v, uint32_t n, uint64_t* bs, hipStream_t s) {
  const uint32_t nb = (n + 1 + 255) / 256;
  hipLaunchKernelGGL(k_snap_scan_sum, dim3(nb), dim3(256), 0, s, (const uint64_t*)v, n, bs);
  hipLaunchKernelGGL(k_snap_scan_top, dim3(1), dim3(1024), 0, s, bs, nb);
  hipLaunchKernelGGL(k_snap_scan_apply, dim3(nb), dim3(256), 0, s, v, n, (const uint64_t*)bs);
}

extern "C" {

// the flat tier.  again == 0: 6 KiB of LDS per document (207 parts); again == 1: 24 KiB (865 parts) for the documents the
// first launch left.  YGM_SNAP_TEXT="KiB" picks another measured size for the first launch (4, 5, 53: 5.25, 8).
int ygm_k_launch_snap_text(const ygm_docs* d, const ygm_results* r, uint8_t* claim, unsigned long long* pay, int again, hipStream_t s) {
  if (d->n_docs == 0) return 0;
  const char* env = again ? nullptr : getenv("YGM_SNAP_TEXT");
  if (again) snap_text_launch<24576>(d, r, claim, pay, 1u, s);
  else switch (env ? atoi(env) : 6) {
    case 4: snap_text_launch<4096>(d, r, claim, pay, 0u, s); break;
    case 5: snap_text_launch<5120>(d, r, claim, pay, 0u, s); break;
    case 8: snap_text_launch<8192>(d, r, claim, pay, 0u, s); break;
    case 53: snap_text_launch<5376>(d, r, claim, pay, 0u, s); break;
    default: snap_text_launch<6144>(d, r, claim, pay, 0u, s);
  }
  return ygm_launch_rc(__func__);
}
// phase 1: counts and the scanned workspace offsets (w->ws_off: n_docs + 1 entries, total at [n_docs];
// bs: ceil(n / 256) + 1 scratch entries)
int ygm_k_launch_snap_plan(const ygm_docs* d, const ygm_ws* w, uint64_t* bs, hipStream_t s) {
  if (d->n_docs == 0) return 0;
  const uint32_t g = (d->n_docs + docstage::DPW - 1) / docstage::DPW;
  hipLaunchKernelGGL(k_snap_count, dim3(g), dim3(docstage::NT), 0, s, d->arena, d->doc_off, d->n_docs, d->flags, (uint4*)w->cnt, w->ws_off, w->claim);
  scan_launch(w->ws_off, d->n_docs, bs, s);
  return ygm_launch_rc(__func__);
}
int ygm_k_launch_scan(uint64_t* v, uint32_t n, uint64_t* bs, hipStream_t s) {
  if (n == 0) return 0;
  scan_launch(v, n, bs, s);
  return ygm_launch_rc(__func__);
}
// phase 2: the snapshots (w->ws sized from ws_off[n_docs])
// dpw_hint: documents per wave when YGM_SNAP_DPW is not set (0: the default 16)
int ygm_k_launch_snap(const ygm_docs* d, const ygm_ws* w, const ygm_results* r, unsigned long long* payload, uint32_t* pend_list,
                      unsigned int* pend_n, uint32_t dpw_hint, hipStream_t s) {
  if (d->n_docs == 0) return 0;
  const uint32_t dpw = docstage::docs_per_wave(dpw_hint);
  const uint32_t g = (d->n_docs + dpw - 1) / dpw;
  hipLaunchKernelGGL(k_snap, dim3(g), dim3(docstage::NT), 0, s, d->arena, d->doc_off, d->n_docs, d->flags, (const uint4*)w->cnt,
                     (const uint64_t*)w->ws_off, w->ws, r->out_off, r->out_len, r->status, payload, dpw, w->claim, w->base, pend_list, pend_n, d->opt);
  return ygm_launch_rc(__func__);
}
int ygm_k_launch_pend_plan(const uint32_t* list, uint32_t P, const uint8_t* ws, const uint64_t* out_off, const ygm_pend_batch* b, hipStream_t s) {
  hipLaunchKernelGGL(k_pend_plan, dim3(1), dim3(1024), 0, s, list, P, ws, out_off, b->upd_off, b->doc_upd);
  return ygm_launch_rc(__func__);
}
int ygm_k_launch_pend_copy(const uint32_t* list, uint32_t P, const uint8_t* ws, const uint64_t* out_off, const ygm_pend_batch* b, hipStream_t s) {
  if (P == 0) return 0;
  hipLaunchKernelGGL(k_pend_copy, dim3(P), dim3(256), 0, s, list, ws, out_off, (const uint64_t*)b->upd_off, b->dst);
  return ygm_launch_rc(__func__);
}
int ygm_k_launch_pend_fix(const uint32_t* list, uint32_t P, const ygm_batch_out* m, const int32_t* pst, uint64_t tail,
                          const ygm_results* r, hipStream_t s) {
  if (P == 0) return 0;
  hipLaunchKernelGGL(k_pend_fix, dim3((P + 255) / 256), dim3(256), 0, s, list, P, m->off, m->len, m->status, pst, tail, r->out_off, r->out_len,
                     r->status);
  return ygm_launch_rc(__func__);
}
int ygm_k_launch_pend_split(const uint32_t* list, uint32_t P, const uint32_t* ask_ix, const uint8_t* ws, const uint64_t* out_off,
                            const ygm_side* sv, const ygm_pend_parts* p, int pass, hipStream_t s) {
  if (P == 0) return 0;
  const uint64_t* offs = p->offs;   // (as the copy kernels read it)
  if (!ask_ix) {
    if (pass == 0) hipLaunchKernelGGL(k_pend_split_plan, dim3(1), dim3(1024), 0, s, list, P, ws, out_off, sv->off, p->offs);
    else hipLaunchKernelGGL(k_pend_split_copy, dim3(P), dim3(256), 0, s, list, P, ws, out_off, sv->arena, sv->off, offs, p->da, p->db, p->dc, p->dsv);
  } else if (pass == 0) hipLaunchKernelGGL(k_pend_split_plan_g, dim3(1), dim3(1024), 0, s, list, P, ask_ix, ws, out_off, sv->off, p->offs);
  else hipLaunchKernelGGL(k_pend_split_copy_g, dim3(P), dim3(256), 0, s, list, P, ask_ix, ws, out_off, sv->arena, sv->off, offs, p->da, p->db, p->dc,
                          p->dsv);
  return ygm_launch_rc(__func__);
}
int ygm_k_launch_ask_pending(const uint32_t* ask_ix, uint32_t n_asks, const int32_t* st_state, uint32_t* list, unsigned int* n_out,
                             hipStream_t s) {
  if (n_asks == 0) return 0;
  hipLaunchKernelGGL(k_ask_pending, dim3((n_asks + 255) / 256), dim3(256), 0, s, ask_ix, n_asks, st_state, list, n_out);
  return ygm_launch_rc(__func__);
}
int ygm_k_launch_pend_join(uint32_t P, const ygm_batch_out* a, const ygm_batch_out* c, const ygm_pend_parts* p, const ygm_pend_batch* b,
                           int32_t* pst, int pass, hipStream_t s) {
  if (P == 0) return 0;
  const uint64_t* offs = p->offs;
  if (pass == 0) hipLaunchKernelGGL(k_pend_join_plan, dim3(1), dim3(1024), 0, s, P, a->len, a->status, offs, c->len, c->status, b->upd_off, b->doc_upd, pst);
  else hipLaunchKernelGGL(k_pend_join_copy, dim3(P), dim3(256), 0, s, P, a->data, a->off, (const uint8_t*)p->db, offs, c->data, c->off,
                          (const uint64_t*)b->upd_off, b->dst);
  return ygm_launch_rc(__func__);
}

// read-only SyncStep2 containment: workspace plan (the snapshot scan), then one thread per document
int ygm_k_launch_cont_plan(const ygm_docs* st, const ygm_ws* w, uint64_t* bs, hipStream_t s) {
  if (st->n_docs == 0) return 0;
  const uint32_t g = (st->n_docs + docstage::NT - 1) / docstage::NT;
  hipLaunchKernelGGL(k_cont_count, dim3(g), dim3(docstage::NT), 0, s, st->arena, st->doc_off, st->n_docs, st->flags, w->ws_off);
  scan_launch(w->ws_off, st->n_docs, bs, s);
  return ygm_launch_rc(__func__);
}
int ygm_k_launch_cont(const ygm_docs* st, const ygm_side* upd, const ygm_ws* w, const ygm_results* r, hipStream_t s) {
  if (st->n_docs == 0) return 0;
  const uint32_t g = (st->n_docs + docstage::NT - 1) / docstage::NT;
  hipLaunchKernelGGL(k_cont, dim3(g), dim3(docstage::NT), 0, s, st->arena, st->doc_off, upd->arena, upd->off, st->n_docs, st->flags,
                     (const uint64_t*)w->ws_off, w->ws, r->out, r->out_off, r->out_len, r->status);
  return ygm_launch_rc(__func__);
}

}  // extern "C"
