// ygm_text.hip -- plain text of stored documents (ygm_text_v1; ygm_text.hpp for the semantics):
//   k_text_flat : flat-text documents asked by their single root name, one per wave: lane 0 integrates in LDS
//                 (snapt::TDoc, as k_snap_text), the wave copies the live slices out; what it leaves unclaimed takes
//   k_text      : the general path: documents staged in LDS, dpw per wave (staging, lane prologue and epilogue:
//                 ygm_docstage.hpp), workspaces from the snapshot's count and scan launches (ygm_k_launch_snap_plan),
//                 the text in the workspace's output region
// Outputs of the flat tier go to per-document slots at align16(2 * doc_off[d] + 64 * d), as k_snap_text's (the text
// is never longer than the input: disjoint slices of it).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "ygm_common.hpp"
#include "ygm_text.hpp"
#include "ygm_docstage.hpp"
#include "ygm_launch.hpp"

namespace ygm {

using docstage::Lane;
constexpr uint32_t TX_SHORT = 16;     // a part up to this long is copied by its own lane

// k_text_flat: one document per workgroup (one wave).  Lane 0 runs TDoc::parse / integrate_all / apply_ds over the
// workgroup's LB bytes of LDS exactly as k_snap_text does (same layout, same envelope), checks the asked name and
// linearises the list into sq[]; then the 64 lanes take the list parts in strides: a wave exclusive scan of the live
// lengths places each part, short parts are copied by their own lanes (neighbouring lanes write neighbouring bytes),
// longer ones by the whole wave with contiguous byte stores.  Both modes share the tier: the envelope has no nested
// types.  A document outside the envelope, asked by another name, or whose slot lies past the region is left
// unclaimed for k_text.
template <uint32_t LB>
__global__ __launch_bounds__(docstage::NT) void k_text_flat(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off,
                                                    const uint8_t* __restrict__ names, const uint64_t* __restrict__ name_off, uint32_t n_docs,
                                                    uint32_t flags, uint8_t* __restrict__ out, uint64_t* __restrict__ out_off,
                                                    uint64_t* __restrict__ out_len, int32_t* __restrict__ status, uint8_t* __restrict__ claim,
                                                    unsigned long long* __restrict__ pay, uint32_t again, uint64_t slot_total) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[LB];
  const uint32_t d = blockIdx.x;
  if (again && claim[d]) return;   // (again: the first launch took it; wave-uniform)
  const uint64_t a = doc_off[d], b = doc_off[d + 1];
  const uint64_t slot = snap::al16(2 * a + 64ull * d);
  int32_t cnt = -1;
  if (threadIdx.x == 0) {
    const uint64_t na = name_off[d], nb = name_off[d + 1];
    if (b > a && b - a < 0xFFFFu && slot + 2 * (b - a) + 48 <= slot_total && nb >= na && nb - na < 0xFFFFu) {
      snapt::TDoc D;
      if (text::flat_init(D, arena + a, (uint32_t)(b - a), flags, lds, LB)) cnt = text::flat_prepare(D, names + na, (uint32_t)(nb - na));
    }
  }
  __syncthreads();   // (lane 0's parts and sq[] in LDS, for the wave)
  cnt = __shfl(cnt, 0, WAVE);
  if (cnt < 0) {
    if (threadIdx.x == 0) claim[d] = 0;
    return;
  }
  const snapt::P* p = text::flat_parts(lds);
  const uint16_t* sq = text::flat_seq(lds, LB);
  const uint8_t* src = arena + a;
  uint8_t* dst = out + slot;
  const uint32_t lane = threadIdx.x;
  uint32_t base = 0;
  for (uint32_t i0 = 0; i0 < (uint32_t)cnt; i0 += WAVE) {
    const uint32_t i = i0 + lane;
    uint32_t len = 0, coff = 0;
    if (i < (uint32_t)cnt) {
      const snapt::P& u = p[sq[i]];
      if (text::flat_live(u.fl)) { len = u.len; coff = u.coff; }
    }
    const uint32_t inc = wave_incl_scan_add(len);
    const uint32_t o = base + inc - len;
    if (len <= TX_SHORT) for (uint32_t k = 0; k < len; k++) dst[o + k] = src[coff + k];
    unsigned long long m = __ballot(len > TX_SHORT);
    while (m) {
      const int j = __ffsll((long long)m) - 1;
      m &= m - 1;
      const uint32_t L = __shfl(len, j, WAVE), C = __shfl(coff, j, WAVE), O = __shfl(o, j, WAVE);
      for (uint32_t k = lane; k < L; k += WAVE) dst[O + k] = src[C + k];
    }
    base += __shfl(inc, WAVE - 1, WAVE);
  }
  if (lane == 0) {
    out_off[d] = slot; out_len[d] = base; status[d] = ST_OK;
    claim[d] = 1;
    atomicAdd(pay, (unsigned long long)base);
    atomicAdd(pay + 1, 1ull);
  }
}

__global__ __launch_bounds__(docstage::NT) void k_text(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off,
                                               const uint8_t* __restrict__ names, const uint64_t* __restrict__ name_off, uint32_t n_docs,
                                               uint32_t flags, uint32_t mode, const uint4* __restrict__ cnt, const uint64_t* __restrict__ ws_off,
                                               uint8_t* __restrict__ ws, uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_len,
                                               int32_t* __restrict__ status, unsigned long long* __restrict__ payload, uint32_t dpw,
                                               const uint8_t* __restrict__ claim, uint64_t base) {
  __shared__ __attribute__((aligned(16))) uint8_t stg[docstage::STAGE + 16];
  const Lane L = docstage::lane_doc(stg, arena, doc_off, n_docs, dpw);
  const uint32_t d = L.d;
  uint64_t mine = 0;
  if (L.on && !(claim && claim[d])) {
    const uint4 c = cnt[d];
    const uint64_t a = doc_off[d], b = doc_off[d + 1], na = name_off[d], nb = name_off[d + 1];
    uint32_t oo = 0, ol = 0;
    snap::Caps k;
    int st = docstage::lane_caps(nb >= na && nb - na < (1ull << 30), a, b, c, k);
    if (st == ST_OK) st = text::text_doc(L.in, c.w, flags, ws + base + ws_off[d], k, names + na, (uint32_t)(nb - na), mode, oo, ol);
    mine = docstage::put(d, out_off, out_len, status, base + ws_off[d] + oo, st == ST_OK ? ol : 0u, st);
  }
  docstage::add_payload(mine, payload);
}

}  // namespace ygm

using namespace ygm;

extern "C" {

// the flat tier at k_snap_text's two LDS sizes: again == 0: 6 KiB per document; again == 1: 24 KiB for the documents
// the first launch left (claim[] written by every launch for the documents it looked at)
int ygm_k_launch_text_flat(const ygm_docs* d, const ygm_side* names, const ygm_results* r, uint8_t* claim, unsigned long long* pay, int again, hipStream_t s) {
  if (d->n_docs == 0) return 0;
  auto k = again ? k_text_flat<24576> : k_text_flat<6144>;
  hipLaunchKernelGGL(k, dim3(d->n_docs), dim3(docstage::NT), 0, s, d->arena, d->doc_off, names->arena, names->off, d->n_docs, d->flags, r->out,
                     r->out_off, r->out_len, r->status, claim, pay, again ? 1u : 0u, r->slot_total);
  return ygm_launch_rc(__func__);
}
// the general path over the workspaces ygm_k_launch_snap_plan sized (w->cnt, w->ws_off); dpw as ygm_k_launch_snap
int ygm_k_launch_text(const ygm_docs* d, const ygm_side* names, uint32_t mode, const ygm_ws* w, const ygm_results* r,
                      unsigned long long* payload, hipStream_t s) {
  if (d->n_docs == 0) return 0;
  const uint32_t dpw = docstage::docs_per_wave(0);
  const uint32_t g = (d->n_docs + dpw - 1) / dpw;
  hipLaunchKernelGGL(k_text, dim3(g), dim3(docstage::NT), 0, s, d->arena, d->doc_off, names->arena, names->off, d->n_docs, d->flags, mode,
                     (const uint4*)w->cnt, (const uint64_t*)w->ws_off, w->ws, r->out_off, r->out_len, r->status, payload, dpw, w->claim, w->base);
  return ygm_launch_rc(__func__);
}

}  // extern "C"
