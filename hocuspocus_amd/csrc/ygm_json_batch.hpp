// ygm_json_batch.hpp -- the batch that k_json<false>, k_json<true> and k_tojson share (HIP only): a wave's documents
// staged in LDS, the JSON in the workspace's output region, and the overflow route for a JSON that does not fit.
// A kernel is its parameter list and one call of json_batch<W>; the walker W supplies the two runs:
//   W::doc : the first run of a staged document into its workspace (ST_JSON_MORE and the length needed when it does not fit)
//   W::run : the second run of a listed document, unstaged, into the region its first run claimed
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ygm_common.hpp"
#include "ygm_docmeta.hpp"
#include "ygm_json.hpp"
#include "ygm_docstage.hpp"

namespace ygm {
namespace docstage {

// again == 0: documents [0, n_docs), dpw per wave.  again == 1: the n_list documents of list[], the lanes of a wave
// taking consecutive entries; document d writes out_len[d] bytes (the length its first run recorded) at out_off[d].
// ovf_base: where the overflow region starts in ws (after the workspaces).  stg: the kernel's STAGE + 16 bytes of LDS.
template <class W>
__device__ __forceinline__ void json_batch(uint8_t* stg, const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off,
                                           const uint8_t* __restrict__ names, const uint64_t* __restrict__ name_off, uint32_t n_docs,
                                           uint32_t flags, uint32_t kind, const uint4* __restrict__ cnt, const uint64_t* __restrict__ ws_off,
                                           uint8_t* __restrict__ ws, uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_len,
                                           int32_t* __restrict__ status, DocMeta* __restrict__ meta, uint32_t dpw, uint64_t base,
                                           uint64_t ovf_base, uint32_t* __restrict__ list, uint32_t n_list, uint32_t again) {
  uint64_t mine = 0;
  if (!again) {
    const Lane L = lane_doc(stg, arena, doc_off, n_docs, dpw);
    const uint32_t d = L.d;
    if (L.on) {
      const uint4 c = cnt[d];
      const uint64_t a = doc_off[d], b = doc_off[d + 1], na = name_off[d], nb = name_off[d + 1];
      uint32_t oo = 0, ol = 0;
      snap::Caps k;
      int st = lane_caps(nb >= na && nb - na < (1ull << 30), a, b, c, k);
      if (st == ST_OK) st = W::doc(L.in, c.w, flags, ws + base + ws_off[d], k, names + na, (uint32_t)(nb - na), kind, oo, ol);
      if (st == json::ST_JSON_MORE) {   // ol: the length needed
        const uint32_t i = atomicAdd(&meta->fb_count, 1u);
        const unsigned long long at = atomicAdd(&meta->cursor, (unsigned long long)snap::al16(ol));
        list[i] = d;   // (i < n_docs: a document lists itself once)
        out_off[d] = ovf_base + at;
        out_len[d] = ol;
        status[d] = st;
      } else mine = put(d, out_off, out_len, status, base + ws_off[d] + oo, st == ST_OK ? ol : 0u, st);
    }
  } else {
    const uint32_t i = blockIdx.x * dpw + threadIdx.x;
    if (threadIdx.x < dpw && i < n_list) {
      const uint32_t d = list[i];
      const uint4 c = cnt[d];
      const uint64_t a = doc_off[d], na = name_off[d], nb = name_off[d + 1];
      const uint32_t need = (uint32_t)out_len[d];
      const snap::Caps k = snap::caps_of(c.x, c.y, c.z, c.w);
      uint32_t ol = 0;
      int st = W::run(arena + a, c.w, flags, ws + base + ws_off[d], k, names + na, (uint32_t)(nb - na), kind, ws + out_off[d], need, ol);
      if (st == json::ST_JSON_MORE || (st == ST_OK && ol != need)) st = ST_NOMEM;   // (cannot happen: the same walk twice)
      out_len[d] = st == ST_OK ? ol : 0u;   // (out_off[d]: the place the first run claimed)
      status[d] = st;
      mine = st == ST_OK ? ol : 0u;
    }
  }
  add_payload(mine, &meta->payload);
}

}  // namespace docstage
}  // namespace ygm
