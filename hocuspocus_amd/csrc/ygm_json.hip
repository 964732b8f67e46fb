// ygm_json.hip -- stored documents as ProseMirror / Tiptap JSON (ygm_json_v1, and ygm_json_fields_v1's object of
// several fields; ygm_json.hpp for the semantics):
//   k_json : a wave's documents staged in LDS, dpw per wave (staging, lane prologue and epilogue: ygm_docstage.hpp),
//            workspaces from the snapshot's count and scan launches (ygm_k_launch_snap_plan), the JSON in the
//            workspace's output region.
// There is no LDS flat tier: the flat-text envelope has no nested types, so it holds no ProseMirror document.
// Unlike the text, the JSON is not bounded by Caps::out (every op repeats the current marks).  A document whose JSON
// does not fit records the needed length, claims that many bytes of the overflow region after the workspaces with
// the launch's atomic cursor (as the merge overflow does) and puts itself on a list; the engine grows the buffer and
// launches k_json again for the listed documents alone (again = 1: one per lane, parsed again, unstaged -- the rare
// path), each into its claimed region.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "ygm_common.hpp"
#include "ygm_docmeta.hpp"
#include "ygm_json.hpp"
#include "ygm_json_batch.hpp"
#include "ygm_launch.hpp"

namespace ygm {

// the batch's walker (ygm_json_batch.hpp): the ProseMirror JSON of one field, or the object of several
template <bool FIELDS, bool FLOATS>
struct JsonWalk {
  template <class... A> static YDEV int doc(A&&... a) { return json::json_doc<FIELDS, FLOATS>(a...); }
  template <class... A> static YDEV int run(A&&... a) { return json::json_run<FIELDS, FLOATS>(a...); }
};

// The batch and its arguments: docstage::json_batch.
// FIELDS (ygm_json_fields_v1): names / name_off hold a field list per document and the JSON is the object of its
// fields; staging, workspaces and the overflow route are the same, so the single-field kernel is its own instantiation
// and carries none of the fields code.
// FLOATS (a context opened with YGM_F_FLOATS): the walk's FLOATS form (json::Walk) -- instantiations of their own again,
// so the two kernels of a context without the flag carry none of the number conversion and stay what they were.
template <bool FIELDS, bool FLOATS>
__global__ __launch_bounds__(docstage::NT) void k_json(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off,
                                               const uint8_t* __restrict__ names, const uint64_t* __restrict__ name_off, uint32_t n_docs,
                                               uint32_t flags, uint32_t kind, const uint4* __restrict__ cnt, const uint64_t* __restrict__ ws_off,
                                               uint8_t* __restrict__ ws, uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_len,
                                               int32_t* __restrict__ status, DocMeta* __restrict__ meta, uint32_t dpw, uint64_t base,
                                               uint64_t ovf_base, uint32_t* __restrict__ list, uint32_t n_list, uint32_t again) {
  __shared__ __attribute__((aligned(16))) uint8_t stg[docstage::STAGE + 16];
  docstage::json_batch<JsonWalk<FIELDS, FLOATS>>(stg, arena, doc_off, names, name_off, n_docs, flags, kind, cnt, ws_off, ws, out_off, out_len, status,
                                         meta, dpw, base, ovf_base, list, n_list, again);
}

}  // namespace ygm

using namespace ygm;

extern "C" {

// over the workspaces ygm_k_launch_snap_plan sized (w->cnt, w->ws_off); dpw as ygm_k_launch_text.  run->again: the listed
// documents' second run (n_list of them).  fields: names hold field lists (ygm_json_fields_v1)
int ygm_k_launch_json(const ygm_docs* d, const ygm_side* names, uint32_t kind, const ygm_ws* w, const ygm_results* r,
                      const ygm_rerun* run, void* meta, int fields, hipStream_t s) {
  const uint32_t n = run->again ? run->n_list : d->n_docs;
  if (n == 0) return 0;
  const uint32_t dpw = docstage::docs_per_wave(0);
  const uint32_t g = (n + dpw - 1) / dpw;
  auto k = d->flags & F_FLOATS ? (fields ? k_json<true, true> : k_json<false, true>) : (fields ? k_json<true, false> : k_json<false, false>);
  hipLaunchKernelGGL(k, dim3(g), dim3(docstage::NT), 0, s, d->arena, d->doc_off, names->arena, names->off, d->n_docs, d->flags, kind,
                     (const uint4*)w->cnt, (const uint64_t*)w->ws_off, w->ws, r->out_off, r->out_len, r->status, (DocMeta*)meta, dpw, w->base,
                     run->ovf_base, run->list, run->n_list, run->again ? 1u : 0u);
  return ygm_launch_rc(__func__);
}

}  // extern "C"
