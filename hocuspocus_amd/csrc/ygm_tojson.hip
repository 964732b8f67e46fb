// ygm_tojson.hip -- toJSON of stored documents' Map, Array and Text roots (ygm_tojson_v1; ygm_tojson.hpp for the
// semantics):
//   k_tojson : k_json's batch with another walker -- a wave's documents staged in LDS, dpw per wave (staging, lane
//              prologue and epilogue: ygm_docstage.hpp), workspaces from the snapshot's count and scan launches
//              (ygm_k_launch_snap_plan), the JSON in the workspace's output region.
// A kernel of its own, in a file of its own: k_json's two instantiations carry none of this walker and stay what they
// were.  The JSON is not bounded by Caps::out (a control character is written as six bytes): the overflow route is
// k_json's -- a document whose JSON does not fit records the needed length, claims that many bytes of the overflow
// region after the workspaces with the launch's atomic cursor and puts itself on a list; the engine grows the buffer
// and launches k_tojson again for the listed documents alone (again = 1: one per lane, parsed again, unstaged), each
// into its claimed region.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "ygm_common.hpp"
#include "ygm_docmeta.hpp"
#include "ygm_tojson.hpp"
#include "ygm_json_batch.hpp"
#include "ygm_launch.hpp"

namespace ygm {

// the batch's walker (ygm_json_batch.hpp): toJSON of a Map, Array or Text root
template <bool FLOATS>
struct ToJsonWalk {
  template <class... A> static YDEV int doc(A&&... a) { return tojson::tojson_doc<FLOATS>(a...); }
  template <class... A> static YDEV int run(A&&... a) { return tojson::tojson_run<FLOATS>(a...); }
};

// The batch and its arguments: docstage::json_batch.
// FLOATS (a context opened with YGM_F_FLOATS): the walk's FLOATS form (tojson::emit_tojson) -- an instantiation of its
// own, so the kernel of a context without the flag carries none of the number conversion and stays what it was.
template <bool FLOATS>
__global__ __launch_bounds__(docstage::NT) void k_tojson(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off,
                                                 const uint8_t* __restrict__ names, const uint64_t* __restrict__ name_off, uint32_t n_docs,
                                                 uint32_t flags, uint32_t kind, const uint4* __restrict__ cnt, const uint64_t* __restrict__ ws_off,
                                                 uint8_t* __restrict__ ws, uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_len,
                                                 int32_t* __restrict__ status, DocMeta* __restrict__ meta, uint32_t dpw, uint64_t base,
                                                 uint64_t ovf_base, uint32_t* __restrict__ list, uint32_t n_list, uint32_t again) {
  __shared__ __attribute__((aligned(16))) uint8_t stg[docstage::STAGE + 16];
  docstage::json_batch<ToJsonWalk<FLOATS>>(stg, arena, doc_off, names, name_off, n_docs, flags, kind, cnt, ws_off, ws, out_off, out_len, status, meta,
                                   dpw, base, ovf_base, list, n_list, again);
}

}  // namespace ygm

using namespace ygm;

extern "C" {

// as ygm_k_launch_json, and its signature: over the workspaces ygm_k_launch_snap_plan sized (w->cnt, w->ws_off); run->again:
// the listed documents' second run (n_list of them).  kind: YGM_TOJSON_MAP / _ARRAY / _TEXT (checked by the engine).
// A root has no field list: `fields` is not read
int ygm_k_launch_tojson(const ygm_docs* d, const ygm_side* names, uint32_t kind, const ygm_ws* w, const ygm_results* r,
                        const ygm_rerun* run, void* meta, int /*fields*/, hipStream_t s) {
  const uint32_t n = run->again ? run->n_list : d->n_docs;
  if (n == 0) return 0;
  const uint32_t dpw = docstage::docs_per_wave(0);
  const uint32_t g = (n + dpw - 1) / dpw;
  auto k = d->flags & F_FLOATS ? k_tojson<true> : k_tojson<false>;
  hipLaunchKernelGGL(k, dim3(g), dim3(docstage::NT), 0, s, d->arena, d->doc_off, names->arena, names->off, d->n_docs, d->flags, kind,
                     (const uint4*)w->cnt, (const uint64_t*)w->ws_off, w->ws, r->out_off, r->out_len, r->status, (DocMeta*)meta, dpw, w->base,
                     run->ovf_base, run->list, run->n_list, run->again ? 1u : 0u);
  return ygm_launch_rc(__func__);
}

}  // extern "C"
