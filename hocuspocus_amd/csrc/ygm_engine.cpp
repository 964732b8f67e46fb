// ygm_engine.cpp -- host runtime behind include/ygm.h.
//
// One context per GPU: a HIP stream, grow-only device workspaces, host result
// buffers and HIP-event timers.  A batch call = H2D of the packed inputs, one
// fast-path launch (look-back placed, packed output), an 8-byte-class meta
// read, the sequential kernel only when some document needed it, D2H.
// The stored-document operations (snapshot, text, JSON, contains) are one
// workspace batch: ws_begin / ws_flat / ws_plan / ws_finish.  Every read-back
// goes through read_meta, read_u64s or read_u64_pair, which count the call's host waits.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <thread>
#include <vector>

#include "../../include/ygm.h"
#include "ygm_chunks.hpp"
#include "ygm_docmeta.hpp"
#include "ygm_launch.hpp"

namespace {

using Meta = ygm::DocMeta;   // the per-launch device counters: the kernels' own struct (read_meta, the counter memsets)
unsigned long long payload_total(const Meta& m) {
  unsigned long long t = m.payload;
  for (unsigned long long x : m.payload_sh) t += x;
  return t;
}

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  // keep > 0: the first `keep` bytes survive a regrowth (copied on stream s, which is then synchronised)
  bool ensure(size_t n, size_t keep = 0, hipStream_t s = nullptr) {
    if (n <= cap && p) return true;
    if (p && keep) {
      void* q = nullptr;
      size_t c = n + n / 4;
      if (hipMalloc(&q, c) != hipSuccess) return false;
      if (hipMemcpyAsync(q, p, std::min(keep, cap), hipMemcpyDeviceToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        (void)hipFree(q); return false;
      }
      (void)hipFree(p); p = q; cap = c;
      return true;
    }
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    size_t c = std::max<size_t>(n, 256);
    c += c / 4;  // grow with headroom
    if (hipMalloc(&p, c) != hipSuccess) { p = nullptr; return false; }
    cap = c;
    return true;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return (T*)p; }
};

// pinned (page-locked) host memory: DMA-able staging for the host API's copies
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  bool ensure(size_t n, size_t keep = 0) {   // keep: leading bytes preserved across a regrowth
    if (n <= cap && p) return true;
    size_t c = std::max<size_t>(n, 4096);
    c += c / 4;
    void* q = nullptr;
    if (hipHostMalloc(&q, c, hipHostMallocDefault) != hipSuccess) return false;
    if (p) { if (keep) memcpy(q, p, std::min(keep, cap)); (void)hipHostFree(p); }
    p = q; cap = c;
    return true;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
  template <class T> T* as() const { return (T*)p; }
};

}  // namespace

struct ygm_ctx {
  int device = 0;
  uint32_t flags = 0;
  uint32_t lean_flags = 0;   // bits for the narrow lean kernel alone (LN_F_NO_IDLEN: YGM_LN_NO_IDLEN, read at ygm_open)
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // the large-document tier's 16-wave launch, beside the mid size's on `stream`
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr;
  // device inputs (host API staging)
  DevBuf arena, offs, docs, sv_arena, sv_offs, opt;   // (opt: the chunk's per-document option bytes, *_opts_v1)
  // device outputs + state
  DevBuf out, out_off, out_len, status, lb, meta, fb_list, defer_list, defer2_list, defer_w_list, route_list;
  // where a call's results go: the per-document buffers as prep_outputs (or ws_begin) left them, over an output arena
  // (`out` for the merge and the walkers), the slot region's and the arena's size
  ygm_results results_in(const DevBuf& arena, uint64_t slot_total, uint64_t out_cap) const {
    return {arena.as<uint8_t>(), out_off.as<uint64_t>(), out_len.as<uint64_t>(), status.as<int32_t>(), slot_total, out_cap};
  }
  ygm_results results(uint64_t slot_total, uint64_t out_cap) const { return results_in(out, slot_total, out_cap); }
  // ... of a workspace batch, whose bytes lie in sn_ws (the flat tier's slots first); the pending documents' launches
  // read their PendHdr records back through it
  ygm_results ws_results(uint64_t slot_total = 0) const { return results_in(sn_ws, slot_total, sn_ws.cap); }
  // ... of a version cut: per-unit slots in the `total` bytes of vr_out
  ygm_results vr_results(uint64_t total) const {
    return {vr_out.as<uint8_t>(), vr_off.as<uint64_t>(), vr_len.as<uint64_t>(), vr_st.as<int32_t>(), total, total};
  }
  ygm_packed packed() const { return {s2_data.as<uint8_t>(), s2_off.as<uint64_t>(), s2_st.as<int32_t>()}; }   // (after pack_snapshots)
  // step2 of pending documents: their parts as step2_pending_split placed them
  ygm_pend_parts pend_parts() const { return {pq_off.as<uint64_t>(), pq_a.as<uint8_t>(), pq_b.as<uint8_t>(), pq_c.as<uint8_t>(), pq_s.as<uint8_t>()}; }
  // the pending documents' three-update batch (arena: false in the planning pass, which sizes it)
  ygm_pend_batch pend_batch(bool arena) const { return {pn_off.as<uint64_t>(), pn_du.as<uint32_t>(), arena ? pn_arena.as<uint8_t>() : nullptr}; }
  Meta* h_meta = nullptr;  // pinned read-back of the per-launch counters
  int mslot = 0;           // counter slot of the next merge launch
  void* meta_slot(int i) const { return (uint8_t*)meta.p + (size_t)i * sizeof(Meta); }
  DevBuf s_readers, s_order, s_tmp, s_ubase, s_ulen, s_cnt, s_drec;
  DevBuf big_blk, big_rec, big_list, big_scan, big_up;   // large-document tier: block tables, struct records, documents sent on, scan
  DevBuf sv_tbl, sv_tn;                // diff: sorted state-vector tables (k_sv_table) and their entry counts
  // shared-state diff / step2: per ask the checked state id, the scanned state lengths (slot bases, n_asks + 1), scan
  // scratch; step2: the asks of pending states and their count
  DevBuf ask_ix, ask_base, ask_bs, ask_pl, ask_pn;
  // the workspace batch (snapshot, text, JSON, contains): per-document counts, workspace offsets, scan scratch,
  // [flat-tier output slots | workspaces], flat-tier claims, its payload / claimed counters
  DevBuf sn_cnt, sn_off, sn_bs, sn_ws, sn_claim, sn_pay;
  DevBuf sn_pend, pn_off, pn_du, pn_arena;   // snapshot: documents left pending, their three-update batch for the merge
  DevBuf pq_off, pq_a, pq_b, pq_c, pq_s, pq_st;   // step2 of pending documents: their parts and state vectors, statuses
  ygm_ctx* pend_ctx = nullptr;               // ... merged on this child context (its own buffers and counters)
  ygm_ctx* pend_dx[2] = {nullptr, nullptr};  // ... and the step2 diffs of their parts on these
  // update V2: per-update V1 sizes -> offsets, transcoding statuses, scan scratch, the V1 arena, per-document column
  // lengths, the V2 outputs (packed), their offsets / lengths / statuses
  DevBuf v2_len, v2_st, v2_bs, v2_v1, v2_L, v2_out, v2_off, v2_olen, v2_ost, v2_fo, v2_claim, v2_pay, v2_scr, v21_cl;
  // host API: results in pinned memory (packed outputs, per-document offset / length / status), the
  // pinned input staging of this context when it serves as a pipeline stage, the packed device copy,
  // and the two stage contexts (own streams and buffers) that double-buffer a batch's chunks
  PinBuf h_data, h_off, h_len, h_status, h_in;
  DevBuf pk_data, pk_off, pk_bsum;
  DevBuf vr_out, vr_off, vr_len, vr_st, vr_pk, vr_pkoff;   // version restore: the cut's slots, places, lengths, statuses; the cut updates packed
  DevBuf s2_data, s2_off, s2_bsum, s2_st;   // sync step2: packed snapshots, their offsets, scan scratch, snapshot statuses
  ygm_ctx* kid[2] = {nullptr, nullptr};
  std::vector<uint32_t> h_doc_upd;
  ygm_stats_t stats{};
  // the batch enqueued by ygm_merge_v1_device_async, completed by ygm_merge_v1_device_finish
  struct Pending {
    bool live = false;
    hipStream_t s = nullptr;
    ygm_merge_in in{};   // what every tier reads (in.meta: the counter slot of the launch)
    ygm_results res{};   // where every tier writes
    uint64_t arena_bytes = 0;
    uint32_t n_upd = 0, n_docs = 0;
    bool wide_route = false;   // the launch was the wide lean kernel over the whole batch
    // the compact input form (ygm_merge_v1_device_lens): in.upd_off is the context's table, built for deferred documents
    const uint64_t* doc_off = nullptr; const uint16_t* upd_len = nullptr;
  } pend;
  DevBuf lens_off;   // update-offset table of a compact-form batch (entries of the documents the lean kernel defers)
  uint32_t lean_span_n = 0;   // lean launches enqueued since the last finish (timed as one span, e0 .. e1)
};

static int herr(hipError_t e) { return e == hipSuccess ? YGM_OK : YGM_EDEVICE; }
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return YGM_EDEVICE; } while (0)

extern "C" {

const char* ygm_version(void) { return "ygm 0.1 (gfx950; yjs 13.6.26 update-v1 semantics)"; }

const char* ygm_strerror(int code) {
  switch (code) {
    case YGM_OK: return "ok";
    case YGM_EMALFORMED: return "Unexpected end of array / malformed update";
    case YGM_ERANGE: return "Integer out of Range";
    case YGM_ENONCANON: return "non-canonical content (yjs would re-encode it)";
    case YGM_ESURROGATE: return "lone surrogate in string slice (yjs 13.5 compat)";
    case YGM_EDEPTH: return "Any/JSON nesting too deep";
    case YGM_ENOMEM: return "out of device memory";
    case YGM_EDEVICE: return "HIP device error";
    case YGM_EINVAL: return "invalid argument";
    case YGM_EUNSUPPORTED: return "outside the snapshot kernel's envelope (pending structs / delete set, sub-documents, ...)";
  }
  return "unknown error";
}

int ygm_open(int device, uint32_t flags, ygm_ctx** out) {
  if (!out) return YGM_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return YGM_EDEVICE;
  ygm_ctx* c = new ygm_ctx();
  c->device = device; c->flags = flags;
  // YGM_LN_NO_IDLEN (A/B runs and tests inside one build): every document takes the narrow lean kernel's generic parse
  c->lean_flags = getenv("YGM_LN_NO_IDLEN") != nullptr ? ygm_k_lean_no_idlen_flag() : 0u;
  // stream2 (the large-document tier's 16-wave size) is created at the high priority on first use: a queue of its own
  // (a process with more streams than hardware queues shares them, and two streams on one queue run their kernels
  // one after the other); contexts that never run that size (the host API's stage contexts, most pool members) do
  // not hold one
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->e0) != hipSuccess || hipEventCreate(&c->e1) != hipSuccess || hipEventCreate(&c->e2) != hipSuccess ||
      hipEventCreate(&c->e3) != hipSuccess) {
    delete c;
    return YGM_EDEVICE;
  }
  // counter slots: 0 / 1 alternate between merge launches (each lean launch zeroes the other
  // slot for the next one: no reset kernel per batch), 2 = SV / diff (reset per call)
  if (!c->meta.ensure(3 * sizeof(Meta)) || hipMemset(c->meta.p, 0, 3 * sizeof(Meta)) != hipSuccess) { ygm_close(c); return YGM_ENOMEM; }
  if (hipHostMalloc((void**)&c->h_meta, sizeof(Meta), hipHostMallocDefault) != hipSuccess) { c->h_meta = nullptr; ygm_close(c); return YGM_ENOMEM; }
  *out = c;
  return YGM_OK;
}

void ygm_close(ygm_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  for (ygm_ctx* k : c->kid) if (k) ygm_close(k);
  if (c->pend_ctx) ygm_close(c->pend_ctx);
  for (ygm_ctx* k : c->pend_dx) if (k) ygm_close(k);
  for (hipEvent_t e : {c->e0, c->e1, c->e2, c->e3}) if (e) (void)hipEventDestroy(e);
  if (c->h_meta) (void)hipHostFree(c->h_meta);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  delete c;   // every DevBuf / PinBuf member frees itself
}

int ygm_stats(ygm_ctx* c, ygm_stats_t* out) {
  if (!c || !out) return YGM_EINVAL;
  *out = c->stats;
  return YGM_OK;
}

// ------------------------------------------------------------------ device API
static int prep_outputs(ygm_ctx* c, uint32_t n_docs, uint64_t out_cap, hipStream_t s, bool lookback) {
  const size_t tiles = (size_t)n_docs / 256 + 2;  // look-back tiles of the SV/diff kernels (256 documents each)
  if (!c->out.ensure(out_cap + 64) || !c->out_off.ensure((size_t)n_docs * 8 + 8) || !c->out_len.ensure((size_t)n_docs * 8 + 8) ||
      !c->status.ensure((size_t)n_docs * 4 + 4) || !c->lb.ensure(tiles * 8) || !c->fb_list.ensure((size_t)n_docs * 4 + 4) ||
      !c->defer_list.ensure((size_t)n_docs * 4 + 4) || !c->defer2_list.ensure((size_t)n_docs * 4 + 4) ||
      !c->defer_w_list.ensure((size_t)n_docs * 4 + 4) || !c->route_list.ensure((size_t)n_docs * 4 + 4))
    return YGM_ENOMEM;
  if (lookback) {   // SV / diff: look-back tiles and counter slot 2 reset per call
    HIPCHK(hipMemsetAsync(c->lb.p, 0, tiles * 8, s));
    HIPCHK(hipMemsetAsync(c->meta_slot(2), 0, sizeof(Meta), s));
  }
  return YGM_OK;
}

static int read_meta(ygm_ctx* c, hipStream_t s, Meta& m, const void* slot) {
  c->stats.host_syncs++;
  HIPCHK(hipMemcpyAsync(c->h_meta, slot, sizeof(Meta), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  m = *c->h_meta;
  return YGM_OK;
}
// Every read-back smaller than a Meta goes through the three helpers below (through the pinned h_meta), so
// ygm_stats_t.host_syncs counts each of the calls' waits.
static_assert(sizeof(Meta) >= 5 * sizeof(uint64_t), "h_meta holds read_u64s' four values and the large tier's five counters");
// one 8-byte value from each of up to four device places, read with one wait
static int read_u64s(ygm_ctx* c, hipStream_t s, std::initializer_list<const uint64_t*> src, uint64_t* v) {
  if (src.size() > 4) return YGM_EINVAL;
  c->stats.host_syncs++;
  uint64_t* h = (uint64_t*)c->h_meta;
  for (const uint64_t* p : src) HIPCHK(hipMemcpyAsync(h++, p, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  memcpy(v, c->h_meta, 8 * src.size());
  return YGM_OK;
}
// the two consecutive values at d_p (a tier's byte and document counters), one 16-byte copy
static int read_u64_pair(ygm_ctx* c, hipStream_t s, const uint64_t* d_p, uint64_t (&v)[2]) {
  c->stats.host_syncs++;
  HIPCHK(hipMemcpyAsync(c->h_meta, d_p, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  memcpy(v, c->h_meta, 16);
  return YGM_OK;
}
static uint64_t read_u64(ygm_ctx* c, hipStream_t s, const uint64_t* d_p, int& e) {
  uint64_t v = 0;
  e = read_u64s(c, s, {d_p}, &v);
  return v;
}

static void fill_dev_result(ygm_ctx* c, uint64_t data_bytes, ygm_device_result* out) {
  const ygm_results r = c->results(0, 0);
  out->data = r.out; out->off = r.out_off; out->len = r.out_len; out->status = r.status;
  out->data_bytes = data_bytes;
  out->payload_bytes = data_bytes;
}

static int merge_async(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_upd_off, const uint32_t* d_doc_upd,
                       uint32_t n_upd, uint32_t n_docs, void* stream, const uint64_t* d_doc_off, const uint16_t* d_upd_len) {
  if (!c) return YGM_EINVAL;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  // output arena: one slot per document (2|in| + 64 B, no cross-document dependency),
  // then the overflow region for outputs that outgrow their slot (<= 3|in| + 16/doc)
  const uint64_t slot_total = 2 * arena_bytes + 64ull * n_docs;
  const uint64_t out_cap = slot_total + 3 * arena_bytes + 16ull * n_docs + 64;
  int e = prep_outputs(c, n_docs, out_cap, s, false);
  if (e) return e;
  // the wide route: a batch whose average document outgrows the narrow kernel's staging (multi-character inserts,
  // many clients: the realistic logs of c2_mixed) would be deferred by it almost whole -- a pass that only reads
  // headers yet costs as much as merging a C2 batch (latency-bound) -- so the wide kernel takes every document
  const bool wide_route = n_docs && arena_bytes / n_docs > (uint64_t)ygm_k_lean_stage_bytes() && getenv("YGM_NO_WIDE_ROUTE") == nullptr;
  if (d_doc_off) {   // compact form: the table every tier after the narrow kernel reads (only deferred documents' entries)
    if (!c->lens_off.ensure(8ull * n_upd + 16)) return YGM_ENOMEM;
    d_upd_off = c->lens_off.as<uint64_t>();
    if (wide_route && ygm_k_launch_build_off(d_doc_off, d_upd_len, d_doc_upd, nullptr, n_docs, c->lens_off.as<uint64_t>(), s))
      return YGM_EDEVICE;
  }
  // tier 1: lean wave-per-document kernel (debounce-log shape); everything else is deferred.
  // Timing: one event before the first launch since the last finish, one in finish after the
  // last -- per-launch event pairs between back-to-back launches cost ~8 us of stream time each.
  if (c->lean_span_n == 0) HIPCHK(hipEventRecord(c->e0, s));
  c->lean_span_n++;
  const ygm_merge_in in{d_arena, d_upd_off, d_doc_upd, c->flags, c->meta_slot(c->mslot)};
  const ygm_results res = c->results(slot_total, out_cap);
  void* meta_next = c->meta_slot(1 - c->mslot);   // zeroed by this launch for the next one
  if (wide_route) {
    if (ygm_k_launch_merge_lean_wide(&in, &res, n_docs, nullptr, n_docs, meta_next, c->defer_w_list.as<uint32_t>(), d_upd_len, s))
      return YGM_EDEVICE;
  } else if (ygm_k_launch_merge_lean(&in, &res, n_docs, c->lean_flags, meta_next, c->defer_list.as<uint32_t>(), d_doc_off, d_upd_len, s))
    return YGM_EDEVICE;
  ygm_ctx::Pending& P = c->pend;
  P.wide_route = wide_route;
  if (n_docs) c->mslot = 1 - c->mslot;   // (an empty batch launches nothing: the slot stays current)
  P.live = true; P.s = s; P.in = in; P.res = res;
  P.arena_bytes = arena_bytes; P.n_upd = n_upd; P.n_docs = n_docs;
  P.doc_off = wide_route ? nullptr : d_doc_off; P.upd_len = d_upd_len;   // (wide route: the table is whole)
  return YGM_OK;
}
int ygm_merge_v1_device_async(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_upd_off,
                              const uint32_t* d_doc_upd, uint32_t n_upd, uint32_t n_docs, void* stream) {
  return merge_async(c, d_arena, arena_bytes, d_upd_off, d_doc_upd, n_upd, n_docs, stream, nullptr, nullptr);
}
int ygm_merge_v1_device_lens_async(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off,
                                   const uint16_t* d_upd_len, const uint32_t* d_doc_upd, uint32_t n_upd, uint32_t n_docs, void* stream) {
  if (!d_doc_off || !d_upd_len) return YGM_EINVAL;
  return merge_async(c, d_arena, arena_bytes, nullptr, d_doc_upd, n_upd, n_docs, stream, d_doc_off, d_upd_len);
}

// ---- ygm_merge_v1_device_finish: the tiers after the lean launch, a step each.  A step enqueues its kernels on the
// call's stream between the events e0 and e1, reads the counters back (one host wait) and leaves them to the next.
struct MergeRun {
  ygm_ctx* c;
  hipStream_t s;
  const ygm_ctx::Pending& P;
  Meta m{};             // the call's counters as last read
  uint32_t n_gen = 0;   // documents the lean kernels left to the general tiers
  uint32_t n_seq = 0;   // documents the large-document tier left to the sequential replay
  unsigned long long cnt[5] = {0, 0, 0, 0, 0};   // tier 4: the scan's counters ([4], the slow queue's entries: the YGM_TIER_COUNTS line's only)
  int reread() {        // the counters after a step; a kernel's fault ends the call
    const int e = read_meta(c, s, m, P.in.meta);
    return e ? e : m.fault ? YGM_EDEVICE : YGM_OK;
  }
  void add_span() {     // e0 .. e1 into the kernel time (after the wait that follows e1)
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) c->stats.kernel_ms += ms;
  }
  int lean_span(), general(), large(), seq();
  void report(ygm_device_result* out);
};
// the lean span (every lean launch since the last finish, e0 .. e1) and the counters its last launch left
int MergeRun::lean_span() {
  HIPCHK(hipEventRecord(c->e1, s));
  if (const int e = reread()) return e;
  float ms = 0;
  if (c->lean_span_n && hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) { c->stats.kernel_ms += ms; c->stats.lean_ms += ms; }
  c->stats.lean_launches += c->lean_span_n;
  c->lean_span_n = 0;
  return YGM_OK;
}
// The general tiers, chained on the device: the wide lean kernel (tier 1b: updates <= 64 bytes, documents <= 7 KB),
// the routing pass that takes the large-document tier's documents out (k_route_big), the wave kernel (tier 2) and the
// workgroup kernel (tier 3: documents over the wave class).  Each reads its count from the counter the kernel before
// it wrote (stream order; the host's `bound` only sizes the persistent grid) -- one host wait for all of them.
// On the wide route the wide kernel took the whole batch at the launch (async): it does not run here, the routing
// pass takes the host's count of its deferrals, and the documents it was given are the batch.
int MergeRun::general() {
  // the DocMeta counters the tier kernels read as the device-side counts of their lists
  const unsigned int* d_wide_defer = (const unsigned int*)((const char*)P.in.meta + offsetof(Meta, wide_defer));
  const unsigned int* d_defer_count = (const unsigned int*)((const char*)P.in.meta + offsetof(Meta, defer_count));
  const unsigned int* d_route_n = (const unsigned int*)((const char*)P.in.meta + offsetof(Meta, route_n));
  uint32_t *narrow_left = c->defer_list.as<uint32_t>(), *wide_left = c->defer_w_list.as<uint32_t>(), *routed = c->route_list.as<uint32_t>(),
           *wave_left = c->defer2_list.as<uint32_t>(), *to_large = c->fb_list.as<uint32_t>();
  const uint32_t wide_in = P.wide_route ? P.n_docs : m.lean_defer;      // documents given to the wide kernel
  const uint32_t bound = P.wide_route ? m.wide_defer : m.lean_defer;    // documents the chain may see (0: no chain)
  n_gen = P.wide_route ? m.wide_defer : 0;
  HIPCHK(hipEventRecord(c->e0, s));
  if (bound) {
    if (!P.wide_route) {
      if (P.doc_off && ygm_k_launch_build_off(P.doc_off, P.upd_len, P.in.doc_upd, narrow_left, bound, const_cast<uint64_t*>(P.in.upd_off), s))
        return YGM_EDEVICE;   // (compact form: the deferred documents' offsets)
      if (ygm_k_launch_merge_lean_wide(&P.in, &P.res, P.n_docs, narrow_left, bound, nullptr, wide_left, P.upd_len, s)) return YGM_EDEVICE;
    }
    if (ygm_k_launch_route_big(&P.in, &P.res, wide_left, P.wide_route ? nullptr : d_wide_defer, bound, to_large, routed, s) ||
        ygm_k_launch_merge_wave(&P.in, &P.res, routed, d_route_n, bound, wave_left, to_large, s) ||
        ygm_k_launch_merge_fast(&P.in, &P.res, wave_left, d_defer_count, bound, to_large, s))
      return YGM_EDEVICE;
    HIPCHK(hipEventRecord(c->e1, s));
    if (const int e = reread()) return e;
    add_span();
    if (!P.wide_route) n_gen = m.wide_defer;
  }
  c->stats.docs_lean_wide += wide_in - n_gen;
  return YGM_OK;
}
// Tier 4: large [snapshot, ...log] documents, one workgroup each; what it cannot finish goes on to tier 5 (n_seq).
// The snapshot scan; then documents with a snapshot over BIG_MID_U0 on the 16-wave size (stream2) beside the mid size
// over the rest (stream); a log over the mid size's LDS goes on to the 16-wave size after it.
int MergeRun::large() {
  const uint64_t blk_cap = m.fb_bytes / 4 + 2ull * m.fb_count + 16, rec_cap = m.fb_bytes + 2ull * m.fb_count + 16;
  if (!c->big_blk.ensure(blk_cap * ygm_k_big_blk_bytes()) || !c->big_rec.ensure(rec_cap * ygm_k_big_rec_bytes()) ||
      !c->big_list.ensure((size_t)m.fb_count * 4 + 4) || !c->big_up.ensure((size_t)m.fb_count * 4 + 4) ||
      !c->big_scan.ensure(ygm_k_big_scan_bytes(m.fb_count, m.fb_bytes)))
    return YGM_ENOMEM;
  const ygm_big_tier big{c->fb_list.as<uint32_t>(), m.fb_count, m.fb_bytes, c->big_scan.p, c->big_blk.p, blk_cap, c->big_rec.p, rec_cap,
                         c->big_up.as<uint32_t>(), c->big_list.as<uint32_t>()};
  HIPCHK(hipEventRecord(c->e0, s));
  if (ygm_k_launch_big_scan(&P.in, &big, s)) return YGM_EDEVICE;
  unsigned long long* d_cnt; uint32_t *llist, *mlist;
  ygm_k_big_lists(big.scan, big.n_fb, big.fb_bytes, &d_cnt, &llist, &mlist);
  c->stats.host_syncs++;
  HIPCHK(hipMemcpyAsync(c->h_meta, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  memcpy(cnt, c->h_meta, sizeof cnt);
  const uint32_t n_wide = (uint32_t)cnt[2], n_mid = (uint32_t)cnt[3];   // documents that start on the 16-wave / the mid size
  // once the 16-wave size runs on stream2, every exit waits for it: its kernels write the outputs, the counters
  // and the tier's scratch, which the next call on this context reuses on `stream`
  struct Join2 {
    hipStream_t st = nullptr;
    ~Join2() { if (st) (void)hipStreamSynchronize(st); }
  } join2;
  if (n_wide) {
    if (!c->stream2) {   // created on first use, only on contexts that run the 16-wave size
      int prio_lo = 0, prio_hi = 0;
      HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
#ifndef YGM_S2_PRIO
#define YGM_S2_PRIO 1
#endif
      HIPCHK(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, YGM_S2_PRIO ? prio_hi : prio_lo));
    }
    HIPCHK(hipEventRecord(c->e2, s));
    HIPCHK(hipStreamWaitEvent(c->stream2, c->e2, 0));
    join2.st = c->stream2;
    if (ygm_k_launch_merge_big(1, &P.in, &P.res, &big, llist, n_wide, c->stream2)) return YGM_EDEVICE;
    HIPCHK(hipEventRecord(c->e3, c->stream2));
    if (n_mid && ygm_k_launch_big_wait(P.in.meta, n_wide, s)) return YGM_EDEVICE;   // (their workgroups resident first)
  }
  if (ygm_k_launch_merge_big(0, &P.in, &P.res, &big, mlist, n_mid, s)) return YGM_EDEVICE;
  if (const int e = reread()) return e;
  if (m.mid_defer && ygm_k_launch_merge_big(1, &P.in, &P.res, &big, big.up_list, m.mid_defer, s)) return YGM_EDEVICE;
  if (n_wide) { HIPCHK(hipStreamWaitEvent(s, c->e3, 0)); join2.st = nullptr; }
  HIPCHK(hipEventRecord(c->e1, s));
  if (const int e = reread()) return e;
  add_span();
  c->stats.docs_big += m.fb_count - m.big_defer;
  n_seq = m.big_defer;
  return YGM_OK;
}
// Tier 5: the exact sequential replay of the documents tier 4 left (scratch sized from its counters: an upper bound)
int MergeRun::seq() {
  const uint64_t upd_cap = m.fb_upds + 1, byte_cap = m.fb_bytes + 8ull * m.fb_count + 8;
  if (!c->s_readers.ensure(upd_cap * ygm_k_seq_reader_bytes()) || !c->s_order.ensure(upd_cap * 4) || !c->s_tmp.ensure(upd_cap * 4) ||
      !c->s_ubase.ensure(upd_cap * 8) || !c->s_ulen.ensure(upd_cap * 4) || !c->s_cnt.ensure(byte_cap * 4) ||
      !c->s_drec.ensure((byte_cap / 2 + 1) * ygm_k_drec_bytes()))
    return YGM_ENOMEM;
  const ygm_seq_scratch scr{c->s_readers.p, c->s_order.as<int>(), c->s_tmp.as<int>(), c->s_ubase.as<const uint8_t*>(), c->s_ulen.as<uint32_t>(),
                            c->s_cnt.as<uint32_t>(), c->s_drec.p, upd_cap, byte_cap};
  HIPCHK(hipEventRecord(c->e0, s));
  if (ygm_k_launch_merge_seq(&P.in, &P.res, c->big_list.as<uint32_t>(), n_seq, &scr, s)) return YGM_EDEVICE;
  HIPCHK(hipEventRecord(c->e1, s));
  if (const int e = read_meta(c, s, m, P.in.meta)) return e;
  add_span();
  c->stats.docs_seq += n_seq;
  return YGM_OK;
}
// the tier lines, the call's statistics and its result
void MergeRun::report(ygm_device_result* out) {
  // YGM_TIER_COUNTS (testing knob): the call's raw tier counters, one stderr line (all 0 when the chain did not run)
  if (getenv("YGM_TIER_COUNTS"))
    fprintf(stderr, "ygm merge tiers: docs %u lean_defer %u wide_defer %u to_wave %u to_workgroup %u to_large %u to_seq %u\n", P.n_docs,
            m.lean_defer, m.wide_defer, m.route_n, m.defer_count, m.fb_count, m.big_defer);
  // ... and, when tier 4 ran, the large-document tier's: the scan's carves and slow queue, the two lists, the hand-ons
  if (m.fb_count && getenv("YGM_TIER_COUNTS"))
    fprintf(stderr, "ygm large tiers: docs %u positions %llu tasks %llu slow_queue %llu wide_first %llu mid_first %llu mid_to_wide %u to_seq %u\n",
            m.fb_count, cnt[0], cnt[1], cnt[4], cnt[2], cnt[3], m.mid_defer, m.big_defer);
  c->stats.calls++; c->stats.docs += P.n_docs; c->stats.updates += P.n_upd;
  c->stats.docs_fast += n_gen - m.fb_count;   // finished by the wave / workgroup tiers (tier 4 counted above)
  c->stats.docs_lean += P.n_docs - n_gen;      // finished by the lean kernels (narrow + wide)
  c->stats.bytes_in += P.arena_bytes; c->stats.bytes_out += payload_total(m);
  fill_dev_result(c, P.res.slot_total + m.cursor, out);
  out->payload_bytes = payload_total(m);
}

int ygm_merge_v1_device_finish(ygm_ctx* c, ygm_device_result* out) {
  if (!c || !out || !c->pend.live) return YGM_EINVAL;
  c->pend.live = false;
  (void)hipSetDevice(c->device);
  MergeRun R{c, c->pend.s, c->pend};
  int e;
  if ((e = R.lean_span()) || (e = R.general())) return e;
  if (R.m.fb_count && (e = R.large())) return e;
  if (R.n_seq && (e = R.seq())) return e;
  R.report(out);
  return YGM_OK;
}

int ygm_merge_v1_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_upd_off,
                        const uint32_t* d_doc_upd, uint32_t n_upd, uint32_t n_docs, void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  const int e = ygm_merge_v1_device_async(c, d_arena, arena_bytes, d_upd_off, d_doc_upd, n_upd, n_docs, stream);
  if (e) return e;
  return ygm_merge_v1_device_finish(c, out);
}
int ygm_merge_v1_device_lens(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off,
                             const uint16_t* d_upd_len, const uint32_t* d_doc_upd, uint32_t n_upd, uint32_t n_docs, void* stream,
                             ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  const int e = ygm_merge_v1_device_lens_async(c, d_arena, arena_bytes, d_doc_off, d_upd_len, d_doc_upd, n_upd, n_docs, stream);
  if (e) return e;
  return ygm_merge_v1_device_finish(c, out);
}

// the plan of a shared-state call: c->ask_ix (checked state id per ask) and c->ask_base (exclusive scan of the asks'
// state lengths, the total at [n_asks])
static int ask_plan(ygm_ctx* c, hipStream_t s, const uint64_t* d_doc_off, uint32_t n_docs, const uint32_t* d_ask_doc, uint32_t n_asks) {
  const size_t nb = ((size_t)n_asks + 1 + 255) / 256 + 2;
  if (!c->ask_ix.ensure(4ull * n_asks + 4) || !c->ask_base.ensure(8ull * n_asks + 16) || !c->ask_bs.ensure(8 * nb)) return YGM_ENOMEM;
  return ygm_k_launch_ask_plan(d_doc_off, n_docs, d_ask_doc, n_asks, c->ask_ix.as<uint32_t>(), c->ask_base.as<uint64_t>(),
                               c->ask_bs.as<uint64_t>(), s) ? YGM_EDEVICE : YGM_OK;
}

enum { DOC_SV = 0, DOC_DIFF = 1 };   // the walker kernels' mode argument (ygm_k_launch_doc, ygm_k_launch_doc_lean)
// gather (DOC_DIFF only): the batch is n_asks asks over n_docs shared documents, ask a answered from document
// d_ask_doc[a] with state vector a; results are indexed by ask, slots placed from the asks' scanned state lengths
static int run_doc_kernel(ygm_ctx* c, int mode, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off,
                          const uint8_t* d_sv, uint64_t sv_bytes, const uint64_t* d_sv_off, uint32_t n_docs, void* stream,
                          ygm_device_result* out, uint32_t extra_flags = 0, bool gather = false, const uint32_t* d_ask_doc = nullptr,
                          uint32_t n_asks = 0) {
  const uint32_t flags = c ? c->flags | extra_flags : 0;
  if (!c || !out || (gather && mode != DOC_DIFF)) return YGM_EINVAL;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  int e = YGM_OK;
  const uint32_t n_states = n_docs;
  uint64_t vbytes = arena_bytes;   // gather: the virtual bytes V, the sum over asks of the ask's state length
  if (gather) {
    if ((e = ask_plan(c, s, d_doc_off, n_states, d_ask_doc, n_asks))) return e;
    vbytes = read_u64(c, s, c->ask_base.as<uint64_t>() + n_asks, e);   // the one read that sizes the output region
    if (e) return e;
    n_docs = n_asks;
  }
  // per-document slots (lean kernel), then the packed region of the exact kernel's deferred documents
  const uint64_t slot_total = 2 * vbytes + 64ull * n_docs;
  const uint64_t out_cap = slot_total + 2 * vbytes + 32ull * n_docs + 64;
  e = prep_outputs(c, n_docs, out_cap, s, true);
  if (e) return e;
  void* meta = c->meta_slot(2);
  const ygm_results res = c->results(slot_total, out_cap);
  if (mode == DOC_DIFF && (!c->sv_tbl.ensure(ygm_k_sv_table_bytes(n_docs)) || !c->sv_tn.ensure(4ull * n_docs + 4))) return YGM_ENOMEM;
  HIPCHK(hipEventRecord(c->e0, s));
  if (gather) {
    if (ygm_k_launch_doc_lean_gather(d_arena, d_doc_off, d_sv, d_sv_off, c->ask_ix.as<uint32_t>(), c->ask_base.as<uint64_t>(), n_asks, &res,
                                     meta, c->defer_list.as<uint32_t>(), c->sv_tbl.as<uint8_t>(), c->sv_tn.as<uint32_t>(), s))
      return YGM_EDEVICE;
  } else
  if (ygm_k_launch_doc_lean(mode, d_arena, arena_bytes, d_doc_off, d_sv, sv_bytes, d_sv_off, n_docs, flags, &res, meta,
                            c->defer_list.as<uint32_t>(), c->sv_tbl.as<uint8_t>(), c->sv_tn.as<uint32_t>(), s))
    return YGM_EDEVICE;
  HIPCHK(hipEventRecord(c->e1, s));
  Meta m;
  if ((e = read_meta(c, s, m, meta))) return e;
  if (m.fault) return YGM_EDEVICE;
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) { c->stats.kernel_ms += ms; c->stats.lean_ms += ms; c->stats.lean_launches++; }
  // YGM_TIER_COUNTS (testing knob): who finished the call's documents, one stderr line (exact: the walker's deferred list)
  if (getenv("YGM_TIER_COUNTS"))
    fprintf(stderr, "ygm walk tiers: op %s docs %u walker %u exact %u\n", gather ? "diff_shared" : mode == DOC_DIFF ? "diff" : "sv", n_docs,
            n_docs - m.lean_defer, m.lean_defer);
  if (m.lean_defer) {   // the exact per-document kernel over the deferred list, packed after the slots
    HIPCHK(hipEventRecord(c->e0, s));
    if (gather) {
      if (ygm_k_launch_doc_gather(d_arena, d_doc_off, d_sv, d_sv_off, c->defer_list.as<uint32_t>(), c->ask_ix.as<uint32_t>(), m.lean_defer,
                                  flags, &res, c->lb.as<unsigned long long>(), meta, s))
        return YGM_EDEVICE;
    } else
    if (ygm_k_launch_doc(mode, d_arena, d_doc_off, d_sv, d_sv_off, c->defer_list.as<uint32_t>(), m.lean_defer, flags, &res,
                         c->lb.as<unsigned long long>(), meta, s))
      return YGM_EDEVICE;
    HIPCHK(hipEventRecord(c->e1, s));
    if ((e = read_meta(c, s, m, meta))) return e;
    if (m.fault) return YGM_EDEVICE;
    if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) c->stats.kernel_ms += ms;
  }
  // gather: an ask of a refused state id carries YGM_EINVAL (whatever the kernels left there)
  if (gather && ygm_k_launch_ask_status(c->ask_ix.as<uint32_t>(), n_asks, nullptr, res.status, res.out_len, s))
    return YGM_EDEVICE;
  const uint64_t payload = payload_total(m) + m.fast_total;
  c->stats.calls++; c->stats.docs += n_docs; c->stats.docs_fast += m.lean_defer; c->stats.docs_lean += n_docs - m.lean_defer;
  c->stats.bytes_in += arena_bytes; c->stats.bytes_out += payload;
  fill_dev_result(c, slot_total + m.fast_total, out);
  out->payload_bytes = payload;
  return YGM_OK;
}

static ygm_batch_out batch_out(const ygm_device_result& r) { return {r.data, r.off, r.len, r.status}; }   // (for a later launch)
// The pending documents' three-update batch (c->pn_arena / pn_off / pn_du, `total` bytes) merged on the child context
// c->pend_ctx; the merged bytes appended to `dst` at `used` and the documents' places, lengths and statuses written
// (k_pend_fix; pst: statuses decided before the merge, nullable)
static int pend_merge_place(ygm_ctx* c, hipStream_t s, uint32_t P, uint64_t total, const int32_t* pst, DevBuf& dst, uint64_t used,
                            uint64_t& data_bytes, unsigned long long& payload, const uint32_t* list = nullptr) {
  if (!list) list = c->sn_pend.as<uint32_t>();   // (the shared-state step2: its list of asks)
  if (!c->pend_ctx) { const int e = ygm_open(c->device, c->flags, &c->pend_ctx); if (e) return e; }
  const ygm_pend_batch b = c->pend_batch(true);
  int e = ygm_merge_v1_device_async(c->pend_ctx, b.dst, total, b.upd_off, b.doc_upd, 3 * P, P, s);
  ygm_device_result r;
  if (!e) e = ygm_merge_v1_device_finish(c->pend_ctx, &r);
  if (e) return e;
  if (!dst.ensure(used + r.data_bytes + 64, used, s)) return YGM_ENOMEM;
  if (r.data_bytes) HIPCHK(hipMemcpyAsync(dst.as<uint8_t>() + used, r.data, r.data_bytes, hipMemcpyDeviceToDevice, s));
  const ygm_batch_out merged = batch_out(r);
  const ygm_results res = c->results_in(dst, 0, dst.cap);
  if (ygm_k_launch_pend_fix(list, P, &merged, pst, used, &res, s)) return YGM_EDEVICE;
  data_bytes = used + r.data_bytes;
  payload += r.payload_bytes;
  c->stats.docs_pending += P;
  return YGM_OK;
}
// Documents k_snap left pending (ST_PEND: PendHdr, then [state, pendingDs, pending structs]): encodeStateAsUpdate
// returns mergeUpdates of the three (Y@23300).  They are packed into one arena as three-update documents (k_pend_plan /
// k_pend_copy) and merged by pend_merge_place, which appends the merged bytes to the snapshot's output region at `used`.
static int snap_resolve_pending(ygm_ctx* c, hipStream_t s, uint32_t P, uint64_t used, uint64_t& data_bytes, unsigned long long& payload) {
  if (!c->pn_off.ensure(8ull * (3ull * P + 1) + 16) || !c->pn_du.ensure(4ull * (P + 1) + 16)) return YGM_ENOMEM;
  ygm_pend_batch b = c->pend_batch(false);
  const ygm_results rec = c->ws_results();   // (the documents' records)
  if (ygm_k_launch_pend_plan(c->sn_pend.as<uint32_t>(), P, rec.out, rec.out_off, &b, s)) return YGM_EDEVICE;
  int e = 0;
  const uint64_t total = read_u64(c, s, b.upd_off + 3ull * P, e);
  if (e) return e;
  if (!c->pn_arena.ensure(total + 64)) return YGM_ENOMEM;
  HIPCHK(hipMemsetAsync(c->pn_arena.as<uint8_t>() + total, 0, 64, s));   // (the merge kernels' tail padding)
  b = c->pend_batch(true);
  if (ygm_k_launch_pend_copy(c->sn_pend.as<uint32_t>(), P, rec.out, rec.out_off, &b, s)) return YGM_EDEVICE;
  return pend_merge_place(c, s, P, total, nullptr, c->sn_ws, used, data_bytes, payload);
}

// ---- the workspace batch: the steps the stored-document operations share (snapshot, text, JSON, contains).  A batch
// writes per-document places, lengths and statuses (c->out_off, out_len, status) and its bytes into c->sn_ws:
// [the flat tier's per-document slots | the general path's workspaces], the workspaces sized by a count and scan
// launch into c->sn_off.  An operation names only what differs: its launches, its tier line, what it does with the
// counters.  The context's snapshot buffers serve every operation (one batch in flight per context).
struct WsBatch {
  ygm_ctx* c; hipStream_t s; uint32_t n_docs;
  void* meta;               // counter slot 2, reset by ws_begin
  uint64_t slot_total = 0;  // bytes of the flat tier's slot region (0: the tier did not run)
  uint64_t total = 0;       // bytes of the workspaces after it (ws_plan)
  uint64_t flat_pay = 0, flat_docs = 0, flat_first = 0;   // flat tier: payload bytes, documents claimed, by launch 0
  const uint8_t* claim() const { return slot_total ? c->sn_claim.as<uint8_t>() : nullptr; }
  // the launch arguments (ygm_launch.hpp): the batch's documents under the call's flags, the workspaces (after ws_plan,
  // which grows the buffer), the results over c->sn_ws
  ygm_docs docs(const uint8_t* arena, const uint64_t* off, uint32_t flags, const uint8_t* opt = nullptr) const { return {arena, off, n_docs, flags, opt}; }
  ygm_ws ws() const { return {c->sn_cnt.p, c->sn_off.as<uint64_t>(), c->sn_ws.as<uint8_t>(), slot_total, claim()}; }
  ygm_results results() const { return c->ws_results(slot_total); }
  unsigned long long* payload() const { return (unsigned long long*)((uint8_t*)meta + offsetof(Meta, payload)); }
  unsigned int* fb_count() const { return (unsigned int*)((uint8_t*)meta + offsetof(Meta, fb_count)); }
};
// begin: the per-document buffers, the counters reset, event e0
static int ws_begin(ygm_ctx* c, hipStream_t s, uint32_t n_docs, WsBatch& B) {
  const uint32_t nb = (n_docs + 1 + 255) / 256;
  if (!c->sn_cnt.ensure(16ull * n_docs + 16) || !c->sn_off.ensure(8ull * n_docs + 16) || !c->sn_bs.ensure(8ull * nb + 16) ||
      !c->out_off.ensure(8ull * n_docs + 8) || !c->out_len.ensure(8ull * n_docs + 8) || !c->status.ensure(4ull * n_docs + 4))
    return YGM_ENOMEM;
  B.c = c; B.s = s; B.n_docs = n_docs; B.meta = c->meta_slot(2);
  HIPCHK(hipMemsetAsync(B.meta, 0, sizeof(Meta), s));
  HIPCHK(hipEventRecord(c->e0, s));
  return YGM_OK;
}
// the flat tier: launch(results, claims, counters, again) writes flat documents (input + workspace in LDS) into per-document slots of c->sn_ws
// and claims them -- 6 KiB of LDS per document, then 24 KiB for what that left; one read of the tier's counters after
// each.  The documents it leaves take the general path, whose workspaces follow the slot region.  YGM_SNAP_NOLDS
// (testing knob) turns the tier off.
extern "C++" template <class L>
static int ws_flat(WsBatch& B, uint64_t in_bytes, L launch) {
  ygm_ctx* c = B.c;
  if (!B.n_docs || getenv("YGM_SNAP_NOLDS")) return YGM_OK;
  B.slot_total = 2 * in_bytes + 64ull * B.n_docs + 64;
  if (!c->sn_ws.ensure(B.slot_total + 64) || !c->sn_claim.ensure((size_t)B.n_docs + 16) || !c->sn_pay.ensure(16)) return YGM_ENOMEM;
  HIPCHK(hipMemsetAsync(c->sn_pay.p, 0, 16, B.s));
  uint64_t pay[2] = {0, 0};
  const ygm_results r = B.results();   // (over the slot region)
  for (int again = 0; again < 2 && pay[1] < B.n_docs; again++) {
    if (launch(r, c->sn_claim.as<uint8_t>(), c->sn_pay.as<unsigned long long>(), again)) return YGM_EDEVICE;
    const int e = read_u64_pair(c, B.s, c->sn_pay.as<uint64_t>(), pay);
    if (e) return e;
    if (again == 0) B.flat_first = pay[1];
  }
  B.flat_pay = pay[0]; B.flat_docs = pay[1];
  return YGM_OK;
}
// plan: the count and scan launches (cont: the containment's), one read of the scanned total, c->sn_ws grown to hold
// the workspaces after the slot region, which is kept
static int ws_plan(WsBatch& B, const ygm_docs& d, bool cont = false) {
  ygm_ctx* c = B.c;
  const ygm_ws w = B.ws();   // (its buffer as it is now: the plan sizes it)
  if ((cont ? ygm_k_launch_cont_plan : ygm_k_launch_snap_plan)(&d, &w, c->sn_bs.as<uint64_t>(), B.s)) return YGM_EDEVICE;
  int e = 0;
  if (B.n_docs) B.total = read_u64(c, B.s, w.ws_off + B.n_docs, e);
  if (e) return e;
  return c->sn_ws.ensure(B.slot_total + B.total + 64, B.slot_total, B.s) ? YGM_OK : YGM_ENOMEM;
}
// finish: event e1 and the wait for it, the call's statistics, the result over `data`
static int ws_finish(WsBatch& B, uint64_t in_bytes, uint8_t* data, uint64_t data_bytes, uint64_t payload, ygm_device_result* out) {
  ygm_ctx* c = B.c;
  HIPCHK(hipEventRecord(c->e1, B.s));
  HIPCHK(hipEventSynchronize(c->e1));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->e0, c->e1) == hipSuccess) c->stats.kernel_ms += ms;
  c->stats.calls++; c->stats.docs += B.n_docs; c->stats.bytes_in += in_bytes; c->stats.bytes_out += payload;
  const ygm_results r = B.results();
  out->data = data; out->off = r.out_off; out->len = r.out_len; out->status = r.status; out->data_bytes = data_bytes; out->payload_bytes = payload;
  return YGM_OK;
}

// the snapshot batch; xf: YGM_F_SNAP_STATE (contains) for states that leave pending parts
// leave: when non-null, documents left pending are not resolved: their count goes there (list c->sn_pend, statuses
// ST_PEND, their PendHdr layouts at out_off)
// dpw: k_snap's documents per wave (0: its default)
// d_opt: the documents' option bytes (YGM_DOC_NO_GC; null: none set), read by k_snap_text and k_snap
static int snapshot_dev(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off, uint32_t n_docs,
                        hipStream_t s, ygm_device_result* out, uint32_t xf, uint32_t* leave = nullptr, uint32_t dpw = 0,
                        const uint8_t* d_opt = nullptr) {
  if (leave) *leave = 0;
  WsBatch B;
  int e = ws_begin(c, s, n_docs, B);
  if (e) return e;
  const ygm_docs d = B.docs(d_arena, d_doc_off, c->flags | xf, d_opt);
  // tier 1: k_snap_text (the flat-text tier writes updates only: a take batch, YGM_F_SNAP_VERSION, goes to k_snap whole)
  if (!(xf & YGM_F_SNAP_VERSION) && (e = ws_flat(B, arena_bytes, [&](const ygm_results& r, uint8_t* claim, unsigned long long* pay, int again) {
        return ygm_k_launch_snap_text(&d, &r, claim, pay, again, s);
      })))
    return e;
  uint64_t total_out = 0;   // the output region's extent when pending documents' merged bytes follow the workspaces
  Meta m;
  memset(&m, 0, sizeof(m));
  if (!B.slot_total || B.flat_docs < n_docs) {   // the count / scan / k_snap path
    if ((e = ws_plan(B, d))) return e;
    if (!c->sn_pend.ensure(4ull * n_docs + 16)) return YGM_ENOMEM;
    const ygm_ws w = B.ws();
    const ygm_results r = B.results();
    if (ygm_k_launch_snap(&d, &w, &r, B.payload(), c->sn_pend.as<uint32_t>(), B.fb_count(), dpw, s)) return YGM_EDEVICE;
    if ((e = read_meta(c, s, m, B.meta))) return e;
    if (m.fb_count && leave) *leave = m.fb_count;
    else if (m.fb_count && (e = snap_resolve_pending(c, s, m.fb_count, B.slot_total + B.total, total_out, m.payload))) return e;
  }
  m.payload += B.flat_pay;
  // YGM_TIER_COUNTS (testing knob): the tier that finished the call's documents, one stderr line (general: the count /
  // scan / k_snap path, the documents it left pending among them)
  if (getenv("YGM_TIER_COUNTS"))
    fprintf(stderr, "ygm snapshot tiers: docs %u text_first %llu text_second %llu general %llu pending %u\n", n_docs,
            (unsigned long long)B.flat_first, (unsigned long long)(B.flat_docs - B.flat_first), (unsigned long long)(n_docs - B.flat_docs),
            m.fb_count);
  c->stats.docs_snapshot += n_docs;
  return ws_finish(B, arena_bytes, c->sn_ws.as<uint8_t>(), total_out ? total_out : B.slot_total + B.total, m.payload, out);
}
int ygm_snapshot_opts_v1_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off,
                                const uint8_t* d_doc_opt, uint32_t n_docs, void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  (void)hipSetDevice(c->device);
  return snapshot_dev(c, d_arena, arena_bytes, d_doc_off, n_docs, stream ? (hipStream_t)stream : c->stream, out, 0, nullptr, 0, d_doc_opt);
}
int ygm_snapshot_v1_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off, uint32_t n_docs,
                           void* stream, ygm_device_result* out) {
  return ygm_snapshot_opts_v1_device(c, d_arena, arena_bytes, d_doc_off, nullptr, n_docs, stream, out);
}
// ---- plain text of stored documents: the snapshot batch's tiers with another last stage.  k_text_flat as the flat
// tier, then k_text over the workspaces for the documents it left.  Nothing is left pending: a state with pending
// parts is read through its integrated part.
int ygm_text_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off, const uint8_t* d_names,
                       const uint64_t* d_name_off, uint32_t mode, uint32_t n_docs, void* stream, ygm_device_result* out) {
  if (!c || !out || mode > YGM_TEXT_DEEP || (n_docs && (!d_state_off || !d_name_off))) return YGM_EINVAL;
  (void)hipSetDevice(c->device);
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  WsBatch B;
  int e = ws_begin(c, s, n_docs, B);
  if (e) return e;
  const ygm_docs d = B.docs(d_states, d_state_off, c->flags);
  const ygm_side names{d_names, d_name_off};
  if ((e = ws_flat(B, states_bytes, [&](const ygm_results& r, uint8_t* claim, unsigned long long* pay, int again) {
        return ygm_k_launch_text_flat(&d, &names, &r, claim, pay, again, s);
      })))
    return e;
  Meta m;
  memset(&m, 0, sizeof(m));
  if (n_docs && (!B.slot_total || B.flat_docs < n_docs)) {
    if ((e = ws_plan(B, d))) return e;
    const ygm_ws w = B.ws();
    const ygm_results r = B.results();
    if (ygm_k_launch_text(&d, &names, mode, &w, &r, B.payload(), s)) return YGM_EDEVICE;
    if ((e = read_meta(c, s, m, B.meta))) return e;
  }
  if (getenv("YGM_TIER_COUNTS"))   // (testing knob, as the snapshot's line: the tier that finished the call's documents)
    fprintf(stderr, "ygm text tiers: docs %u flat_first %llu flat_second %llu general %llu\n", n_docs, (unsigned long long)B.flat_first,
            (unsigned long long)(B.flat_docs - B.flat_first), (unsigned long long)(n_docs - B.flat_docs));
  return ws_finish(B, states_bytes, c->sn_ws.as<uint8_t>(), B.slot_total + B.total, m.payload + B.flat_pay, out);
}
// ---- stored documents as ProseMirror JSON: k_json over the workspaces (no flat tier: its envelope holds no nested
// types).  A JSON is not bounded by its workspace's output region: k_json lists the documents whose JSON did not fit,
// with the lengths they need and their places in an overflow region claimed from the launch's cursor; only then the
// buffer grows by that region (the workspaces, which hold the other documents' outputs, are kept) and k_json runs
// again for the listed documents alone -- one more host wait.  fields: the second arena holds a field list per
// document (ygm_json_fields_v1): the same batch, k_json's fields instantiation in both launches.
// tojson: ygm_tojson_v1 -- the same batch with k_tojson in both launches, its kind one of YGM_TOJSON_*; the load is
// the snapshot's (counted in docs_snapshot).
static int json_dev(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off, const uint8_t* d_names,
                    const uint64_t* d_name_off, uint32_t kind, uint32_t n_docs, void* stream, ygm_device_result* out, int fields,
                    int tojson = 0) {
  if (!c || !out || (tojson ? kind > YGM_TOJSON_TEXT : kind != YGM_JSON_PROSEMIRROR) || (n_docs && (!d_state_off || !d_name_off)))
    return YGM_EINVAL;
  (void)hipSetDevice(c->device);
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  WsBatch B;
  int e = ws_begin(c, s, n_docs, B);
  if (e) return e;
  if (!c->sn_pend.ensure(4ull * n_docs + 16)) return YGM_ENOMEM;
  const ygm_docs d = B.docs(d_states, d_state_off, c->flags);
  const ygm_side names{d_names, d_name_off};
  uint64_t ovf = 0;
  uint32_t reran = 0;
  Meta m;
  memset(&m, 0, sizeof(m));
  if (n_docs) {
    if ((e = ws_plan(B, d))) return e;
    auto launch = [&](uint32_t n_list, int again) {   // (the buffer may have grown between the two: built per launch)
      const ygm_ws w = B.ws();
      const ygm_results r = B.results();
      const ygm_rerun rr{B.total, c->sn_pend.as<uint32_t>(), n_list, again};
      return (tojson ? ygm_k_launch_tojson : ygm_k_launch_json)(&d, &names, kind, &w, &r, &rr, B.meta, fields, s);
    };
    if (launch(0, 0)) return YGM_EDEVICE;
    if ((e = read_meta(c, s, m, B.meta))) return e;
    if (m.fb_count) {   // the documents whose JSON did not fit: sized from the recorded lengths, run again
      reran = m.fb_count; ovf = m.cursor;
      if (!c->sn_ws.ensure(B.total + ovf + 64, B.total, s)) return YGM_ENOMEM;
      if (launch(reran, 1)) return YGM_EDEVICE;
      if ((e = read_meta(c, s, m, B.meta))) return e;
    }
  }
  if (getenv("YGM_TIER_COUNTS"))   // (testing knob, as the text's line)
    fprintf(stderr, "ygm %s tiers: docs %u general %u overflow %u overflow_bytes %llu\n", tojson ? "tojson" : "json", n_docs, n_docs, reran,
            (unsigned long long)ovf);
  if (tojson) c->stats.docs_snapshot += n_docs;
  return ws_finish(B, states_bytes, c->sn_ws.as<uint8_t>(), B.total + ovf, m.payload, out);
}
int ygm_json_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off, const uint8_t* d_names,
                       const uint64_t* d_name_off, uint32_t kind, uint32_t n_docs, void* stream, ygm_device_result* out) {
  return json_dev(c, d_states, states_bytes, d_state_off, d_names, d_name_off, kind, n_docs, stream, out, 0);
}
int ygm_json_fields_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off, const uint8_t* d_fields,
                              const uint64_t* d_field_off, uint32_t kind, uint32_t n_docs, void* stream, ygm_device_result* out) {
  return json_dev(c, d_states, states_bytes, d_state_off, d_fields, d_field_off, kind, n_docs, stream, out, 1);
}
int ygm_tojson_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off, const uint8_t* d_names,
                         const uint64_t* d_name_off, uint32_t kind, uint32_t n_docs, void* stream, ygm_device_result* out) {
  return json_dev(c, d_states, states_bytes, d_state_off, d_names, d_name_off, kind, n_docs, stream, out, 0, 1);
}
// a snapshot batch's outputs packed into one arena on the device (k_pack_*: offsets n + 1, the total at [n]) with its
// statuses, for kernels that read documents by offsets (step2's diff, contains)
static int pack_snapshots(ygm_ctx* c, hipStream_t s, const ygm_device_result& r1, uint32_t n_docs) {
  const uint32_t nb = (n_docs + 255) / 256;
  if (!c->s2_data.ensure(r1.payload_bytes + 64) || !c->s2_off.ensure(8ull * n_docs + 16) || !c->s2_bsum.ensure(8ull * nb + 16) ||
      !c->s2_st.ensure(4ull * n_docs + 4))
    return YGM_ENOMEM;
  HIPCHK(hipMemsetAsync((uint8_t*)c->s2_data.p + r1.payload_bytes, 0, 64, s));   // readable tail for the walker's chunks
  if (n_docs) {
    if (ygm_k_launch_pack(r1.data, r1.off, r1.len, r1.status, n_docs, c->s2_bsum.as<uint64_t>(), c->s2_data.as<uint8_t>(),
                          c->s2_off.as<uint64_t>(), s))
      return YGM_EDEVICE;
    HIPCHK(hipMemcpyAsync(c->s2_off.as<uint64_t>() + n_docs, c->s2_bsum.as<uint64_t>() + nb, 8, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->s2_st.p, r1.status, 4ull * n_docs, hipMemcpyDeviceToDevice, s));
  } else HIPCHK(hipMemsetAsync(c->s2_off.p, 0, 8, s));
  return YGM_OK;
}

// ---- version history.  take: the snapshot batch in its Y.snapshot view (YGM_F_SNAP_STATE) ending with encode_version
int ygm_version_take_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off, uint32_t n_docs,
                               void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  (void)hipSetDevice(c->device);
  return snapshot_dev(c, d_states, states_bytes, d_state_off, n_docs, stream ? (hipStream_t)stream : c->stream, out,
                      YGM_F_SNAP_STATE | YGM_F_SNAP_VERSION);
}
// the restores' tail over n cut units (documents, or asks): (3) the cut, launched by `cut` into per-unit slots of
// c->vr_out (`total` bytes), (4) packed, padded, (5) snapshotted into the new documents (restored_opt); the cut's
// statuses carried into the result.  cut_ms: the cut's HIP-event time
extern "C++" template <class C>
static int restore_tail(ygm_ctx* c, hipStream_t s, uint32_t n, uint64_t total, C cut, const uint8_t* d_restored_opt, ygm_device_result* out,
                        float& cut_ms) {
  const uint32_t nb = (n + 255) / 256;
  if (!c->vr_out.ensure(total + 64) || !c->vr_off.ensure(8ull * n + 8) || !c->vr_len.ensure(8ull * n + 8) || !c->vr_st.ensure(4ull * n + 4) ||
      !c->vr_pk.ensure(total + 64) || !c->vr_pkoff.ensure(8ull * n + 16) || !c->s2_bsum.ensure(8ull * nb + 16))
    return YGM_ENOMEM;
  HIPCHK(hipEventRecord(c->e2, s));
  if (cut()) return YGM_EDEVICE;
  HIPCHK(hipEventRecord(c->e3, s));
  uint64_t xb = 0;
  int e = 0;
  if (n) {
    if (ygm_k_launch_pack(c->vr_out.as<uint8_t>(), c->vr_off.as<uint64_t>(), c->vr_len.as<uint64_t>(), c->vr_st.as<int32_t>(), n,
                          c->s2_bsum.as<uint64_t>(), c->vr_pk.as<uint8_t>(), c->vr_pkoff.as<uint64_t>(), s))
      return YGM_EDEVICE;
    HIPCHK(hipMemcpyAsync(c->vr_pkoff.as<uint64_t>() + n, c->s2_bsum.as<uint64_t>() + nb, 8, hipMemcpyDeviceToDevice, s));
    xb = read_u64(c, s, c->vr_pkoff.as<uint64_t>() + n, e);
    if (e) return e;
    if (xb > total) return YGM_EDEVICE;
  } else HIPCHK(hipMemsetAsync(c->vr_pkoff.p, 0, 8, s));
  HIPCHK(hipMemsetAsync(c->vr_pk.as<uint8_t>() + xb, 0, 64, s));   // (the snapshot kernels' tail padding)
  cut_ms = 0;
  if (hipEventElapsedTime(&cut_ms, c->e2, c->e3) == hipSuccess) c->stats.kernel_ms += cut_ms;
  if ((e = snapshot_dev(c, c->vr_pk.as<uint8_t>(), xb, c->vr_pkoff.as<uint64_t>(), n, s, out, 0, nullptr, 0, d_restored_opt))) return e;
  if (n && ygm_k_launch_v2_status(c->vr_st.as<int32_t>(), n, out->status, out->len, s)) return YGM_EDEVICE;
  return YGM_OK;
}
// restore: (1) the states' no-GC snapshots in their Y.snapshot view, (2) packed, then restore_tail over the documents
// (k_ver_cut at the versions' clocks with the versions' delete sets appended); the statuses of (1) and (3) carried
int ygm_version_restore_v1_device(ygm_ctx* c, const uint8_t* d_states, const uint64_t* d_state_off, const uint8_t* d_versions,
                                  const uint64_t* d_version_off, const uint8_t* d_restored_opt, uint32_t n_docs, void* stream,
                                  ygm_device_result* out) {
  if (!c || !out || ((uintptr_t)d_versions & 15u)) return YGM_EINVAL;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  uint64_t sv[2] = {0, 0};   // the states' bytes, the versions' bytes
  int e = n_docs ? read_u64s(c, s, {d_state_off + n_docs, d_version_off + n_docs}, sv) : 0;
  if (e) return e;
  ygm_device_result r1;
  const double k0 = c->stats.kernel_ms;
  e = snapshot_dev(c, d_states, sv[0], d_state_off, n_docs, s, &r1, YGM_F_SNAP_STATE | YGM_F_SNAP_NOGC);
  if (e || (e = pack_snapshots(c, s, r1, n_docs))) return e;
  const double k1 = c->stats.kernel_ms;
  const uint64_t total = r1.payload_bytes + sv[1] + 32ull * n_docs + 64;
  float ms = 0;
  const ygm_side versions{d_versions, d_version_off};
  e = restore_tail(c, s, n_docs, total, [&] {   // (the cut's buffers are restore_tail's: built after it has them)
    const ygm_packed S = c->packed();
    const ygm_results r = c->vr_results(total);
    return ygm_k_launch_ver_cut(&S, &versions, n_docs, c->flags, &r, s);
  }, d_restored_opt, out, ms);
  if (e) return e;
  HIPCHK(hipStreamSynchronize(s));
  if (getenv("YGM_VERSION_TIMES"))   // (tools/version_probe.py: the three stages' HIP-event times)
    fprintf(stderr, "ygm version restore: docs %u snapshot_nogc_ms %.3f cut_ms %.3f snapshot_restored_ms %.3f\n", n_docs, k1 - k0, (double)ms,
            c->stats.kernel_ms - k1 - (double)ms);
  return YGM_OK;
}
// k_snap's documents per wave for the states of a shared-state call (0: its default).  k_snap runs 16 documents per wave
// and its lanes diverge by document.  The per-pair call over these asks would hold n_asks / n_states copies of a state
// on neighbouring lanes (no divergence between them): the same number of waves here, with fewer documents each
// (`parity`), is never more serial than that.  While the states fit one resident round of k_snap's waves with fewer per
// wave still (`fill`: 256 CUs x 3 workgroups of 40 KB of LDS), they take that: the shared batch is the smaller one,
// lanes are what it has to spare (profiles/step2_shared/README.md, profiles/version_shared/README.md)
static uint32_t shared_snap_dpw(uint32_t n_states, uint32_t n_asks) {
  if (n_asks <= n_states) return 0;
  const uint32_t parity = std::max<uint32_t>(1u, (uint32_t)(16ull * n_states / n_asks));
  const uint32_t fill = std::max<uint32_t>(1u, (n_states + 767u) / 768u);
  return std::min(parity, fill);
}
// restore of many versions per state: (1) and (2) over the n_states states, each snapshotted once; the ask plan over the
// packed snapshots' offsets (the checked state id per ask and the scan of the asks' snapshot lengths, what sizes the
// cut's slots); restore_tail over the n_asks asks with the gather cut, which reads the packed snapshots in place, and
// the asks' option bytes.  The cut carries a refused id's YGM_EINVAL and a state's refusal to the ask
int ygm_version_restore_shared_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off,
                                         uint32_t n_states, const uint8_t* d_versions, const uint64_t* d_version_off,
                                         const uint32_t* d_ask_state, const uint8_t* d_restored_opt, uint32_t n_asks, void* stream,
                                         ygm_device_result* out) {
  if (!c || !out || ((uintptr_t)d_versions & 15u) || (n_states && !d_state_off) || (n_asks && (!d_version_off || !d_ask_state)))
    return YGM_EINVAL;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  ygm_device_result r1;
  const double k0 = c->stats.kernel_ms;
  int e = snapshot_dev(c, d_states, states_bytes, d_state_off, n_states, s, &r1, YGM_F_SNAP_STATE | YGM_F_SNAP_NOGC, nullptr,
                       shared_snap_dpw(n_states, n_asks));
  if (e || (e = pack_snapshots(c, s, r1, n_states))) return e;
  const double k1 = c->stats.kernel_ms;
  if ((e = ask_plan(c, s, c->s2_off.as<uint64_t>(), n_states, d_ask_state, n_asks))) return e;
  uint64_t av[2] = {0, 0};   // the asks' snapshot bytes, the versions' bytes: the one read that sizes the cut's slots
  if (n_asks && (e = read_u64s(c, s, {c->ask_base.as<uint64_t>() + n_asks, d_version_off + n_asks}, av))) return e;
  const uint64_t total = av[0] + av[1] + 32ull * n_asks + 64;
  float ms = 0;
  const ygm_side versions{d_versions, d_version_off};
  e = restore_tail(c, s, n_asks, total, [&] {
    const ygm_packed S = c->packed();
    const ygm_results r = c->vr_results(total);
    return ygm_k_launch_ver_cut_gather(&S, c->ask_ix.as<uint32_t>(), c->ask_base.as<uint64_t>(), &versions, n_asks, c->flags, &r, s);
  }, d_restored_opt, out, ms);
  if (e) return e;
  // the carries: after the cut's status (restore_tail), as the other shared forms, id and state to ask
  if (n_asks && ygm_k_launch_ask_status(c->ask_ix.as<uint32_t>(), n_asks, c->s2_st.as<int32_t>(), out->status, out->len, s)) return YGM_EDEVICE;
  HIPCHK(hipStreamSynchronize(s));
  if (getenv("YGM_VERSION_TIMES"))   // (tools/version_probe.py: the three stages' HIP-event times)
    fprintf(stderr, "ygm version restore shared: states %u asks %u snapshot_nogc_ms %.3f cut_ms %.3f snapshot_restored_ms %.3f\n", n_states,
            n_asks, k1 - k0, (double)ms, c->stats.kernel_ms - k1 - (double)ms);
  return YGM_OK;
}

// Read-only SyncStep2: the states' Y.snapshot view first -- the snapshot batch with YGM_F_SNAP_STATE (a state that
// leaves pending structs / a pending delete set is seen through its integrated part, as Y.snapshot(doc) sees the
// store) -- packed, then the containment kernels over it; the snapshot's per-document refusals carried into the result
int ygm_contains_v1_device(ygm_ctx* c, const uint8_t* d_states_in, const uint64_t* d_state_off_in, const uint8_t* d_updates,
                           const uint64_t* d_update_off, uint32_t n_docs, void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  int e = 0;
  const uint64_t states_bytes = n_docs ? read_u64(c, s, d_state_off_in + n_docs, e) : 0;
  if (e) return e;
  ygm_device_result r1;
  e = snapshot_dev(c, d_states_in, states_bytes, d_state_off_in, n_docs, s, &r1, YGM_F_SNAP_STATE);
  if (e || (e = pack_snapshots(c, s, r1, n_docs))) return e;
  const ygm_packed S = c->packed();
  // a workspace batch of its own: k_cont_count as the count launch, the answers (a byte per document) in c->out
  WsBatch B;
  if ((e = ws_begin(c, s, n_docs, B))) return e;
  if (!c->out.ensure((uint64_t)n_docs + 64)) return YGM_ENOMEM;
  const ygm_docs d = B.docs(S.data, S.off, c->flags);
  const ygm_side updates{d_updates, d_update_off};
  if ((e = ws_plan(B, d, true))) return e;
  const ygm_ws w = B.ws();
  const ygm_results r = c->results(0, n_docs);
  if (ygm_k_launch_cont(&d, &updates, &w, &r, s)) return YGM_EDEVICE;
  if (n_docs && ygm_k_launch_v2_status(S.st, n_docs, r.status, r.out_len, s)) return YGM_EDEVICE;
  if ((e = ws_finish(B, 0, c->out.as<uint8_t>(), n_docs, 0, out))) return e;   // (the call counts no bytes in or out)
  out->payload_bytes = n_docs;
  return YGM_OK;
}

int ygm_diff_v1_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off, const uint8_t* d_sv_arena,
                       const uint64_t* d_sv_off, uint32_t n_docs, void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  // (the state-vector arena's extent is the last offset; its 16-byte window reads stay inside its padding)
  int e = 0;
  (void)hipSetDevice(c->device);
  const uint64_t sv_end = n_docs ? read_u64(c, stream ? (hipStream_t)stream : c->stream, d_sv_off + n_docs, e) : 0;
  if (e) return e;
  return run_doc_kernel(c, DOC_DIFF, d_arena, arena_bytes, d_doc_off, d_sv_arena, sv_end, d_sv_off, n_docs, stream, out);
}

int ygm_sv_from_update_v1_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off, uint32_t n_docs,
                                 void* stream, ygm_device_result* out) {
  return run_doc_kernel(c, DOC_SV, d_arena, arena_bytes, d_doc_off, nullptr, 0, nullptr, n_docs, stream, out);
}

// SyncStep2 of the documents the snapshot left pending (P of them, list c->sn_pend, PendHdr layouts in its output
// region: split off before the main diff, finished after it): encodeStateAsUpdate(doc, sv) = mergeUpdates([writeStateAsUpdate(doc, sv), pendingDs, diffUpdate(pending
// structs, sv)]) (Y@23300) -- the state part diffed keeping each struct's parentSub bit (an integrated item's write),
// the pending structs by the plain diff (the lazy writer's), on two child contexts; the three merged on a third, and
// appended to the step2 result (`out`, the diff kernels' output region) in the documents' places
// split (before the main diff reuses the snapshot's out_off): parts and state vectors into c->pq_*; tot: their bytes.
// list: the P pending documents, or (gather) the asks of pending states -- ask a's parts come from the workspace record
// of its state c->ask_ix[a], its state vector from the ask
static int step2_pending_split(ygm_ctx* c, hipStream_t s, uint32_t P, const uint32_t* list, bool gather, const uint8_t* d_sv_arena,
                               const uint64_t* d_sv_off, uint64_t (&tot)[4]) {
  const uint64_t np = (uint64_t)P + 1;
  if (!c->pq_off.ensure(8ull * 4 * np + 16) || !c->pq_st.ensure(4ull * P + 16) || !c->pn_off.ensure(8ull * (3ull * P + 1) + 16) ||
      !c->pn_du.ensure(4ull * np + 16))
    return YGM_ENOMEM;
  uint64_t* offs = c->pq_off.as<uint64_t>();
  const ygm_results rec = c->ws_results();   // (the pending states' records)
  const ygm_side sv{d_sv_arena, d_sv_off};
  const uint32_t* ask_ix = gather ? c->ask_ix.as<uint32_t>() : nullptr;
  ygm_pend_parts parts{offs, nullptr, nullptr, nullptr, nullptr};
  if (ygm_k_launch_pend_split(list, P, ask_ix, rec.out, rec.out_off, &sv, &parts, 0, s)) return YGM_EDEVICE;
  const int e = read_u64s(c, s, {offs + P, offs + np + P, offs + 2 * np + P, offs + 3 * np + P}, tot);
  if (e) return e;
  DevBuf* part[4] = {&c->pq_a, &c->pq_b, &c->pq_c, &c->pq_s};
  for (int k = 0; k < 4; k++) {
    if (!part[k]->ensure(tot[k] + 64)) return YGM_ENOMEM;
    HIPCHK(hipMemsetAsync(part[k]->as<uint8_t>() + tot[k], 0, 64, s));   // (readable tail padding for the kernels)
  }
  parts = c->pend_parts();
  return ygm_k_launch_pend_split(list, P, ask_ix, rec.out, rec.out_off, &sv, &parts, 1, s) ? YGM_EDEVICE : YGM_OK;
}
// finish (after the main diff): the two diffs, the join, the merge, the places in `out`
static int step2_pending_finish(ygm_ctx* c, hipStream_t s, uint32_t P, const uint64_t (&tot)[4], ygm_device_result* out,
                                const uint32_t* list = nullptr) {
  const uint64_t np = (uint64_t)P + 1;
  const ygm_pend_parts parts = c->pend_parts();
  for (ygm_ctx*& k : c->pend_dx) if (!k) { const int e = ygm_open(c->device, c->flags, &k); if (e) return e; }
  ygm_device_result ra, rc;
  int e = run_doc_kernel(c->pend_dx[0], 1, parts.da, tot[0], parts.offs, parts.dsv, tot[3], parts.offs + 3 * np, P, s, &ra, YGM_F_KEEP_SUB);
  if (!e) e = run_doc_kernel(c->pend_dx[1], 1, parts.dc, tot[2], parts.offs + 2 * np, parts.dsv, tot[3], parts.offs + 3 * np, P, s, &rc, 0);
  if (e) return e;
  const ygm_batch_out a = batch_out(ra), cc = batch_out(rc);
  ygm_pend_batch b = c->pend_batch(false);
  if (ygm_k_launch_pend_join(P, &a, &cc, &parts, &b, c->pq_st.as<int32_t>(), 0, s)) return YGM_EDEVICE;
  const uint64_t total = read_u64(c, s, b.upd_off + 3ull * P, e);
  if (e) return e;
  if (!c->pn_arena.ensure(total + 64)) return YGM_ENOMEM;
  HIPCHK(hipMemsetAsync(c->pn_arena.as<uint8_t>() + total, 0, 64, s));
  b = c->pend_batch(true);
  if (ygm_k_launch_pend_join(P, &a, &cc, &parts, &b, c->pq_st.as<int32_t>(), 1, s)) return YGM_EDEVICE;
  uint64_t db = 0;
  unsigned long long pay = out->payload_bytes;
  if ((e = pend_merge_place(c, s, P, total, c->pq_st.as<int32_t>(), c->out, out->data_bytes, db, pay, list))) return e;
  out->data = c->out.as<uint8_t>(); out->data_bytes = db; out->payload_bytes = pay;
  return YGM_OK;
}

// SyncStep2 of stored documents (MessageReceiver.ts:137-138): the snapshot batch, its outputs packed into one arena
// on the device (k_pack_*: offsets n + 1, the total at [n]), the diff kernels over it with F_KEEP_SUB, and the
// snapshot's per-document refusals (EUNSUPPORTED, malformed states) carried into the result; states that leave
// pending parts by step2_pending_split / _finish.  d_state_opt: the states' option bytes (a no-GC state's snapshot
// keeps its deleted content, so the diff sends the deleted Items as the reference's live gc: false document does; the
// pending parts are merged, never collected, so only the state part depends on it)
int ygm_sync_step2_opts_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off,
                                  const uint8_t* d_state_opt, const uint8_t* d_sv_arena, const uint64_t* d_sv_off, uint32_t n_docs,
                                  void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  ygm_device_result r1;
  const bool dbg = getenv("YGM_DEBUG") != nullptr;
#define S2CHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { if (dbg) fprintf(stderr, "ygm step2: %s: %s\n", #x, hipGetErrorString(_e)); return YGM_EDEVICE; } } while (0)
  uint32_t P = 0;   // documents the snapshot leaves pending (their parts split off now, answered after the diff)
  uint64_t ptot[4] = {0, 0, 0, 0};
  int e = snapshot_dev(c, d_states, states_bytes, d_state_off, n_docs, s, &r1, 0, &P, 0, d_state_opt);
  if (!e && P) e = step2_pending_split(c, s, P, c->sn_pend.as<uint32_t>(), false, d_sv_arena, d_sv_off, ptot);
  if (dbg) fprintf(stderr, "ygm step2: snapshot rc %d payload %llu\n", e, (unsigned long long)r1.payload_bytes);
  if (e || (e = pack_snapshots(c, s, r1, n_docs))) return e;
  const uint64_t sv_end = n_docs ? read_u64(c, s, d_sv_off + n_docs, e) : 0;
  if (e) return e;
  e = run_doc_kernel(c, DOC_DIFF, c->s2_data.as<uint8_t>(), r1.payload_bytes, c->s2_off.as<uint64_t>(), d_sv_arena, sv_end, d_sv_off, n_docs, s,
                     out, YGM_F_KEEP_SUB);
  if (dbg) fprintf(stderr, "ygm step2: diff rc %d\n", e);
  if (e) return e;
  if (n_docs && ygm_k_launch_v2_status(c->s2_st.as<int32_t>(), n_docs, out->status, out->len, s)) return YGM_EDEVICE;
  if (P && (e = step2_pending_finish(c, s, P, ptot, out))) return e;
  S2CHK(hipStreamSynchronize(s));
  return YGM_OK;
#undef S2CHK
}
int ygm_sync_step2_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off,
                             const uint8_t* d_sv_arena, const uint64_t* d_sv_off, uint32_t n_docs, void* stream,
                             ygm_device_result* out) {
  return ygm_sync_step2_opts_v1_device(c, d_states, states_bytes, d_state_off, nullptr, d_sv_arena, d_sv_off, n_docs, stream, out);
}

// ------------------------------------------------------------------ shared states (device API)
// diffUpdate of n_asks state vectors over n_docs shared updates: the gather walker and the gather exact kernel
int ygm_diff_shared_v1_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off, uint32_t n_docs,
                              const uint8_t* d_sv_arena, const uint64_t* d_sv_off, const uint32_t* d_ask_doc, uint32_t n_asks, void* stream,
                              ygm_device_result* out) {
  if (!c || !out || (n_asks && (!d_sv_off || !d_ask_doc))) return YGM_EINVAL;
  int e = 0;
  (void)hipSetDevice(c->device);
  const uint64_t sv_end = n_asks ? read_u64(c, stream ? (hipStream_t)stream : c->stream, d_sv_off + n_asks, e) : 0;
  if (e) return e;
  return run_doc_kernel(c, DOC_DIFF, d_arena, arena_bytes, d_doc_off, d_sv_arena, sv_end, d_sv_off, n_docs, stream, out, 0, true, d_ask_doc, n_asks);
}

// SyncStep2 of a reconnect storm: the snapshot batch over the n_states states (each once), packed; the gather diff
// with F_KEEP_SUB over the n_asks asks, reading the packed snapshots in place; each state's refusal carried to its
// asks; the asks of states the snapshot left pending split off before the diff (their state's three parts copied per
// ask, the state not snapshotted again) and finished after it at their ask indices.  d_state_opt: one option byte per
// state -- the option acts in the snapshot alone, so a state's asks inherit it (and a bad byte's YGM_EINVAL) through
// the packed snapshot and the status carry; the gather kernels need nothing more
int ygm_sync_step2_shared_opts_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off,
                                         const uint8_t* d_state_opt, uint32_t n_states, const uint8_t* d_sv_arena,
                                         const uint64_t* d_sv_off, const uint32_t* d_ask_state, uint32_t n_asks, void* stream,
                                         ygm_device_result* out) {
  if (!c || !out || (n_asks && (!d_sv_off || !d_ask_state))) return YGM_EINVAL;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  ygm_device_result r1;
  uint32_t P = 0, PA = 0;   // states the snapshot leaves pending; their asks
  uint64_t ptot[4] = {0, 0, 0, 0};
  int e = snapshot_dev(c, d_states, states_bytes, d_state_off, n_states, s, &r1, 0, &P, shared_snap_dpw(n_states, n_asks), d_state_opt);
  if (e) return e;
  if (P && n_asks) {
    if ((e = ask_plan(c, s, d_state_off, n_states, d_ask_state, n_asks))) return e;
    if (!c->ask_pl.ensure(4ull * n_asks + 16) || !c->ask_pn.ensure(16)) return YGM_ENOMEM;
    HIPCHK(hipMemsetAsync(c->ask_pn.p, 0, 16, s));
    if (ygm_k_launch_ask_pending(c->ask_ix.as<uint32_t>(), n_asks, r1.status, c->ask_pl.as<uint32_t>(), c->ask_pn.as<unsigned int>(), s))
      return YGM_EDEVICE;
    PA = (uint32_t)read_u64(c, s, c->ask_pn.as<uint64_t>(), e);
    if (e) return e;
  }
  if (PA && (e = step2_pending_split(c, s, PA, c->ask_pl.as<uint32_t>(), true, d_sv_arena, d_sv_off, ptot))) return e;
  if ((e = pack_snapshots(c, s, r1, n_states))) return e;
  const uint64_t sv_end = n_asks ? read_u64(c, s, d_sv_off + n_asks, e) : 0;
  if (e) return e;
  e = run_doc_kernel(c, DOC_DIFF, c->s2_data.as<uint8_t>(), r1.payload_bytes, c->s2_off.as<uint64_t>(), d_sv_arena, sv_end, d_sv_off, n_states, s,
                     out, YGM_F_KEEP_SUB, true, d_ask_state, n_asks);
  if (e) return e;
  // the status carry from state to ask (the gather form of k_v2_status)
  if (n_states && ygm_k_launch_ask_status(c->ask_ix.as<uint32_t>(), n_asks, c->s2_st.as<int32_t>(), out->status, out->len, s)) return YGM_EDEVICE;
  if (PA && (e = step2_pending_finish(c, s, PA, ptot, out, c->ask_pl.as<uint32_t>()))) return e;
  HIPCHK(hipStreamSynchronize(s));
  return YGM_OK;
}
int ygm_sync_step2_shared_v1_device(ygm_ctx* c, const uint8_t* d_states, uint64_t states_bytes, const uint64_t* d_state_off,
                                    uint32_t n_states, const uint8_t* d_sv_arena, const uint64_t* d_sv_off, const uint32_t* d_ask_state,
                                    uint32_t n_asks, void* stream, ygm_device_result* out) {
  return ygm_sync_step2_shared_opts_v1_device(c, d_states, states_bytes, d_state_off, nullptr, n_states, d_sv_arena, d_sv_off, d_ask_state,
                                              n_asks, stream, out);
}

// ------------------------------------------------------------------ update V2 (device API)
// V2 -> V1 of n units (merge: updates, with doc_upd so single-input documents are skipped; otherwise one per
// document): sizes, scan (c->v2_len becomes the V1 offsets, total at [n]), bytes into c->v2_v1
static int v21_pass(ygm_ctx* c, hipStream_t s, const uint8_t* arena, const uint64_t* off, uint32_t n, const uint32_t* doc_upd,
                    uint32_t n_docs, uint32_t mode, uint64_t& total) {
  const size_t nb = ((size_t)n + 1 + 255) / 256 + 2;
  if (!c->v2_len.ensure(8ull * n + 16) || !c->v2_st.ensure(4ull * n + 4) || !c->v2_bs.ensure(8 * nb) || !c->v21_cl.ensure((size_t)n + 16))
    return YGM_ENOMEM;
  // the register-resident transcoder first (claims), the general one for the rest; the public conversion: general only
  uint8_t* cl = (mode & 1u) || getenv("YGM_V21_NOFAST") ? nullptr : c->v21_cl.as<uint8_t>();
  total = 0;
  if (n == 0) { HIPCHK(hipMemsetAsync(c->v2_len.p, 0, 8, s)); }
  else {
    if (ygm_k_launch_v21(0, arena, off, n, doc_upd, n_docs, mode, c->flags, c->v2_len.as<uint64_t>(), c->v2_st.as<int32_t>(), nullptr, cl, s) ||
        ygm_k_launch_scan(c->v2_len.as<uint64_t>(), n, c->v2_bs.as<uint64_t>(), s))
      return YGM_EDEVICE;
    int e = 0;
    total = read_u64(c, s, c->v2_len.as<uint64_t>() + n, e);
    if (e) return e;
  }
  if (!c->v2_v1.ensure(total + 64)) return YGM_ENOMEM;   // (the V1 kernels read up to 64 bytes past the arena)
  if (n && ygm_k_launch_v21(1, arena, off, n, doc_upd, n_docs, mode, c->flags, c->v2_len.as<uint64_t>(), c->v2_st.as<int32_t>(),
                            c->v2_v1.as<uint8_t>(), cl, s))
    return YGM_EDEVICE;
  return YGM_OK;
}
// V1 -> V2 per document with final statuses.  Documents in the fast encoder's shape (ygm_v2_fast.hpp) are done by
// k_v12_fast into slots of c->v2_out placed from slot_off (the V2 input offsets: merge_slot of the document's input
// bytes); the rest take k_v12_count / scan / k_v12_write, packed after the slot region.  slot_off == nullptr (the
// public conversion): the general kernels only.
static int v12_pass(ygm_ctx* c, hipStream_t s, const uint8_t* v1, const uint64_t* v1_off, const uint64_t* v1_len, const int32_t* v1_st,
                    const uint8_t* v2a, uint64_t v2n, const uint64_t* upd_off, const uint32_t* doc_upd, const int32_t* ust, uint32_t n_docs,
                    uint32_t mode, const uint64_t* slot_off, ygm_device_result* out) {
  const size_t nb = ((size_t)n_docs + 1 + 255) / 256 + 2;
  if (!c->v2_L.ensure(4ull * ygm_k_v2_cols() * n_docs + 16) || !c->v2_off.ensure(8ull * n_docs + 16) || !c->v2_olen.ensure(8ull * n_docs + 8) ||
      !c->v2_ost.ensure(4ull * n_docs + 4) || !c->v2_bs.ensure(8 * nb) || !c->v2_fo.ensure(8ull * n_docs + 8) ||
      !c->v2_claim.ensure((size_t)n_docs + 16) || !c->v2_pay.ensure(16))
    return YGM_ENOMEM;
  const bool fast = slot_off != nullptr && !(mode & 1u) && getenv("YGM_V2_NOFAST") == nullptr;
  const uint64_t slot_total = fast ? 2 * v2n + 64ull * n_docs : 0;
  uint8_t* claim = fast ? c->v2_claim.as<uint8_t>() : nullptr;
  uint64_t total = 0, fast_bytes = 0, fast_docs = 0;
  if (fast && n_docs) {
    if (!c->v2_out.ensure(slot_total + 64) || !c->v2_scr.ensure(ygm_k_v12_fast_scratch())) return YGM_ENOMEM;
    HIPCHK(hipMemsetAsync(c->v2_pay.p, 0, 16, s));
    if (ygm_k_launch_v12_fast(v1, v1_off, v1_len, v1_st, slot_off, doc_upd, ust, n_docs, c->v2_out.as<uint8_t>(), c->v2_fo.as<uint64_t>(),
                              c->v2_olen.as<uint64_t>(), c->v2_ost.as<int32_t>(), claim, c->v2_pay.as<unsigned long long>(),
                              c->v2_scr.as<uint8_t>(), slot_total, s))
      return YGM_EDEVICE;
    uint64_t pay[2];
    const int e = read_u64_pair(c, s, c->v2_pay.as<uint64_t>(), pay);
    if (e) return e;
    fast_bytes = pay[0]; fast_docs = pay[1];
  }
  if (fast && fast_docs == n_docs) {   // every document done by the fast encoder: no general pass
    out->data = c->v2_out.as<uint8_t>(); out->off = c->v2_fo.as<uint64_t>(); out->len = c->v2_olen.as<uint64_t>();
    out->status = c->v2_ost.as<int32_t>(); out->data_bytes = slot_total; out->payload_bytes = fast_bytes;
    return YGM_OK;
  }
  if (n_docs) {
    if (ygm_k_launch_v12_count(v1, v1_off, v1_len, v1_st, v2a, v2n, upd_off, doc_upd, ust, n_docs, mode, c->flags, c->v2_L.as<uint32_t>(),
                               c->v2_off.as<uint64_t>(), c->v2_ost.as<int32_t>(), claim, s) ||
        ygm_k_launch_scan(c->v2_off.as<uint64_t>(), n_docs, c->v2_bs.as<uint64_t>(), s))
      return YGM_EDEVICE;
    int e = 0;
    total = read_u64(c, s, c->v2_off.as<uint64_t>() + n_docs, e);
    if (e) return e;
  }
  if (!c->v2_out.ensure(slot_total + total + 64, slot_total, s)) return YGM_ENOMEM;
  if (n_docs && ygm_k_launch_v12_write(v1, v1_off, v1_len, v2a, v2n, upd_off, doc_upd, n_docs, mode, c->flags, c->v2_L.as<uint32_t>(),
                                       c->v2_off.as<uint64_t>(), c->v2_ost.as<int32_t>(), c->v2_out.as<uint8_t>(), c->v2_olen.as<uint64_t>(),
                                       claim, slot_total, c->v2_fo.as<uint64_t>(), s))
    return YGM_EDEVICE;
  out->data = c->v2_out.as<uint8_t>(); out->off = c->v2_fo.as<uint64_t>(); out->len = c->v2_olen.as<uint64_t>();
  out->status = c->v2_ost.as<int32_t>(); out->data_bytes = slot_total + total; out->payload_bytes = total + fast_bytes;
  return YGM_OK;
}
static const uint32_t V2_EXPORT = 1u, V2_STRUCTS_ONLY = 2u;

// the span of a V2 call's own kernels (the V1 operation inside times itself)
struct V2Timer {
  ygm_ctx* c; hipStream_t s; float pre = 0;
  V2Timer(ygm_ctx* c_, hipStream_t s_) : c(c_), s(s_) { (void)hipEventRecord(c->e2, s); }
  void split() { (void)hipEventRecord(c->e3, s); (void)hipEventSynchronize(c->e3); float ms = 0; if (hipEventElapsedTime(&ms, c->e2, c->e3) == hipSuccess) pre += ms; }
  void resume() { (void)hipEventRecord(c->e2, s); }
  void done() { split(); c->stats.kernel_ms += pre; }
};

int ygm_merge_v2_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_upd_off, const uint32_t* d_doc_upd,
                        uint32_t n_upd, uint32_t n_docs, void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  V2Timer T(c, s);
  uint64_t v1_bytes = 0;
  int e = v21_pass(c, s, d_arena, d_upd_off, n_upd, d_doc_upd, n_docs, 0, v1_bytes);
  if (e) return e;
  T.split();
  ygm_device_result r1;
  if ((e = ygm_merge_v1_device(c, c->v2_v1.as<uint8_t>(), v1_bytes, c->v2_len.as<uint64_t>(), d_doc_upd, n_upd, n_docs, s, &r1))) return e;
  T.resume();
  e = v12_pass(c, s, r1.data, r1.off, r1.len, r1.status, d_arena, arena_bytes, d_upd_off, d_doc_upd, c->v2_st.as<int32_t>(), n_docs, 0, d_upd_off, out);
  T.done();
  return e;
}
int ygm_diff_v2_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off, const uint8_t* d_sv_arena,
                       const uint64_t* d_sv_off, uint32_t n_docs, void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  V2Timer T(c, s);
  uint64_t v1_bytes = 0;
  int e = v21_pass(c, s, d_arena, d_doc_off, n_docs, nullptr, n_docs, 0, v1_bytes);
  if (e) return e;
  T.split();
  ygm_device_result r1;
  if ((e = ygm_diff_v1_device(c, c->v2_v1.as<uint8_t>(), v1_bytes, c->v2_len.as<uint64_t>(), d_sv_arena, d_sv_off, n_docs, s, &r1))) return e;
  T.resume();
  e = v12_pass(c, s, r1.data, r1.off, r1.len, r1.status, d_arena, arena_bytes, nullptr, nullptr, c->v2_st.as<int32_t>(), n_docs, 0, d_doc_off, out);
  T.done();
  return e;
}
int ygm_sv_from_update_v2_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off, uint32_t n_docs,
                                 void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  (void)arena_bytes;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  V2Timer T(c, s);
  uint64_t v1_bytes = 0;
  int e = v21_pass(c, s, d_arena, d_doc_off, n_docs, nullptr, n_docs, V2_STRUCTS_ONLY, v1_bytes);
  if (e) return e;
  T.split();
  if ((e = ygm_sv_from_update_v1_device(c, c->v2_v1.as<uint8_t>(), v1_bytes, c->v2_len.as<uint64_t>(), n_docs, s, out))) return e;
  T.resume();
  if (ygm_k_launch_v2_status(c->v2_st.as<int32_t>(), n_docs, out->status, out->len, s)) return YGM_EDEVICE;
  T.done();
  return YGM_OK;
}
int ygm_convert_v1_to_v2_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off, uint32_t n_docs,
                                void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  (void)arena_bytes;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  V2Timer T(c, s);
  const int e = v12_pass(c, s, d_arena, d_doc_off, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, n_docs, V2_EXPORT, nullptr, out);
  T.done();
  if (!e) { c->stats.calls++; c->stats.docs += n_docs; }
  return e;
}
int ygm_convert_v2_to_v1_device(ygm_ctx* c, const uint8_t* d_arena, uint64_t arena_bytes, const uint64_t* d_doc_off, uint32_t n_docs,
                                void* stream, ygm_device_result* out) {
  if (!c || !out) return YGM_EINVAL;
  (void)arena_bytes;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  (void)hipSetDevice(c->device);
  V2Timer T(c, s);
  uint64_t v1_bytes = 0;
  int e = v21_pass(c, s, d_arena, d_doc_off, n_docs, nullptr, n_docs, V2_EXPORT, v1_bytes);
  if (e) return e;
  if (!c->v2_olen.ensure(8ull * n_docs + 8)) return YGM_ENOMEM;
  if (ygm_k_launch_v2_lens(c->v2_len.as<uint64_t>(), c->v2_st.as<int32_t>(), n_docs, c->v2_olen.as<uint64_t>(), s)) return YGM_EDEVICE;
  T.done();
  c->stats.calls++; c->stats.docs += n_docs;
  out->data = c->v2_v1.as<uint8_t>(); out->off = c->v2_len.as<uint64_t>(); out->len = c->v2_olen.as<uint64_t>();
  out->status = c->v2_st.as<int32_t>(); out->data_bytes = v1_bytes; out->payload_bytes = v1_bytes;
  return YGM_OK;
}

// ------------------------------------------------------------------ host API
// A batch is cut into chunks (about YGM_CHUNK_BYTES of input each; the planners are in ygm_chunks.hpp) that alternate
// between two stage contexts, each with its own stream and device buffers.  run_pipeline drives three parts:
//   stage:  host arenas -> pinned staging (CPU copy) -> H2D               (chunk i + 1, stream of stage (i + 1) % 2)
//   run:    the operation's device entry point on the staged chunk (OPS)  (chunk i, stream of stage i % 2)
//   drain:  device-side packing of the outputs -> D2H                     (chunk i, same stream)
// so the CPU copy and the H2D of one chunk overlap the kernels of the previous one, and the D2H moves
// only the packed outputs (not the per-document slots).  h2d_ms / d2h_ms are the copies' HIP-event
// times (summed over chunks); the results live in the parent context's pinned buffers.
static const uint64_t YGM_CHUNK_BYTES = 64ull << 20;
// A batch of large [snapshot, ...log] documents runs the large-document tier once per chunk, each run as long as its
// largest document: a third of the batch per chunk (at least 64 MB) keeps the copies overlapped and the tier's runs
// few (tools/host_probe.py, profiles/r06_final/host_chunks.jsonl).  YGM_CHUNK_MB overrides (experiments).
static uint64_t chunk_bytes(uint64_t in_bytes) {
  const char* e = getenv("YGM_CHUNK_MB");
  if (e && atoi(e) > 0) return (uint64_t)atoi(e) << 20;
  return in_bytes / 3 > YGM_CHUNK_BYTES ? in_bytes / 3 : YGM_CHUNK_BYTES;
}

namespace {
// The host API's operations; OPS below holds one row per operation, in this order.
enum class Op : uint8_t {
  Sv, Diff, Merge, Snapshot, Contains, MergeV2, DiffV2, SvV2, V1ToV2, V2ToV1, Step2, DiffShared, Step2Shared, VersionTake,
  VersionRestore, VersionRestoreShared, Text, Json, JsonFields, ToJson, Count
};
enum class Primary : uint8_t { Docs, Updates, States };   // what the first arena's offsets count
enum class OptOf : uint8_t { None, Doc, State, Ask };     // whose option bytes travel with a chunk

struct HostCall {
  Op op;
  const uint8_t* arena; const uint64_t* off; uint32_t n_pri;   // primary inputs: documents, a merge's updates, shared states
  uint32_t n_res;                                               // results: documents, or the asks of a shared call
  const uint32_t* link = nullptr;   // merge: each update's document; shared: each ask's state
  const uint8_t* arena2 = nullptr; const uint64_t* off2 = nullptr;   // the second arena, one entry per result (OpRow::second)
  const uint8_t* opt = nullptr;     // option bytes (OpRow::opt says whose), null: none; each chunk stages its slice
  uint32_t text_mode = 0;           // Op::Text: YGM_TEXT_FLAT / YGM_TEXT_DEEP; Op::Json, Op::JsonFields, Op::ToJson: the kind
};
// a chunk's inputs on its stage context, as the device entry points take them
struct Staged {
  const uint8_t* arena; uint64_t bytes; const uint64_t* off; uint32_t n_pri, n_res;
  const uint8_t* arena2; const uint64_t* off2;
  const uint32_t* link;   // merge: the documents' update ranges (n_res + 1); shared: each ask's state, relative to the chunk
  const uint8_t* opt;     // null: no options
  uint32_t text_mode;
};
struct Chunk : ygm::ChunkRange {
  Staged in{};                     // filled by stage
  uint64_t pos = 0, payload = 0;   // packed output position in the parent's result, bytes
  hipEvent_t h0 = nullptr, h1 = nullptr, o0 = nullptr, o1 = nullptr;   // around the H2D / the D2H copies
};
struct OpRow {
  Op op;
  Primary primary;
  bool second;    // a second arena per result (diff: state vectors, contains: updates, restore: versions, text / json: root names, json fields: field lists)
  OptOf opt;
  int (*run)(ygm_ctx* k, const Staged& S, ygm_device_result* dr);   // the staged chunk on stage context k
  int (*enqueue)(ygm_ctx* k, const Staged& S);   // device work enqueued before the next chunk is staged (null: none)
};

static int run_sv(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_sv_from_update_v1_device(k, S.arena, S.bytes, S.off, S.n_res, nullptr, dr);
}
static int run_diff(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_diff_v1_device(k, S.arena, S.bytes, S.off, S.arena2, S.off2, S.n_res, nullptr, dr);
}
// (the lean kernel of chunk i runs while chunk i + 1 is staged)
static int enqueue_merge(ygm_ctx* k, const Staged& S) {
  return ygm_merge_v1_device_async(k, S.arena, S.bytes, S.off, S.link, S.n_pri, S.n_res, nullptr);
}
static int run_merge(ygm_ctx* k, const Staged&, ygm_device_result* dr) { return ygm_merge_v1_device_finish(k, dr); }
static int run_snapshot(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_snapshot_opts_v1_device(k, S.arena, S.bytes, S.off, S.opt, S.n_res, nullptr, dr);
}
static int run_contains(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_contains_v1_device(k, S.arena, S.off, S.arena2, S.off2, S.n_res, nullptr, dr);
}
static int run_merge_v2(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_merge_v2_device(k, S.arena, S.bytes, S.off, S.link, S.n_pri, S.n_res, nullptr, dr);
}
static int run_diff_v2(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_diff_v2_device(k, S.arena, S.bytes, S.off, S.arena2, S.off2, S.n_res, nullptr, dr);
}
static int run_sv_v2(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_sv_from_update_v2_device(k, S.arena, S.bytes, S.off, S.n_res, nullptr, dr);
}
static int run_v1_to_v2(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_convert_v1_to_v2_device(k, S.arena, S.bytes, S.off, S.n_res, nullptr, dr);
}
static int run_v2_to_v1(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_convert_v2_to_v1_device(k, S.arena, S.bytes, S.off, S.n_res, nullptr, dr);
}
static int run_step2(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_sync_step2_opts_v1_device(k, S.arena, S.bytes, S.off, S.opt, S.arena2, S.off2, S.n_res, nullptr, dr);
}
static int run_diff_shared(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_diff_shared_v1_device(k, S.arena, S.bytes, S.off, S.n_pri, S.arena2, S.off2, S.link, S.n_res, nullptr, dr);
}
static int run_step2_shared(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_sync_step2_shared_opts_v1_device(k, S.arena, S.bytes, S.off, S.opt, S.n_pri, S.arena2, S.off2, S.link, S.n_res, nullptr, dr);
}
static int run_version_take(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_version_take_v1_device(k, S.arena, S.bytes, S.off, S.n_res, nullptr, dr);
}
static int run_version_restore(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_version_restore_v1_device(k, S.arena, S.off, S.arena2, S.off2, S.opt, S.n_res, nullptr, dr);
}
static int run_version_restore_shared(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_version_restore_shared_v1_device(k, S.arena, S.bytes, S.off, S.n_pri, S.arena2, S.off2, S.link, S.opt, S.n_res, nullptr, dr);
}
static int run_text(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_text_v1_device(k, S.arena, S.bytes, S.off, S.arena2, S.off2, S.text_mode, S.n_res, nullptr, dr);
}

static int run_json(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_json_v1_device(k, S.arena, S.bytes, S.off, S.arena2, S.off2, S.text_mode, S.n_res, nullptr, dr);
}
static int run_json_fields(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_json_fields_v1_device(k, S.arena, S.bytes, S.off, S.arena2, S.off2, S.text_mode, S.n_res, nullptr, dr);
}
static int run_tojson(ygm_ctx* k, const Staged& S, ygm_device_result* dr) {
  return ygm_tojson_v1_device(k, S.arena, S.bytes, S.off, S.arena2, S.off2, S.text_mode, S.n_res, nullptr, dr);
}

constexpr OpRow OPS[] = {
    {Op::Sv, Primary::Docs, false, OptOf::None, run_sv, nullptr},
    {Op::Diff, Primary::Docs, true, OptOf::None, run_diff, nullptr},
    {Op::Merge, Primary::Updates, false, OptOf::None, run_merge, enqueue_merge},
    {Op::Snapshot, Primary::Docs, false, OptOf::Doc, run_snapshot, nullptr},
    {Op::Contains, Primary::Docs, true, OptOf::None, run_contains, nullptr},
    {Op::MergeV2, Primary::Updates, false, OptOf::None, run_merge_v2, nullptr},
    {Op::DiffV2, Primary::Docs, true, OptOf::None, run_diff_v2, nullptr},
    {Op::SvV2, Primary::Docs, false, OptOf::None, run_sv_v2, nullptr},
    {Op::V1ToV2, Primary::Docs, false, OptOf::None, run_v1_to_v2, nullptr},
    {Op::V2ToV1, Primary::Docs, false, OptOf::None, run_v2_to_v1, nullptr},
    {Op::Step2, Primary::Docs, true, OptOf::Doc, run_step2, nullptr},
    {Op::DiffShared, Primary::States, true, OptOf::None, run_diff_shared, nullptr},
    {Op::Step2Shared, Primary::States, true, OptOf::State, run_step2_shared, nullptr},
    {Op::VersionTake, Primary::Docs, false, OptOf::None, run_version_take, nullptr},
    {Op::VersionRestore, Primary::Docs, true, OptOf::Doc, run_version_restore, nullptr},
    {Op::VersionRestoreShared, Primary::States, true, OptOf::Ask, run_version_restore_shared, nullptr},
    {Op::Text, Primary::Docs, true, OptOf::None, run_text, nullptr},
    {Op::Json, Primary::Docs, true, OptOf::None, run_json, nullptr},
    {Op::JsonFields, Primary::Docs, true, OptOf::None, run_json_fields, nullptr},
    {Op::ToJson, Primary::Docs, true, OptOf::None, run_tojson, nullptr},
};
constexpr bool ops_in_order() {
  for (size_t i = 0; i < sizeof(OPS) / sizeof(OPS[0]); i++) if (OPS[i].op != (Op)i) return false;
  return true;
}
static_assert(sizeof(OPS) / sizeof(OPS[0]) == (size_t)Op::Count && ops_in_order(), "one row per operation, in the enum's order");
extern "C++" constexpr const OpRow& row(Op op) { return OPS[(size_t)op]; }
}  // namespace

static int stage_ctx(ygm_ctx* c, int i, ygm_ctx** out) {
  if (!c->kid[i]) { int e = ygm_open(c->device, c->flags, &c->kid[i]); if (e) return e; }
  *out = c->kid[i];
  return YGM_OK;
}

// large host copies split over threads (one core copies ~10 GB/s; PCIe takes ~55 GB/s)
static void par_memcpy(uint8_t* dst, const uint8_t* src, size_t n) {
  const size_t per = 8u << 20;
  unsigned t = (unsigned)std::min<size_t>((n + per - 1) / per, 8);
  const unsigned hw = std::thread::hardware_concurrency();
  if (hw && t > hw) t = hw;
  if (t <= 1) { memcpy(dst, src, n); return; }
  std::vector<std::thread> th;
  const size_t part = (n + t - 1) / t;
  for (unsigned i = 1; i < t; i++) {
    const size_t a = i * part, b = std::min(n, a + part);
    if (a < b) th.emplace_back([=] { memcpy(dst + a, src + a, b - a); });
  }
  memcpy(dst, src, std::min(n, part));
  for (auto& x : th) x.join();
}

// f(begin, end) over [0, n) split over threads when n is large
extern "C++" template <class F>
static void par_for(size_t n, F f) {
  const size_t per = 1u << 20;
  unsigned t = (unsigned)std::min<size_t>((n + per - 1) / per, 8);
  const unsigned hw = std::thread::hardware_concurrency();
  if (hw && t > hw) t = hw;
  if (t <= 1) { f((size_t)0, n); return; }
  std::vector<std::thread> th;
  const size_t part = (n + t - 1) / t;
  for (unsigned i = 1; i < t; i++) {
    const size_t a = i * part, b = std::min(n, a + part);
    if (a < b) th.emplace_back([=] { f(a, b); });
  }
  f((size_t)0, std::min(n, part));
  for (auto& x : th) x.join();
}

// a staged arena: its bytes, 64 readable zero bytes after them, a multiple of 16
static uint64_t staged_bytes(uint64_t n) { return (n + 64 + 15) & ~15ull; }
static void rebase(uint64_t* dst, const uint64_t* src, uint64_t n, uint64_t base) {
  par_for(n, [=](size_t a, size_t b) { for (size_t j = a; j < b; j++) dst[j] = src[j] - base; });
}

// stage: CPU copy of a chunk's inputs into the stage's pinned buffer -- [arena | offsets | second arena | its offsets |
// link table | option bytes] -- then one async H2D copy per part; C.in is what the run function reads
static int stage(ygm_ctx* k, const HostCall& H, Chunk& C) {
  const OpRow& R = row(H.op);
  const uint32_t n_res = C.r1 - C.r0, n_pri = C.p1 - C.p0;
  const uint64_t a0 = H.off[C.p0], bytes = H.off[C.p1] - a0, ab = staged_bytes(bytes);
  const uint64_t s0 = R.second ? H.off2[C.r0] : 0, sbytes = R.second ? H.off2[C.r1] - s0 : 0, sb = R.second ? staged_bytes(sbytes) : 0;
  const uint64_t n_off = (uint64_t)n_pri + 1, n_off2 = R.second ? (uint64_t)n_res + 1 : 0;
  const uint64_t n_link = R.primary == Primary::Updates ? (uint64_t)n_res + 1 : R.primary == Primary::States ? n_res : 0;
  // a shared state's option byte travels in each of its chunks; the version restore's belong to the restored documents
  const uint64_t n_opt = !H.opt || R.opt == OptOf::None ? 0 : R.opt == OptOf::State ? n_pri : n_res;
  if (!k->h_in.ensure(ab + 8 * n_off + sb + 8 * n_off2 + 4 * n_link + n_opt + 64)) return YGM_ENOMEM;
  uint8_t* P = k->h_in.as<uint8_t>();
  uint64_t* ro = (uint64_t*)(P + ab);
  uint8_t* q = (uint8_t*)(ro + n_off);
  uint64_t* ro2 = (uint64_t*)(q + sb);
  uint32_t* lk = (uint32_t*)(ro2 + n_off2);
  uint8_t* po = (uint8_t*)(lk + n_link);
  if (bytes) par_memcpy(P, H.arena + a0, bytes);
  memset(P + bytes, 0, ab - bytes);
  rebase(ro, H.off + C.p0, n_off, a0);
  if (R.second) {
    if (sbytes) memcpy(q, H.arena2 + s0, sbytes);
    memset(q + sbytes, 0, sb - sbytes);
    rebase(ro2, H.off2 + C.r0, n_off2, s0);
  }
  if (R.primary == Primary::Updates) {   // per-document update ranges, relative to the chunk (one walk over its updates: a
                                         // binary search per document measured 2-3x slower end to end, tools/host_probe.py)
    lk[0] = 0;
    uint32_t u = C.p0;
    for (uint32_t d = 0; d < n_res; d++) { while (u < C.p1 && H.link[u] == C.r0 + d) u++; lk[d + 1] = u - C.p0; }
  } else if (R.primary == Primary::States) {
    for (uint32_t j = 0; j < n_res; j++) lk[j] = H.link[C.r0 + j] - C.p0;
  }
  if (n_opt) memcpy(po, H.opt + (R.opt == OptOf::State ? C.p0 : C.r0), n_opt);
  if (!k->arena.ensure(ab) || !k->offs.ensure(8 * n_off) || (R.second && (!k->sv_arena.ensure(sb) || !k->sv_offs.ensure(8 * n_off2))) ||
      (R.primary != Primary::Docs && !k->docs.ensure(4 * n_link + 4)) || (n_opt && !k->opt.ensure(n_opt)))
    return YGM_ENOMEM;
  hipStream_t s = k->stream;
  HIPCHK(hipEventRecord(C.h0, s));
  HIPCHK(hipMemcpyAsync(k->arena.p, P, ab, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(k->offs.p, ro, 8 * n_off, hipMemcpyHostToDevice, s));
  if (R.second) {
    HIPCHK(hipMemcpyAsync(k->sv_arena.p, q, sb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(k->sv_offs.p, ro2, 8 * n_off2, hipMemcpyHostToDevice, s));
  }
  if (n_link) HIPCHK(hipMemcpyAsync(k->docs.p, lk, 4 * n_link, hipMemcpyHostToDevice, s));
  if (n_opt) HIPCHK(hipMemcpyAsync(k->opt.p, po, n_opt, hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(C.h1, s));
  C.in = Staged{k->arena.as<uint8_t>(), bytes, k->offs.as<uint64_t>(), n_pri, n_res, k->sv_arena.as<uint8_t>(), k->sv_offs.as<uint64_t>(),
                k->docs.as<uint32_t>(), n_opt ? k->opt.as<uint8_t>() : nullptr, H.text_mode};
  return YGM_OK;
}

// drain: device-side packing of a chunk's results, and the async D2H into the parent's pinned results at `pos`
static int drain(ygm_ctx* c, ygm_ctx* k, Chunk& C, const ygm_device_result& dr, uint64_t& pos) {
  const uint32_t n = C.r1 - C.r0, nb = (n + 255) / 256;
  if (!k->pk_data.ensure(dr.payload_bytes + 64) || !k->pk_off.ensure(8ull * n + 8) || !k->pk_bsum.ensure(8ull * nb + 16)) return YGM_ENOMEM;
  if (n && ygm_k_launch_pack(dr.data, dr.off, dr.len, dr.status, n, k->pk_bsum.as<uint64_t>(), k->pk_data.as<uint8_t>(),
                             k->pk_off.as<uint64_t>(), k->stream))
    return YGM_EDEVICE;
  C.pos = pos; C.payload = dr.payload_bytes;
  if (pos + dr.payload_bytes + 1 > c->h_data.cap) {   // regrowth moves the bytes copied so far: let those copies land first
    for (ygm_ctx* x : c->kid) if (x) HIPCHK(hipStreamSynchronize(x->stream));
    if (!c->h_data.ensure(pos + dr.payload_bytes + 1, pos)) return YGM_ENOMEM;
  }
  HIPCHK(hipEventRecord(C.o0, k->stream));
  if (dr.payload_bytes) HIPCHK(hipMemcpyAsync(c->h_data.as<uint8_t>() + pos, k->pk_data.p, dr.payload_bytes, hipMemcpyDeviceToHost, k->stream));
  if (n) {
    HIPCHK(hipMemcpyAsync(c->h_off.as<uint64_t>() + C.r0, k->pk_off.p, 8ull * n, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(hipMemcpyAsync(c->h_len.as<uint64_t>() + C.r0, dr.len, 8ull * n, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(hipMemcpyAsync(c->h_status.as<int32_t>() + C.r0, dr.status, 4ull * n, hipMemcpyDeviceToHost, k->stream));
  }
  HIPCHK(hipEventRecord(C.o1, k->stream));
  pos += dr.payload_bytes;
  return YGM_OK;
}

// device work of a stage context since `b`, into the parent context's counters
static void add_stage_stats(ygm_ctx* c, const ygm_stats_t& a, const ygm_stats_t& b) {
  c->stats.calls += a.calls - b.calls; c->stats.docs += a.docs - b.docs; c->stats.updates += a.updates - b.updates;
  c->stats.bytes_in += a.bytes_in - b.bytes_in; c->stats.bytes_out += a.bytes_out - b.bytes_out;
  c->stats.docs_fast += a.docs_fast - b.docs_fast; c->stats.docs_seq += a.docs_seq - b.docs_seq;
  c->stats.kernel_ms += a.kernel_ms - b.kernel_ms; c->stats.docs_lean += a.docs_lean - b.docs_lean;
  c->stats.lean_ms += a.lean_ms - b.lean_ms; c->stats.lean_launches += a.lean_launches - b.lean_launches;
  c->stats.docs_big += a.docs_big - b.docs_big; c->stats.docs_lean_wide += a.docs_lean_wide - b.docs_lean_wide;
  c->stats.host_syncs += a.host_syncs - b.host_syncs;
  c->stats.docs_pending += a.docs_pending - b.docs_pending;
  c->stats.docs_snapshot += a.docs_snapshot - b.docs_snapshot;
}

// The driver: the planned chunks, double-buffered over the two stage contexts, into the parent's pinned results.
// out_hint sizes the pinned result at first (outputs are usually no larger than the inputs; grown when a chunk needs more)
static int run_pipeline(ygm_ctx* c, const HostCall& H, const std::vector<ygm::ChunkRange>& plan, uint64_t out_hint, ygm_result* out) {
  (void)hipSetDevice(c->device);
  const OpRow& R = row(H.op);
  const uint32_t n = H.n_res;
  if (!c->h_off.ensure(8ull * n + 8) || !c->h_len.ensure(8ull * n + 8) || !c->h_status.ensure(4ull * n + 4) ||
      !c->h_data.ensure(out_hint + 16ull * n + 4096))
    return YGM_ENOMEM;
  std::vector<Chunk> ch(plan.size());
  for (size_t i = 0; i < ch.size(); i++) static_cast<ygm::ChunkRange&>(ch[i]) = plan[i];
  int e = YGM_OK;
  const int nk = ch.size() > 1 ? 2 : 1;
  ygm_ctx* k[2] = {nullptr, nullptr};
  for (int j = 0; j < nk; j++) if ((e = stage_ctx(c, j, &k[j]))) return e;
  for (Chunk& C : ch)
    if (hipEventCreate(&C.h0) != hipSuccess || hipEventCreate(&C.h1) != hipSuccess || hipEventCreate(&C.o0) != hipSuccess ||
        hipEventCreate(&C.o1) != hipSuccess) { e = YGM_EDEVICE; break; }
  ygm_stats_t s0[2] = {k[0]->stats, nk > 1 ? k[1]->stats : ygm_stats_t{}};
  uint64_t pos = 0;
  if (!e) e = stage(k[0], H, ch[0]);
  for (size_t i = 0; i < ch.size() && !e; i++) {
    ygm_ctx* ki = k[i & 1];
    if (R.enqueue && (e = R.enqueue(ki, ch[i].in))) break;
    // the next stage's previous chunk (i - 1) has left its pinned staging (its kernels have run)
    if (i + 1 < ch.size() && (e = stage(k[(i + 1) & 1], H, ch[i + 1]))) break;
    ygm_device_result dr;
    if ((e = R.run(ki, ch[i].in, &dr))) break;
    e = drain(c, ki, ch[i], dr, pos);
  }
  for (int j = 0; j < nk; j++) if (hipStreamSynchronize(k[j]->stream) != hipSuccess && !e) e = YGM_EDEVICE;
  if (!e) {
    float ms = 0;
    for (Chunk& C : ch) {
      if (hipEventElapsedTime(&ms, C.h0, C.h1) == hipSuccess) c->stats.h2d_ms += ms;
      if (hipEventElapsedTime(&ms, C.o0, C.o1) == hipSuccess) c->stats.d2h_ms += ms;
      uint64_t* off = c->h_off.as<uint64_t>() + C.r0;
      for (uint32_t d = 0; d < C.r1 - C.r0; d++) off[d] += C.pos;
    }
    for (int j = 0; j < nk; j++) add_stage_stats(c, k[j]->stats, s0[j]);
    int32_t* st = c->h_status.as<int32_t>();
    uint64_t* ln = c->h_len.as<uint64_t>();
    for (uint32_t d = 0; d < n; d++) {
      if (st[d] >= 100 || st[d] < 0) st[d] = YGM_EDEVICE;   // never leaves internal codes
      if (st[d] != YGM_OK) ln[d] = 0;
    }
    out->data = c->h_data.as<uint8_t>(); out->off = c->h_off.as<uint64_t>(); out->len = ln; out->status = st;
    out->n_docs = n; out->data_bytes = pos;
  }
  for (Chunk& C : ch) for (hipEvent_t ev : {C.h0, C.h1, C.o0, C.o1}) if (ev) (void)hipEventDestroy(ev);
  return e;
}

static const uint64_t ZERO_OFF[1] = {0};   // the offsets of an empty batch

// chunks of whole documents (H.off: the documents', or a merge's updates' offsets)
static int host_call(ygm_ctx* c, const HostCall& H, ygm_result* out) {
  const uint64_t in_bytes = H.off[H.n_pri] - H.off[0];
  return run_pipeline(c, H, ygm::plan_doc_chunks(H.off, H.n_res, row(H.op).primary == Primary::Updates, H.link, H.n_pri, chunk_bytes(in_bytes)),
                      in_bytes, out);
}

// shared states: n_docs states, n_asks asks (ask_doc non-decreasing), results and the second arena indexed by ask
static int host_shared_call(ygm_ctx* c, Op op, const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, const uint8_t* sv_arena,
                            const uint64_t* sv_off, const uint32_t* ask_doc, uint32_t n_asks, ygm_result* out, const uint8_t* opt = nullptr) {
  if (!c || !out || (n_docs && !doc_off) || (n_asks && (!sv_off || !ask_doc))) return YGM_EINVAL;
  for (uint32_t d = 0; d < n_docs; d++) if (doc_off[d + 1] < doc_off[d]) return YGM_EINVAL;
  for (uint32_t a = 0; a < n_asks; a++)
    if (ask_doc[a] >= n_docs || (a && ask_doc[a] < ask_doc[a - 1]) || sv_off[a + 1] < sv_off[a]) return YGM_EINVAL;
  if ((n_docs && doc_off[n_docs] > doc_off[0] && !arena) || (n_asks && sv_off[n_asks] > sv_off[0] && !sv_arena)) return YGM_EINVAL;
  HostCall H{op, arena, n_docs ? doc_off : ZERO_OFF, n_docs, n_asks, ask_doc, sv_arena, n_asks ? sv_off : ZERO_OFF, opt};
  uint64_t vbytes = H.off[n_docs] - H.off[0];   // virtual bytes: the states', plus each ask's state length
  for (uint32_t a = 0; a < n_asks; a++) vbytes += doc_off[ask_doc[a] + 1] - doc_off[ask_doc[a]];
  return run_pipeline(c, H, ygm::plan_shared_chunks(H.off, n_docs, ask_doc, n_asks, chunk_bytes(vbytes)), std::min<uint64_t>(vbytes, 1ull << 30),
                      out);
}

static int host_merge_call(ygm_ctx* c, Op op, const uint8_t* arena, const uint64_t* upd_off, const uint32_t* upd_doc, uint32_t n_upd,
                           uint32_t n_docs, ygm_result* out) {
  if (!c || !out || (n_upd && (!arena || !upd_off || !upd_doc))) return YGM_EINVAL;
  // document ids non-decreasing, offsets non-decreasing
  std::atomic<int> bad{0};
  par_for(n_upd, [&](size_t a, size_t b) {
    for (size_t i = a; i < b; i++)
      if (upd_doc[i] >= n_docs || (i && upd_doc[i] < upd_doc[i - 1]) || upd_off[i + 1] < upd_off[i]) { bad = 1; return; }
  });
  if (bad) return YGM_EINVAL;
  HostCall H{op, arena, n_upd ? upd_off : ZERO_OFF, n_upd, n_docs, upd_doc};
  return host_call(c, H, out);
}

static int host_doc_call(ygm_ctx* c, Op op, const uint8_t* arena, const uint64_t* doc_off, const uint8_t* arena2, const uint64_t* off2,
                         uint32_t n_docs, ygm_result* out, const uint8_t* opt = nullptr) {
  if (!c || !out || (n_docs && (!arena || !doc_off))) return YGM_EINVAL;
  const bool two = row(op).second;
  if (two && n_docs && (!arena2 || !off2)) return YGM_EINVAL;
  for (uint32_t d = 0; d < n_docs; d++) {
    if (doc_off[d + 1] < doc_off[d]) return YGM_EINVAL;
    if (two && off2[d + 1] < off2[d]) return YGM_EINVAL;
  }
  HostCall H{op, arena, n_docs ? doc_off : ZERO_OFF, n_docs, n_docs, nullptr, arena2, n_docs ? off2 : ZERO_OFF, opt};
  return host_call(c, H, out);
}

int ygm_merge_v1(ygm_ctx* c, const uint8_t* arena, const uint64_t* upd_off, const uint32_t* upd_doc, uint32_t n_upd, uint32_t n_docs,
                 ygm_result* out) {
  return host_merge_call(c, Op::Merge, arena, upd_off, upd_doc, n_upd, n_docs, out);
}
int ygm_merge_v2(ygm_ctx* c, const uint8_t* arena, const uint64_t* upd_off, const uint32_t* upd_doc, uint32_t n_upd, uint32_t n_docs,
                 ygm_result* out) {
  return host_merge_call(c, Op::MergeV2, arena, upd_off, upd_doc, n_upd, n_docs, out);
}
int ygm_sv_from_update_v1(ygm_ctx* c, const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::Sv, arena, doc_off, nullptr, nullptr, n_docs, out);
}
int ygm_diff_v1(ygm_ctx* c, const uint8_t* arena, const uint64_t* doc_off, const uint8_t* sv_arena, const uint64_t* sv_off,
                uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::Diff, arena, doc_off, sv_arena, sv_off, n_docs, out);
}
int ygm_diff_v2(ygm_ctx* c, const uint8_t* arena, const uint64_t* doc_off, const uint8_t* sv_arena, const uint64_t* sv_off,
                uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::DiffV2, arena, doc_off, sv_arena, sv_off, n_docs, out);
}
int ygm_sv_from_update_v2(ygm_ctx* c, const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::SvV2, arena, doc_off, nullptr, nullptr, n_docs, out);
}
int ygm_convert_v1_to_v2(ygm_ctx* c, const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::V1ToV2, arena, doc_off, nullptr, nullptr, n_docs, out);
}
int ygm_convert_v2_to_v1(ygm_ctx* c, const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::V2ToV1, arena, doc_off, nullptr, nullptr, n_docs, out);
}
int ygm_contains_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, const uint8_t* updates, const uint64_t* update_off,
                    uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::Contains, states, state_off, updates, update_off, n_docs, out);
}
int ygm_snapshot_v1(ygm_ctx* c, const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::Snapshot, arena, doc_off, nullptr, nullptr, n_docs, out);
}
int ygm_snapshot_opts_v1(ygm_ctx* c, const uint8_t* arena, const uint64_t* doc_off, const uint8_t* doc_opt, uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::Snapshot, arena, doc_off, nullptr, nullptr, n_docs, out, doc_opt);
}
int ygm_sync_step2_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, const uint8_t* sv_arena, const uint64_t* sv_off,
                      uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::Step2, states, state_off, sv_arena, sv_off, n_docs, out);
}
int ygm_sync_step2_opts_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, const uint8_t* state_opt, const uint8_t* sv_arena,
                           const uint64_t* sv_off, uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::Step2, states, state_off, sv_arena, sv_off, n_docs, out, state_opt);
}
int ygm_version_take_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::VersionTake, states, state_off, nullptr, nullptr, n_docs, out);
}
int ygm_version_restore_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, const uint8_t* versions, const uint64_t* version_off,
                           const uint8_t* restored_opt, uint32_t n_docs, ygm_result* out) {
  return host_doc_call(c, Op::VersionRestore, states, state_off, versions, version_off, n_docs, out, restored_opt);
}
int ygm_text_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, const uint8_t* names, const uint64_t* name_off, uint32_t mode,
                uint32_t n_docs, ygm_result* out) {
  if (!c || !out || mode > YGM_TEXT_DEEP || (n_docs && (!states || !state_off || !name_off))) return YGM_EINVAL;
  for (uint32_t d = 0; d < n_docs; d++) if (state_off[d + 1] < state_off[d] || name_off[d + 1] < name_off[d]) return YGM_EINVAL;
  static const uint8_t no_names[1] = {0};   // (every name empty: the arena may be NULL)
  if (n_docs && !names) { if (name_off[n_docs] != name_off[0]) return YGM_EINVAL; names = no_names; }   // (no byte of it is read)
  HostCall H{Op::Text, states, n_docs ? state_off : ZERO_OFF, n_docs, n_docs, nullptr, names, n_docs ? name_off : ZERO_OFF};
  H.text_mode = mode;
  return host_call(c, H, out);
}

int ygm_json_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, const uint8_t* names, const uint64_t* name_off, uint32_t kind,
                uint32_t n_docs, ygm_result* out) {
  if (!c || !out || kind != YGM_JSON_PROSEMIRROR || (n_docs && (!states || !state_off || !name_off))) return YGM_EINVAL;
  for (uint32_t d = 0; d < n_docs; d++) if (state_off[d + 1] < state_off[d] || name_off[d + 1] < name_off[d]) return YGM_EINVAL;
  static const uint8_t no_names[1] = {0};   // (every name empty: the arena may be NULL)
  if (n_docs && !names) { if (name_off[n_docs] != name_off[0]) return YGM_EINVAL; names = no_names; }   // (no byte of it is read)
  HostCall H{Op::Json, states, n_docs ? state_off : ZERO_OFF, n_docs, n_docs, nullptr, names, n_docs ? name_off : ZERO_OFF};
  H.text_mode = kind;
  return host_call(c, H, out);
}
int ygm_json_fields_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, const uint8_t* fields, const uint64_t* field_off,
                       uint32_t kind, uint32_t n_docs, ygm_result* out) {
  if (!c || !out || kind != YGM_JSON_PROSEMIRROR || (n_docs && (!states || !state_off || !field_off))) return YGM_EINVAL;
  for (uint32_t d = 0; d < n_docs; d++) if (state_off[d + 1] < state_off[d] || field_off[d + 1] < field_off[d]) return YGM_EINVAL;
  static const uint8_t no_fields[1] = {0};   // (every list empty: the arena may be NULL)
  if (n_docs && !fields) { if (field_off[n_docs] != field_off[0]) return YGM_EINVAL; fields = no_fields; }   // (no byte of it is read)
  HostCall H{Op::JsonFields, states, n_docs ? state_off : ZERO_OFF, n_docs, n_docs, nullptr, fields, n_docs ? field_off : ZERO_OFF};
  H.text_mode = kind;
  return host_call(c, H, out);
}
int ygm_tojson_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, const uint8_t* names, const uint64_t* name_off, uint32_t kind,
                  uint32_t n_docs, ygm_result* out) {
  if (!c || !out || kind > YGM_TOJSON_TEXT || (n_docs && (!states || !state_off || !name_off))) return YGM_EINVAL;
  for (uint32_t d = 0; d < n_docs; d++) if (state_off[d + 1] < state_off[d] || name_off[d + 1] < name_off[d]) return YGM_EINVAL;
  static const uint8_t no_names[1] = {0};   // (every name empty: the arena may be NULL)
  if (n_docs && !names) { if (name_off[n_docs] != name_off[0]) return YGM_EINVAL; names = no_names; }   // (no byte of it is read)
  HostCall H{Op::ToJson, states, n_docs ? state_off : ZERO_OFF, n_docs, n_docs, nullptr, names, n_docs ? name_off : ZERO_OFF};
  H.text_mode = kind;
  return host_call(c, H, out);
}

int ygm_diff_shared_v1(ygm_ctx* c, const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, const uint8_t* sv_arena,
                       const uint64_t* sv_off, const uint32_t* ask_doc, uint32_t n_asks, ygm_result* out) {
  return host_shared_call(c, Op::DiffShared, arena, doc_off, n_docs, sv_arena, sv_off, ask_doc, n_asks, out);
}
int ygm_sync_step2_shared_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, uint32_t n_states, const uint8_t* sv_arena,
                             const uint64_t* sv_off, const uint32_t* ask_state, uint32_t n_asks, ygm_result* out) {
  return host_shared_call(c, Op::Step2Shared, states, state_off, n_states, sv_arena, sv_off, ask_state, n_asks, out);
}
int ygm_sync_step2_shared_opts_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, const uint8_t* state_opt, uint32_t n_states,
                                  const uint8_t* sv_arena, const uint64_t* sv_off, const uint32_t* ask_state, uint32_t n_asks,
                                  ygm_result* out) {
  return host_shared_call(c, Op::Step2Shared, states, state_off, n_states, sv_arena, sv_off, ask_state, n_asks, out, state_opt);
}
int ygm_version_restore_shared_v1(ygm_ctx* c, const uint8_t* states, const uint64_t* state_off, uint32_t n_states, const uint8_t* versions,
                                  const uint64_t* version_off, const uint32_t* ask_state, const uint8_t* restored_opt, uint32_t n_asks,
                                  ygm_result* out) {
  return host_shared_call(c, Op::VersionRestoreShared, states, state_off, n_states, versions, version_off, ask_state, n_asks, out,
                          restored_opt);
}

}  // extern "C"
