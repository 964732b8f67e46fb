// ygm_launch.hpp -- the kernel launchers (ygm_k_*): defined in the .hip files, called by the host runtime
// (ygm_engine.cpp).  Every definer and the caller include this header, so a definition that disagrees with its
// declaration does not compile (C-linkage functions cannot be overloaded).  The merge tiers and the SV / diff walkers
// take what they all share as two structs, each filled in one place per call: ygm_merge_in (what a tier reads) and
// ygm_results (where results go).  A pointer cannot then land in its neighbour's place at a call site; a launcher
// lists after them only what is its own (documents, device count, bound, lists, scratch, the stream last) and unpacks
// them into its kernel's parameter list.  The stored-document launchers (snapshot, text, JSON, toJSON, contains, the
// pending documents, the version cuts) take theirs the same way: ygm_docs, ygm_side, ygm_ws, ygm_results again,
// ygm_rerun, ygm_packed, ygm_batch_out, ygm_pend_parts and ygm_pend_batch (each described below), built in one place
// each by the engine (ygm_ctx::results_in and its kin, WsBatch::docs / ws / results).  The update-V2 launchers keep their
// own argument lists.  ygm_launch_rc is every launcher's return: the launch's error, reported once.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

// 0, or -1 with one stderr line when the launches since the last check left an error (fn: the launcher's __func__)
static inline int ygm_launch_rc(const char* fn) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { fprintf(stderr, "ygm: %s: %s\n", fn, hipGetErrorString(e)); return -1; }
  return 0;
}

extern "C" {
// what every merge tier reads: the packed updates, the context's flags, the call's counter slot (a DocMeta)
struct ygm_merge_in { const uint8_t* arena; const uint64_t* upd_off; const uint32_t* doc_upd; uint32_t flags; void* meta; };
// where results go: the output arena (per-document slots in [0, slot_total), the overflow region up to out_cap) and
// each document's place, length and status
struct ygm_results { uint8_t* out; uint64_t* out_off; uint64_t* out_len; int32_t* status; uint64_t slot_total, out_cap; };
// the large-document tier's documents (n_fb entries of the routing pass's list, fb_bytes in all) and its scratch: the
// scan (ygm_k_big_scan_bytes), block tables and struct records, the mid size's hand-ons, the documents left to replay
struct ygm_big_tier {
  const uint32_t* fb_list; uint32_t n_fb; uint64_t fb_bytes;
  void *scan, *blk; uint64_t blk_cap; void* rec; uint64_t rec_cap;
  uint32_t *up_list, *seq_list;
};
// the sequential replay's scratch: upd_cap entries of the per-update arrays, byte_cap of cnt, byte_cap / 2 + 1 of drec
struct ygm_seq_scratch { void* readers; int *order, *tmp; const uint8_t** ubase; uint32_t *ulen, *cnt; void* drec; uint64_t upd_cap, byte_cap; };
// the documents a stored-document batch reads: the arena, its n_docs + 1 offsets, the context's flags or-ed with the
// call's view bits, the per-document option bytes (nullable: none set).  Filled by WsBatch::docs
struct ygm_docs { const uint8_t* arena; const uint64_t* doc_off; uint32_t n_docs, flags; const uint8_t* opt; };
// the second per-document arena of a call and its offsets (one more than its units): names, field lists, the updates of
// contains, versions, state vectors.  Filled at the entry point from the caller's pair
struct ygm_side { const uint8_t* arena; const uint64_t* off; };
// the general path's workspaces, as ygm_k_launch_snap_plan (or _cont_plan) sizes them: per-document counts, the scanned
// offsets (n_docs + 1, the total last), the buffer, where the workspaces start in it (after the flat tier's slots), the
// flat tier's claims (nullable: the tier did not run).  Filled by WsBatch::ws
struct ygm_ws { void* cnt; uint64_t* ws_off; uint8_t* ws; uint64_t base; const uint8_t* claim; };
// the JSON kernels' second run: where the overflow region starts (after the workspaces), the list the first run wrote
// and the second reads, its length, 0 / 1 for the first / second run.  Filled by json_dev per launch
struct ygm_rerun { uint64_t ovf_base; uint32_t* list; uint32_t n_list; int again; };
// a snapshot batch's outputs packed into one arena (offsets n + 1) with the snapshots' statuses.  Filled by
// ygm_ctx::packed after pack_snapshots
struct ygm_packed { const uint8_t* data; const uint64_t* off; const int32_t* st; };
// a finished batch's results as a later launch reads them (a ygm_device_result's pointers)
struct ygm_batch_out { const uint8_t* data; const uint64_t* off; const uint64_t* len; const int32_t* status; };
// step2 of pending documents: the four scanned offset tables (offs: 4 x (P + 1)) and the parts they place -- state part,
// pending delete set, pending structs, state vector (null in the planning pass).  Placed by step2_pending_split, filled by ygm_ctx::pend_parts
struct ygm_pend_parts { uint64_t* offs; uint8_t *da, *db, *dc, *dsv; };
// the pending documents' three-update batch for the merge: update offsets (3 P + 1), doc_upd (P + 1), the arena (null
// in a planning pass).  Filled by ygm_ctx::pend_batch
struct ygm_pend_batch { uint64_t* upd_off; uint32_t* doc_upd; uint8_t* dst; };
size_t ygm_k_meta_bytes();
size_t ygm_k_seq_reader_bytes();
size_t ygm_k_drec_bytes();
// (the SV / diff launchers: r->slot_total is where the exact kernel's packed region starts)
int ygm_k_launch_doc(int mode, const uint8_t* arena, const uint64_t* doc_off, const uint8_t* sv_arena, const uint64_t* sv_off,
                     const uint32_t* docs, uint32_t n_docs, uint32_t flags, const ygm_results* r, unsigned long long* lb, void* meta,
                     hipStream_t s);
size_t ygm_k_sv_table_bytes(uint32_t n_docs);
int ygm_k_launch_ask_plan(const uint64_t* doc_off, uint32_t n_docs, const uint32_t* ask_doc, uint32_t n_asks, uint32_t* ask_ix,
                          uint64_t* ask_base, uint64_t* bs, hipStream_t s);
int ygm_k_launch_ask_status(const uint32_t* ask_ix, uint32_t n_asks, const int32_t* st_state, int32_t* status, uint64_t* len, hipStream_t s);
int ygm_k_launch_ask_pending(const uint32_t* ask_ix, uint32_t n_asks, const int32_t* st_state, uint32_t* list, unsigned int* n_out,
                             hipStream_t s);
int ygm_k_launch_doc_lean_gather(const uint8_t* arena, const uint64_t* doc_off, const uint8_t* sv_arena, const uint64_t* sv_off,
                                 const uint32_t* ask_ix, const uint64_t* ask_base, uint32_t n_asks, const ygm_results* r, void* meta,
                                 uint32_t* defer_list, uint8_t* tbl, uint32_t* tbl_n, hipStream_t s);
int ygm_k_launch_doc_gather(const uint8_t* arena, const uint64_t* doc_off, const uint8_t* sv_arena, const uint64_t* sv_off,
                            const uint32_t* docs, const uint32_t* ask_ix, uint32_t n_docs, uint32_t flags, const ygm_results* r,
                            unsigned long long* lb, void* meta, hipStream_t s);
// The stored-document launchers.  r: in the flat tiers r->out is the workspace buffer and r->slot_total its slot region;
// the general path writes into w->ws and takes r's places, lengths and statuses alone; in ygm_k_launch_cont r->out holds
// the answers, a byte per document; in the version cuts r->slot_total is the slots' extent (the kernels' out_total).
int ygm_k_launch_snap_plan(const ygm_docs* d, const ygm_ws* w, uint64_t* bs, hipStream_t s);
int ygm_k_launch_snap_text(const ygm_docs* d, const ygm_results* r, uint8_t* claim, unsigned long long* pay, int again, hipStream_t s);
int ygm_k_launch_text_flat(const ygm_docs* d, const ygm_side* names, const ygm_results* r, uint8_t* claim, unsigned long long* pay, int again, hipStream_t s);
int ygm_k_launch_text(const ygm_docs* d, const ygm_side* names, uint32_t mode, const ygm_ws* w, const ygm_results* r,
                      unsigned long long* payload, hipStream_t s);
// one signature for the two walkers (fields: ygm_k_launch_json alone, 0 for ygm_k_launch_tojson)
int ygm_k_launch_json(const ygm_docs* d, const ygm_side* names, uint32_t kind, const ygm_ws* w, const ygm_results* r,
                      const ygm_rerun* run, void* meta, int fields, hipStream_t s);
int ygm_k_launch_tojson(const ygm_docs* d, const ygm_side* names, uint32_t kind, const ygm_ws* w, const ygm_results* r,
                        const ygm_rerun* run, void* meta, int fields, hipStream_t s);
int ygm_k_launch_cont_plan(const ygm_docs* st, const ygm_ws* w, uint64_t* bs, hipStream_t s);   // (w->ws_off alone)
int ygm_k_launch_cont(const ygm_docs* st, const ygm_side* upd, const ygm_ws* w, const ygm_results* r, hipStream_t s);
int ygm_k_launch_snap(const ygm_docs* d, const ygm_ws* w, const ygm_results* r, unsigned long long* payload, uint32_t* pend_list,
                      unsigned int* pend_n, uint32_t dpw_hint, hipStream_t s);
// the pending documents (list, P of them) of the snapshot in ws, their PendHdr layouts at out_off
int ygm_k_launch_pend_plan(const uint32_t* list, uint32_t P, const uint8_t* ws, const uint64_t* out_off, const ygm_pend_batch* b, hipStream_t s);
int ygm_k_launch_pend_copy(const uint32_t* list, uint32_t P, const uint8_t* ws, const uint64_t* out_off, const ygm_pend_batch* b, hipStream_t s);
// m: the merged batch; tail: where its bytes were appended to r's arena
int ygm_k_launch_pend_fix(const uint32_t* list, uint32_t P, const ygm_batch_out* m, const int32_t* pst, uint64_t tail,
                          const ygm_results* r, hipStream_t s);
// ask_ix non-null: the gather form (list holds asks, ask a's parts come from the record of its state ask_ix[a])
int ygm_k_launch_pend_split(const uint32_t* list, uint32_t P, const uint32_t* ask_ix, const uint8_t* ws, const uint64_t* out_off,
                            const ygm_side* sv, const ygm_pend_parts* parts, int pass, hipStream_t s);
// a, c: the diffs of the state parts and of the pending structs (parts->db between them)
int ygm_k_launch_pend_join(uint32_t P, const ygm_batch_out* a, const ygm_batch_out* c, const ygm_pend_parts* parts,
                           const ygm_pend_batch* b, int32_t* pst, int pass, hipStream_t s);
int ygm_k_launch_ver_cut(const ygm_packed* S, const ygm_side* V, uint32_t n_docs, uint32_t flags, const ygm_results* r, hipStream_t s);
int ygm_k_launch_ver_cut_gather(const ygm_packed* S, const uint32_t* ix, const uint64_t* ask_base, const ygm_side* V, uint32_t n_asks,
                                uint32_t flags, const ygm_results* r, hipStream_t s);
int ygm_k_launch_pack(const uint8_t* src, const uint64_t* off, const uint64_t* len, const int32_t* status, uint32_t n, uint64_t* bsum,
                      uint8_t* dst, uint64_t* poff, hipStream_t s);
int ygm_k_launch_doc_lean(int mode, const uint8_t* arena, uint64_t arena_bytes, const uint64_t* doc_off, const uint8_t* sv_arena,
                          uint64_t sv_bytes, const uint64_t* sv_off, uint32_t n_docs, uint32_t flags, const ygm_results* r, void* meta,
                          uint32_t* defer_list, uint8_t* tbl, uint32_t* tbl_n, hipStream_t s);
uint32_t ygm_k_lean_stage_bytes();
uint32_t ygm_k_lean_no_idlen_flag();   // the lean_flags bit of ygm_k_launch_merge_lean that switches the id-length parse off
// The merge tiers.  Each takes the input and the results, then what is its own.  n_dev: the device-side count of the
// list (nullptr: the bound is the count); bound: the host's upper bound of it, which sizes the grid.
int ygm_k_launch_merge_lean(const ygm_merge_in* in, const ygm_results* r, uint32_t n_docs, uint32_t lean_flags, void* meta_next,
                            uint32_t* defer_list, const uint64_t* doc_off, const uint16_t* upd_len, hipStream_t s);
int ygm_k_launch_big_wait(void* meta, uint32_t n_large, hipStream_t s);
int ygm_k_launch_build_off(const uint64_t* doc_off, const uint16_t* upd_len, const uint32_t* doc_upd, const uint32_t* list, uint32_t n,
                           uint64_t* upd_off, hipStream_t s);
int ygm_k_launch_merge_lean_wide(const ygm_merge_in* in, const ygm_results* r, uint32_t n_docs, const uint32_t* list, uint32_t n_list,
                                 void* meta_next, uint32_t* defer_list, const uint16_t* upd_len, hipStream_t s);
int ygm_k_launch_route_big(const ygm_merge_in* in, const ygm_results* r, const uint32_t* docs, const unsigned int* n_dev, uint32_t bound,
                           uint32_t* fb_list, uint32_t* rest, hipStream_t s);
int ygm_k_launch_merge_wave(const ygm_merge_in* in, const ygm_results* r, const uint32_t* docs, const unsigned int* n_dev, uint32_t bound,
                            uint32_t* defer_list, uint32_t* fb_list, hipStream_t s);
int ygm_k_launch_merge_fast(const ygm_merge_in* in, const ygm_results* r, const uint32_t* docs, const unsigned int* n_dev, uint32_t bound,
                            uint32_t* fb_list, hipStream_t s);
int ygm_k_launch_merge_seq(const ygm_merge_in* in, const ygm_results* r, const uint32_t* list, uint32_t n, const ygm_seq_scratch* scr,
                           hipStream_t s);
int ygm_k_launch_scan(uint64_t* v, uint32_t n, uint64_t* bs, hipStream_t s);
size_t ygm_k_v2_cols();
int ygm_k_launch_v21(int pass, const uint8_t* arena, const uint64_t* upd_off, uint32_t n_upd, const uint32_t* doc_upd, uint32_t n_docs,
                     uint32_t mode, uint32_t flags, uint64_t* len_or_off, int32_t* st, uint8_t* out, uint8_t* cl, hipStream_t s);
int ygm_k_launch_v12_count(const uint8_t* v1, const uint64_t* v1_off, const uint64_t* v1_len, const int32_t* v1_st, const uint8_t* v2a,
                           uint64_t v2n, const uint64_t* upd_off, const uint32_t* doc_upd, const int32_t* ust, uint32_t n_docs, uint32_t mode,
                           uint32_t flags, uint32_t* L, uint64_t* tot, int32_t* st, const uint8_t* claim, hipStream_t s);
int ygm_k_launch_v12_write(const uint8_t* v1, const uint64_t* v1_off, const uint64_t* v1_len, const uint8_t* v2a, uint64_t v2n,
                           const uint64_t* upd_off, const uint32_t* doc_upd, uint32_t n_docs, uint32_t mode, uint32_t flags, const uint32_t* L,
                           const uint64_t* off, int32_t* st, uint8_t* out, uint64_t* out_len, const uint8_t* claim, uint64_t base, uint64_t* fo,
                           hipStream_t s);
int ygm_k_launch_v12_fast(const uint8_t* v1, const uint64_t* v1_off, const uint64_t* v1_len, const int32_t* v1_st, const uint64_t* slot_off,
                          const uint32_t* doc_upd, const int32_t* ust, uint32_t n_docs, uint8_t* out, uint64_t* fo, uint64_t* olen, int32_t* ost,
                          uint8_t* claim, unsigned long long* payload, uint8_t* scr, uint64_t slot_total, hipStream_t s);
size_t ygm_k_v12_fast_scratch();
int ygm_k_launch_v2_status(const int32_t* ust, uint32_t n, int32_t* status, uint64_t* len, hipStream_t s);
int ygm_k_launch_v2_lens(const uint64_t* off, const int32_t* st, uint32_t n, uint64_t* len, hipStream_t s);
size_t ygm_k_big_blk_bytes();
size_t ygm_k_big_rec_bytes();
int ygm_k_launch_big_scan(const ygm_merge_in* in, const ygm_big_tier* big, hipStream_t s);   // (writes no results)
// large = 0: the mid size, large = 1: the 16-wave size, over the big->fb_list indices in fbx[0, n)
int ygm_k_launch_merge_big(int large, const ygm_merge_in* in, const ygm_results* r, const ygm_big_tier* big, const uint32_t* fbx, uint32_t n,
                           hipStream_t s);
size_t ygm_k_big_scan_bytes(uint32_t n_fb, uint64_t fb_bytes);
void ygm_k_big_lists(void* scan, uint32_t n_fb, uint64_t fb_bytes, unsigned long long** cnt, uint32_t** llist, uint32_t** mlist);
}
