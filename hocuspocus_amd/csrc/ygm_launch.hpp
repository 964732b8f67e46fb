// ygm_launch.hpp -- the kernel launchers (ygm_k_*): defined in the .hip files, called by the host runtime
// (ygm_engine.cpp).  Every definer and the caller include this header, so a definition that disagrees with its
// declaration does not compile (C-linkage functions cannot be overloaded).  The merge tiers and the SV / diff walkers
// take what they all share as two structs, each filled in one place per call: ygm_merge_in (what a tier reads) and
// ygm_results (where results go).  A pointer cannot then land in its neighbour's place at a call site; a launcher
// lists after them only what is its own (documents, device count, bound, lists, scratch, the stream last) and unpacks
// them into its kernel's parameter list.  ygm_launch_rc is every launcher's return: the launch's error, reported once.
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
int ygm_k_launch_pend_split_g(const uint32_t* list, uint32_t P, const uint32_t* ask_ix, const uint8_t* ws, const uint64_t* out_off,
                              const uint8_t* sv, const uint64_t* sv_off, uint64_t* offs, uint8_t* da, uint8_t* db, uint8_t* dc,
                              uint8_t* dsv, int pass, hipStream_t s);
int ygm_k_launch_snap_plan(const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, uint32_t flags, void* cnt, uint64_t* ws_off,
                           uint64_t* bs, const uint8_t* claim, hipStream_t s);
int ygm_k_launch_snap_text(const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, uint32_t flags, uint8_t* out, uint64_t* out_off,
                           uint64_t* out_len, int32_t* status, uint8_t* claim, unsigned long long* pay, int again, uint64_t slot_total,
                           const uint8_t* opt, hipStream_t s);
int ygm_k_launch_text_flat(const uint8_t* arena, const uint64_t* doc_off, const uint8_t* names, const uint64_t* name_off, uint32_t n_docs,
                           uint32_t flags, uint8_t* out, uint64_t* out_off, uint64_t* out_len, int32_t* status, uint8_t* claim,
                           unsigned long long* pay, int again, uint64_t slot_total, hipStream_t s);
int ygm_k_launch_text(const uint8_t* arena, const uint64_t* doc_off, const uint8_t* names, const uint64_t* name_off, uint32_t n_docs,
                      uint32_t flags, uint32_t mode, const void* cnt, const uint64_t* ws_off, uint8_t* ws, uint64_t* out_off,
                      uint64_t* out_len, int32_t* status, unsigned long long* payload, const uint8_t* claim, uint64_t base, hipStream_t s);
int ygm_k_launch_json(const uint8_t* arena, const uint64_t* doc_off, const uint8_t* names, const uint64_t* name_off, uint32_t n_docs,
                      uint32_t flags, uint32_t kind, const void* cnt, const uint64_t* ws_off, uint8_t* ws, uint64_t* out_off,
                      uint64_t* out_len, int32_t* status, void* meta, uint64_t base, uint64_t ovf_base, uint32_t* list, uint32_t n_list,
                      int again, int fields, hipStream_t s);
int ygm_k_launch_tojson(const uint8_t* arena, const uint64_t* doc_off, const uint8_t* names, const uint64_t* name_off, uint32_t n_docs,
                        uint32_t flags, uint32_t kind, const void* cnt, const uint64_t* ws_off, uint8_t* ws, uint64_t* out_off,
                        uint64_t* out_len, int32_t* status, void* meta, uint64_t base, uint64_t ovf_base, uint32_t* list, uint32_t n_list,
                        int again, hipStream_t s);
int ygm_k_launch_cont_plan(const uint8_t* st_arena, const uint64_t* st_off, uint32_t n_docs, uint32_t flags, uint64_t* ws_off, uint64_t* bs,
                           hipStream_t s);
int ygm_k_launch_cont(const uint8_t* st_arena, const uint64_t* st_off, const uint8_t* up_arena, const uint64_t* up_off, uint32_t n_docs,
                      uint32_t flags, const uint64_t* ws_off, uint8_t* ws, uint8_t* out, uint64_t* out_off, uint64_t* out_len,
                      int32_t* status, hipStream_t s);
int ygm_k_launch_snap(const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, uint32_t flags, const void* cnt, const uint64_t* ws_off,
                      uint8_t* ws, uint64_t* out_off, uint64_t* out_len, int32_t* status, unsigned long long* payload, const uint8_t* claim,
                      uint64_t base, uint32_t* pend_list, unsigned int* pend_n, hipStream_t s);
int ygm_k_launch_snap_w(const uint8_t* arena, const uint64_t* doc_off, uint32_t n_docs, uint32_t flags, const void* cnt, const uint64_t* ws_off,
                        uint8_t* ws, uint64_t* out_off, uint64_t* out_len, int32_t* status, unsigned long long* payload, const uint8_t* claim,
                        uint64_t base, uint32_t* pend_list, unsigned int* pend_n, uint32_t dpw_hint, const uint8_t* opt, hipStream_t s);
int ygm_k_launch_pend_plan(const uint32_t* list, uint32_t P, const uint8_t* ws, const uint64_t* out_off, uint64_t* upd_off, uint32_t* doc_upd,
                           hipStream_t s);
int ygm_k_launch_pend_copy(const uint32_t* list, uint32_t P, const uint8_t* ws, const uint64_t* out_off, const uint64_t* upd_off, uint8_t* dst,
                           hipStream_t s);
int ygm_k_launch_pend_fix(const uint32_t* list, uint32_t P, const uint64_t* m_off, const uint64_t* m_len, const int32_t* m_st,
                          const int32_t* pst, uint64_t tail, uint64_t* out_off, uint64_t* out_len, int32_t* status, hipStream_t s);
int ygm_k_launch_pend_split(const uint32_t* list, uint32_t P, const uint8_t* ws, const uint64_t* out_off, const uint8_t* sv,
                            const uint64_t* sv_off, uint64_t* offs, uint8_t* da, uint8_t* db, uint8_t* dc, uint8_t* dsv, int pass,
                            hipStream_t s);
int ygm_k_launch_pend_join(uint32_t P, const uint8_t* ad, const uint64_t* a_off, const uint64_t* a_len, const int32_t* a_st, const uint8_t* bd,
                           const uint64_t* offs, const uint8_t* cd, const uint64_t* c_off, const uint64_t* c_len, const int32_t* c_st,
                           uint64_t* upd_off, uint32_t* doc_upd, int32_t* pst, uint8_t* dst, int pass, hipStream_t s);
int ygm_k_launch_ver_cut(const uint8_t* S, const uint64_t* s_off, const int32_t* s_st, const uint8_t* V, const uint64_t* v_off,
                         uint32_t n_docs, uint32_t flags, uint8_t* out, uint64_t out_total, uint64_t* out_off, uint64_t* out_len,
                         int32_t* status, hipStream_t s);
int ygm_k_launch_ver_cut_gather(const uint8_t* S, const uint64_t* s_off, const int32_t* s_st, const uint32_t* ix, const uint64_t* ask_base,
                                const uint8_t* V, const uint64_t* v_off, uint32_t n_asks, uint32_t flags, uint8_t* out, uint64_t out_total,
                                uint64_t* out_off, uint64_t* out_len, int32_t* status, hipStream_t s);
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
