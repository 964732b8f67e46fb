// ygm_docstage.hpp -- what the stored-document kernels share (k_snap_count, k_snap, k_text, k_json; HIP only: the
// host twins under tools/snapdev run one document at a time and include none of this):
//   NT, STAGE, DPW : one wave per block; the LDS bytes that hold a wave's documents; the default documents per wave
//   stage          : the wave's consecutive documents copied into LDS when they fit
//   lane_doc       : the lane prologue -- the wave's documents [d0, d1), the lane's document and its input pointer
//   lane_caps      : the statuses decided before a document runs (bad offsets, the empty update), else its Caps
//   put, add_payload : the epilogue -- a document's place, length and status; the wave's payload bytes, one atomic
//   docs_per_wave  : (host) the launchers' documents per wave: YGM_SNAP_DPW, else the caller's hint, else DPW
// A thread per document keeps the reference's sequential algorithm while dpw documents share a wave (lanes >= dpw
// idle): the per-document code diverges from lane to lane, so fewer documents per wave trade SIMD lanes for less
// serialised divergence and more waves in flight.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "ygm_common.hpp"
#include "ygm_snapshot.hpp"

namespace ygm {
namespace docstage {

constexpr int NT = 64;             // one wave per block: documents are independent
constexpr uint32_t DPW = 16;       // documents per wave of the count pass, and the other kernels' default
constexpr uint32_t STAGE = 40960;  // LDS bytes that hold a wave's documents (the kernels declare STAGE + 16)

// The wave's documents [d0, d1) are consecutive in the arena: when their bytes fit, the wave copies them into LDS
// with 16-byte loads and each lane parses its document from there (the codec walks bytes one dependent read at a
// time: ~100 cycles from LDS instead of a global-memory round trip).  Returns the lane's input pointer.
YDEV const uint8_t* stage(uint8_t* stg, const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off, uint32_t d0, uint32_t d1,
                          uint32_t d) {
  const uint64_t a = doc_off[d0], b = doc_off[d1];
  const uint64_t a16 = a & ~15ull;
  const bool staged = b >= a && b - a16 <= STAGE;
  if (staged) {
    const uint4* src = (const uint4*)(arena + a16);
    for (uint32_t c = threadIdx.x; 16u * c < b - a16; c += NT) ((uint4*)stg)[c] = src[c];   // (arena tail padding >= 16)
  }
  __syncthreads();
  if (d >= d1) return nullptr;
  const uint64_t x = doc_off[d];
  return staged && x >= a && doc_off[d + 1] <= b ? stg + (x - a16) : arena + x;
}

// the lane's document of a block that takes dpw of them: d, its input (staged or not), on: the lane has one
struct Lane { uint32_t d; const uint8_t* in; bool on; };
YDEV Lane lane_doc(uint8_t* stg, const uint8_t* __restrict__ arena, const uint64_t* __restrict__ doc_off, uint32_t n_docs, uint32_t dpw) {
  const uint32_t d0 = blockIdx.x * dpw, d1 = d0 + dpw < n_docs ? d0 + dpw : n_docs;
  const uint32_t d = d0 + threadIdx.x;
  const uint8_t* in = stage(stg, arena, doc_off, d0, d1, threadIdx.x < dpw ? d : d1);
  return Lane{d, in, threadIdx.x < dpw && d < n_docs};
}
// a document's length as the count pass takes it: 0 for offsets out of order or 2^30 bytes and more
YDEV uint32_t doc_len(uint64_t a, uint64_t b) { return b > a && b - a < (1ull << 30) ? (uint32_t)(b - a) : 0u; }
// before document [a, b) with counts c (k_snap_count's) runs: ST_INVAL (ok: what else the kernel checked), ST_MALFORMED,
// or ST_OK and the workspace's Caps
YDEV int lane_caps(bool ok, uint64_t a, uint64_t b, const uint4& c, snap::Caps& k) {
  if (!ok || b < a || b - a >= (1ull << 30)) return ST_INVAL;
  if (c.w == 0) return ST_MALFORMED;   // (an empty update: yjs throws reading it)
  k = snap::caps_of(c.x, c.y, c.z, c.w);
  return ST_OK;
}

// the epilogue: document d's place, length (the caller's: 0 unless its status keeps bytes) and status; returns the
// bytes it adds to the payload
YDEV uint64_t put(uint32_t d, uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_len, int32_t* __restrict__ status, uint64_t off,
                  uint32_t len, int st) {
  out_off[d] = off;
  out_len[d] = len;
  status[d] = st;
  return st == ST_OK ? len : 0u;
}
YDEV void add_payload(uint64_t mine, unsigned long long* __restrict__ payload) {
  mine = wave_sum(mine);
  if ((threadIdx.x & (WAVE - 1)) == 0 && mine) atomicAdd(payload, (unsigned long long)mine);
}

// documents per wave of a launch: YGM_SNAP_DPW, else hint (0: none), else DPW; outside 1..NT: DPW
static inline uint32_t docs_per_wave(uint32_t hint) {
  const char* env = getenv("YGM_SNAP_DPW");
  const uint32_t dpw = env ? (uint32_t)atoi(env) : (hint ? hint : DPW);
  return dpw < 1 || dpw > (uint32_t)NT ? DPW : dpw;
}

}  // namespace docstage
}  // namespace ygm
