// ygm_version.hip -- version history (ygm_version_restore_v1 / ygm_version_restore_shared_v1): the cut kernel between the two snapshot passes.
//   k_ver_cut : one wave per document.  The walk over S (the packed no-GC snapshot) finds struct boundaries one
//               after the other, so it is wave-uniform (every lane holds the same cursor, in registers); what it
//               finds is long contiguous runs -- a block's kept prefix, the version's delete set -- which the wave
//               copies in 16-byte pieces at any source / destination phase, bytes only at a run's ragged ends.  The
//               version's state vector (at most ver::MAX_SV entries) sits in LDS; a block's client is looked up by
//               the whole wave, lane l testing entries l, l + 64, ..., then one ballot.
//   k_ver_cut_gather : the same cut for asks that share states (ygm_version_restore_shared_v1): one wave per ask, ask a
//               reading the packed snapshot of state ix[a] in place and its own version; the asks of one state sit on
//               neighbouring workgroups, so all but the first read of S come from L2 / MALL.  S is only read.
// Reads are aligned 16-byte pieces: up to 31 bytes past a run's end, inside the 64 readable bytes that follow each
// arena (pack_snapshots pads S; the host API pads the versions, the device form asks for it).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "ygm_common.hpp"
#include "ygm_version.hpp"
#include "ygm_launch.hpp"

namespace ygm {

constexpr int VR_NT = 64;

YDEV uint64_t vr_fsh(uint64_t a, uint64_t b, uint32_t s) { return s ? (a >> s) | (b << (64u - s)) : a; }

struct WaveW {
  uint32_t l;
  YDEV uint32_t lane() const { return l; }
  YDEV int32_t find(const ver::SvEnt* t, uint32_t n, uint32_t client) const {
    for (uint32_t b = 0; b < n; b += VR_NT) {
      const uint32_t i = b + l;
      const unsigned long long m = __ballot(i < n && t[i].client == client);
      if (m) return (int32_t)(b + (uint32_t)__ffsll((long long)m) - 1u);
    }
    return -1;
  }
  // one lane stores, the wave (the whole workgroup) sees it after the barrier
  YDEV void put(ver::SvEnt* t, uint32_t i, uint32_t client, uint32_t clock) const {
    if (l == 0) { t[i].client = client; t[i].clock = clock; }
    __syncthreads();
  }
  // d[0, n) = s[0, n): bytes up to the destination's 16-byte boundary, then aligned 16-byte stores whose source is
  // two aligned 16-byte loads shifted by its phase (one load when the phases agree), then the last bytes
  YDEV void copy(uint8_t* d, const uint8_t* s, uint32_t n) const {
    uint32_t head = (uint32_t)(0u - (uint32_t)(uintptr_t)d) & 15u;
    if (head > n) head = n;
    if (l < head) d[l] = s[l];
    d += head; s += head; n -= head;
    const uint32_t nch = n >> 4, ph = (uint32_t)(uintptr_t)s & 15u;
    const uint4* sa = (const uint4*)(s - ph);
    uint4* da = (uint4*)d;
    if (ph == 0) {
      for (uint32_t c = l; c < nch; c += VR_NT) da[c] = sa[c];
    } else {
      const uint32_t sh = 8u * (ph & 7u);
      for (uint32_t c = l; c < nch; c += VR_NT) {
        const uint4 lo = sa[c], hi = sa[c + 1];
        const uint64_t q0 = (uint64_t)lo.x | ((uint64_t)lo.y << 32), q1 = (uint64_t)lo.z | ((uint64_t)lo.w << 32);
        const uint64_t q2 = (uint64_t)hi.x | ((uint64_t)hi.y << 32), q3 = (uint64_t)hi.z | ((uint64_t)hi.w << 32);
        const uint64_t a = ph < 8 ? q0 : q1, b = ph < 8 ? q1 : q2, e = ph < 8 ? q2 : q3;
        const uint64_t r0 = vr_fsh(a, b, sh), r1 = vr_fsh(b, e, sh);
        da[c] = make_uint4((uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)r1, (uint32_t)(r1 >> 32));
      }
    }
    const uint32_t t0 = nch << 4;
    if (l < n - t0) d[t0 + l] = s[t0 + l];
  }
};

// Document d's slot: al16(s_off[d] + v_off[d] + 32 d), capacity |S| + |version| + 16 (the header and the delete set
// come from the version, every block from S and no longer than there).  A document whose snapshot was refused
// (s_st) keeps that status.
__global__ __launch_bounds__(VR_NT) void k_ver_cut(const uint8_t* __restrict__ S, const uint64_t* __restrict__ s_off,
                                                  const int32_t* __restrict__ s_st, const uint8_t* __restrict__ V,
                                                  const uint64_t* __restrict__ v_off, uint32_t n_docs, uint32_t flags,
                                                  uint8_t* __restrict__ out, uint64_t out_total, uint64_t* __restrict__ out_off,
                                                  uint64_t* __restrict__ out_len, int32_t* __restrict__ status) {
  __shared__ ver::SvEnt tbl[ver::MAX_SV];
  const uint32_t d = blockIdx.x;
  if (d >= n_docs) return;
  const uint64_t a = s_off[d], b = s_off[d + 1], va = v_off[d], vb = v_off[d + 1];
  const uint64_t slot = (a + va + 32ull * d + 15ull) & ~15ull;
  int st = s_st[d];
  uint32_t ol = 0;
  if (st == ST_OK) {
    if (b < a || vb < va || b - a >= (1ull << 30) || vb - va >= (1ull << 30)) st = ST_INVAL;
    else {
      const uint32_t sn = (uint32_t)(b - a), vn = (uint32_t)(vb - va), cap = sn + vn + 16u;
      if (slot + cap > out_total) st = ST_NOMEM;
      else st = ver::cut_doc(WaveW{threadIdx.x}, S + a, sn, V + va, vn, flags, tbl, out + slot, cap, ol);
    }
  }
  if (threadIdx.x == 0) { out_off[d] = slot; out_len[d] = st == ST_OK ? ol : 0u; status[d] = st; }
}

// The gather form.  ix / ask_base are the plan of k_ask_plan over s_off: the checked state id per ask (VR_ASK_BAD: an id
// the plan refused, never used as an index -- the ask carries ST_INVAL) and the exclusive scan of the asks' snapshot
// lengths.  Ask a's slot: al16(ask_base[a] + v_off[a] + 32 a), capacity |S| + |version| + 16 as above; an ask of a
// refused id or of a refused state writes its offset, length 0 and status, nothing else.
constexpr uint32_t VR_ASK_BAD = 0xFFFFFFFFu;   // (DW_ASK_BAD of the plan kernel, ygm_walk.hip)

__global__ __launch_bounds__(VR_NT) void k_ver_cut_gather(const uint8_t* __restrict__ S, const uint64_t* __restrict__ s_off,
                                                         const int32_t* __restrict__ s_st, const uint32_t* __restrict__ ix,
                                                         const uint64_t* __restrict__ ask_base, const uint8_t* __restrict__ V,
                                                         const uint64_t* __restrict__ v_off, uint32_t n_asks, uint32_t flags,
                                                         uint8_t* __restrict__ out, uint64_t out_total, uint64_t* __restrict__ out_off,
                                                         uint64_t* __restrict__ out_len, int32_t* __restrict__ status) {
  __shared__ ver::SvEnt tbl[ver::MAX_SV];
  const uint32_t q = blockIdx.x;
  if (q >= n_asks) return;
  const uint32_t sd = ix[q];
  const uint64_t va = v_off[q], vb = v_off[q + 1];
  const uint64_t slot = (ask_base[q] + va + 32ull * q + 15ull) & ~15ull;
  int st = sd == VR_ASK_BAD ? (int)ST_INVAL : s_st[sd];
  uint32_t ol = 0;
  if (st == ST_OK) {
    const uint64_t a = s_off[sd], b = s_off[sd + 1];
    if (b < a || vb < va || b - a >= (1ull << 30) || vb - va >= (1ull << 30)) st = ST_INVAL;
    else {
      const uint32_t sn = (uint32_t)(b - a), vn = (uint32_t)(vb - va), cap = sn + vn + 16u;
      if (slot + cap > out_total) st = ST_NOMEM;
      else st = ver::cut_doc(WaveW{threadIdx.x}, S + a, sn, V + va, vn, flags, tbl, out + slot, cap, ol);
    }
  }
  if (threadIdx.x == 0) { out_off[q] = slot; out_len[q] = st == ST_OK ? ol : 0u; status[q] = st; }
}

}  // namespace ygm

using namespace ygm;

extern "C" {

// (r->slot_total: the slots' extent, the kernels' out_total)
int ygm_k_launch_ver_cut(const ygm_packed* S, const ygm_side* V, uint32_t n_docs, uint32_t flags, const ygm_results* r, hipStream_t s) {
  if (n_docs == 0) return 0;
  hipLaunchKernelGGL(k_ver_cut, dim3(n_docs), dim3(VR_NT), 0, s, S->data, S->off, S->st, V->arena, V->off, n_docs, flags, r->out, r->slot_total,
                     r->out_off, r->out_len, r->status);
  return ygm_launch_rc(__func__);
}

int ygm_k_launch_ver_cut_gather(const ygm_packed* S, const uint32_t* ix, const uint64_t* ask_base, const ygm_side* V, uint32_t n_asks,
                                uint32_t flags, const ygm_results* r, hipStream_t s) {
  if (n_asks == 0) return 0;
  hipLaunchKernelGGL(k_ver_cut_gather, dim3(n_asks), dim3(VR_NT), 0, s, S->data, S->off, S->st, ix, ask_base, V->arena, V->off, n_asks, flags,
                     r->out, r->slot_total, r->out_off, r->out_len, r->status);
  return ygm_launch_rc(__func__);
}

}  // extern "C"
