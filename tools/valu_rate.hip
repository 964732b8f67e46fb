// valu_rate.hip -- sustained issue cost of the lean merge kernel's VALU instructions on one SIMD (tooling).
//
// For each instruction: eight independent chains, round robin, in an unrolled loop (no chain waits on itself), run by
// 1, 2 and 4 waves per SIMD at once: one workgroup of 4 W waves per CU (its LDS request keeps a second one off the CU;
// the waves of a workgroup go round robin over the CU's four SIMDs).  Every wave stamps the shader clock (s_memtime)
// around its loop; a workgroup's span is its last end minus its first start, and
//
//     cycles per wave-instruction per SIMD = span / (W x instructions per wave)
//
// 4 at every W says one wave64 instruction holds the SIMD for four cycles whoever issues the next; a figure that falls
// with W says a single wave cannot issue back to back and other waves fill the gaps.  The shader clock's rate comes
// from s_memrealtime (100 MHz) stamped beside it.  Prints one JSON line per (instruction, W).
//
//     hipcc --offload-arch=gfx950 -O3 -o valu_rate valu_rate.hip && ./valu_rate
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int CHAINS = 8, UNROLL = 16, ITERS = 1024;   // 131 072 instructions per wave

enum Op { AND, ADD, CNDMASK, BITOP3, ALIGNBYTE, DOT4, LSHLREV, MOV_DPP, FMA,
          CMP_VCC, CMP_SGPR, BFE, LSHRREV, OR, OR3, LSHL_OR, AND_OR, MOV, READLANE, PERM, BFM, MED3, MIN, MUL24, MAD24,
          LSHL_CONST, SUB, BFI, ALIGNBIT, N_OPS };
static const char* const OP_NAME[N_OPS] = {"v_and_b32", "v_add_u32", "v_cndmask_b32", "v_bitop3_b32", "v_alignbyte_b32",
                                           "v_dot4_u32_u8", "v_lshlrev_b32", "v_mov_b32 dpp row_shr:1", "v_fma_f32",
                                           "v_cmp_lt_u32 vcc", "v_cmp_lt_u32 sgpr pair", "v_bfe_u32", "v_lshrrev_b32", "v_or_b32",
                                           "v_or3_b32", "v_lshl_or_b32", "v_and_or_b32", "v_mov_b32", "v_readlane_b32",
                                           "v_perm_b32", "v_bfm_b32", "v_med3_u32", "v_min_u32", "v_mul_u32_u24",
                                           "v_mad_u32_u24", "v_lshlrev_b32 (constant count)", "v_sub_u32", "v_bfi_b32",
                                           "v_alignbit_b32"};

// one round: the instruction once on each of the eight chains (a, b: loop-invariant operands; m: a lane mask)
#define ROUND8(INS, TAIL)                                                                                       \
  asm volatile(INS " %0, " TAIL(0) "\n\t" INS " %1, " TAIL(1) "\n\t" INS " %2, " TAIL(2) "\n\t" INS " %3, " TAIL(3) "\n\t" \
               INS " %4, " TAIL(4) "\n\t" INS " %5, " TAIL(5) "\n\t" INS " %6, " TAIL(6) "\n\t" INS " %7, " TAIL(7)          \
               : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])  \
               : "v"(a), "v"(b), "s"(m))
// the same for an instruction without a vector destination (a compare, a lane read): its result goes to vcc or s[20:21]
#define ROUND8S(INS, TAIL)                                                                                      \
  asm volatile(INS " " TAIL(0) "\n\t" INS " " TAIL(1) "\n\t" INS " " TAIL(2) "\n\t" INS " " TAIL(3) "\n\t"            \
               INS " " TAIL(4) "\n\t" INS " " TAIL(5) "\n\t" INS " " TAIL(6) "\n\t" INS " " TAIL(7)                     \
               : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7])  \
               : "v"(a), "v"(b), "s"(m) : "vcc", "s20", "s21")
#define T_AB(i) "%8, %" #i                       // dst = a op dst
#define T_CND(i) "%" #i ", %8, %10"              // dst = mask ? a : dst
#define T_3(i) "%" #i ", %8, %9"                 // dst = f(dst, a, b)
#define T_BITOP(i) "%" #i ", %8, %9 bitop3:0x96" // dst = dst ^ a ^ b
#define T_DOT(i) "%8, %9, %" #i                  // dst = dot4(a, b) + dst
#define T_MOV(i) "%8"                            // dst = a
#define T_K3(i) "3, %" #i                        // dst = dst << 3
#define T_VCC(i) "vcc, %8, %" #i                 // vcc = a < x
#define T_SP(i) "s[20:21], %8, %" #i             // s[20:21] = a < x
#define T_RL(i) "s20, %" #i ", 5"                // s20 = lane 5 of x
#define T_DPP(i) "%" #i " row_shr:1 row_mask:0xf bank_mask:0xf"

template <int OP>
__global__ __launch_bounds__(1024) void k_rate(uint64_t* __restrict__ stamps, uint32_t* __restrict__ sink) {
  extern __shared__ uint8_t keep_alone[];   // (only its size matters: one workgroup per CU)
  uint32_t x[CHAINS];
  for (int c = 0; c < CHAINS; c++) x[c] = threadIdx.x * 2654435761u + (uint32_t)c;
  const uint32_t a = 0x01010101u | threadIdx.x, b = 3u;
  const uint64_t m = 0x5555555555555555ull;
  __syncthreads();
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  const uint64_t t0 = __builtin_amdgcn_s_memtime();
  __builtin_amdgcn_sched_barrier(0);
  for (int it = 0; it < ITERS; it++) {
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      if constexpr (OP == AND) ROUND8("v_and_b32", T_AB);
      if constexpr (OP == ADD) ROUND8("v_add_u32", T_AB);
      if constexpr (OP == CNDMASK) ROUND8("v_cndmask_b32", T_CND);
      if constexpr (OP == BITOP3) ROUND8("v_bitop3_b32", T_BITOP);
      if constexpr (OP == ALIGNBYTE) ROUND8("v_alignbyte_b32", T_3);
      if constexpr (OP == DOT4) ROUND8("v_dot4_u32_u8", T_DOT);
      if constexpr (OP == LSHLREV) ROUND8("v_lshlrev_b32", T_AB);
      if constexpr (OP == MOV_DPP) ROUND8("v_mov_b32_dpp", T_DPP);
      if constexpr (OP == FMA) ROUND8("v_fma_f32", T_3);
      if constexpr (OP == CMP_VCC) ROUND8S("v_cmp_lt_u32_e32", T_VCC);
      if constexpr (OP == CMP_SGPR) ROUND8S("v_cmp_lt_u32_e64", T_SP);
      if constexpr (OP == BFE) ROUND8("v_bfe_u32", T_3);
      if constexpr (OP == LSHRREV) ROUND8("v_lshrrev_b32", T_AB);
      if constexpr (OP == OR) ROUND8("v_or_b32", T_AB);
      if constexpr (OP == OR3) ROUND8("v_or3_b32", T_3);
      if constexpr (OP == LSHL_OR) ROUND8("v_lshl_or_b32", T_3);
      if constexpr (OP == AND_OR) ROUND8("v_and_or_b32", T_3);
      if constexpr (OP == MOV) ROUND8("v_mov_b32", T_MOV);
      if constexpr (OP == READLANE) ROUND8S("v_readlane_b32", T_RL);
      if constexpr (OP == PERM) ROUND8("v_perm_b32", T_3);
      if constexpr (OP == BFM) ROUND8("v_bfm_b32", T_AB);
      if constexpr (OP == MED3) ROUND8("v_med3_u32", T_3);
      if constexpr (OP == MIN) ROUND8("v_min_u32", T_AB);
      if constexpr (OP == MUL24) ROUND8("v_mul_u32_u24", T_AB);
      if constexpr (OP == MAD24) ROUND8("v_mad_u32_u24", T_3);
      if constexpr (OP == LSHL_CONST) ROUND8("v_lshlrev_b32", T_K3);
      if constexpr (OP == SUB) ROUND8("v_sub_u32", T_AB);
      if constexpr (OP == BFI) ROUND8("v_bfi_b32", T_3);
      if constexpr (OP == ALIGNBIT) ROUND8("v_alignbit_b32", T_3);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
  uint32_t s = 0;
  for (int c = 0; c < CHAINS; c++) s ^= x[c];
  sink[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if (threadIdx.x % 64 == 0) {
    uint64_t* o = stamps + 4ull * (blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64);
    o[0] = t0; o[1] = t1; o[2] = r0; o[3] = r1;
  }
}

typedef void (*Kern)(uint64_t*, uint32_t*);
template <int OP> static Kern kern_of() { return k_rate<OP>; }
template <int... OPS> struct KernTable { Kern k[sizeof...(OPS)] = {kern_of<OPS>()...}; };
template <int N, int... OPS> struct KernSeq : KernSeq<N - 1, N - 1, OPS...> {};
template <int... OPS> struct KernSeq<0, OPS...> { typedef KernTable<OPS...> T; };
static KernSeq<N_OPS>::T KERNS;
static Kern* const KERN = KERNS.k;

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main() {
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  const int cus = p.multiProcessorCount;
  const size_t lds = 96 * 1024;   // more than half a CU's LDS: one workgroup per CU
  uint64_t* d_st; uint32_t* d_sink;
  const int max_waves = cus * 16;
  CHECK(hipMalloc(&d_st, sizeof(uint64_t) * 4 * max_waves));
  CHECK(hipMalloc(&d_sink, sizeof(uint32_t) * 64 * max_waves));
  std::vector<uint64_t> st(4 * (size_t)max_waves);
  const double n_inst = (double)CHAINS * UNROLL * ITERS;
  for (int op = 0; op < N_OPS; op++) {
    CHECK(hipFuncSetAttribute((const void*)KERN[op], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int W = 1; W <= 4; W *= 2) {
      const int wpb = 4 * W;
      for (int rep = 0; rep < 2; rep++) {   // the second launch is the measurement
        hipLaunchKernelGGL(KERN[op], dim3(cus), dim3(64 * wpb), lds, 0, d_st, d_sink);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
      }
      CHECK(hipMemcpy(st.data(), d_st, sizeof(uint64_t) * 4 * cus * wpb, hipMemcpyDeviceToHost));
      std::vector<double> span, wave, mhz;
      for (int g = 0; g < cus; g++) {
        uint64_t lo = ~0ull, hi = 0;
        for (int w = 0; w < wpb; w++) {
          const uint64_t* o = &st[4 * ((size_t)g * wpb + w)];
          lo = std::min(lo, o[0]); hi = std::max(hi, o[1]);
          wave.push_back((double)(o[1] - o[0]));
          if (o[3] > o[2]) mhz.push_back((double)(o[1] - o[0]) / (double)(o[3] - o[2]) * 100.0);
        }
        span.push_back((double)(hi - lo));
      }
      printf("{\"inst\": \"%s\", \"waves_per_simd\": %d, \"inst_per_wave\": %.0f, \"cycles_per_inst_per_simd\": %.3f, "
             "\"cycles_per_inst_one_wave\": %.3f, \"shader_mhz\": %.0f, \"workgroups\": %d}\n",
             OP_NAME[op], W, n_inst, median(span) / (W * n_inst), median(wave) / n_inst, mhz.empty() ? 0.0 : median(mhz), cus);
      fflush(stdout);
    }
  }
  (void)hipFree(d_st); (void)hipFree(d_sink);
  return 0;
}
