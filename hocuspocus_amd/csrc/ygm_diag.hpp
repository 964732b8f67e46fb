// ygm_diag.hpp -- stamps of the diagnostic build (libygm_diag.so, -DYGM_DIAG; never loaded by the product) for the merge
// kernels; without YGM_DIAG every macro is empty.  Included by ygm_kernels.hip alone, which exports the readers
// (ygm_diag_read, ygm_diag_ts_read, ygm_diag_sw_read; ygm_diag_ds_read for ygm_merge_lean.hpp's array).  The arrays are
// static: a device array is not shared across translation units without relocatable device code, so a second file
// that included this header would get copies and need readers of its own.
#pragma once
#ifdef YGM_DIAG
// shader-clock sums: [0, 8) k_merge_fast's phases (DIAG), [8, 16) k_merge_wave's (DIAGW), [16, 32) k_merge_big's counts
// and follow / spec times
static __device__ unsigned long long ygm_diag[32];
#define DIAG_T0 unsigned long long _dt = __builtin_amdgcn_s_memtime();
#define DIAG(i) do { if (threadIdx.x == 0) { unsigned long long _n = __builtin_amdgcn_s_memtime(); atomicAdd(&ygm_diag[i], _n - _dt); _dt = _n; } } while (0)
#define DIAGW(i) do { if ((threadIdx.x & 63) == 0) { unsigned long long _n = __builtin_amdgcn_s_memtime(); atomicAdd(&ygm_diag[8 + (i)], _n - _dt); _dt = _n; } } while (0)
// lean and large-document kernels: absolute stamps per document (no atomics): ygm_diag_ts[(d % 16384) * 8 + slot]
static __device__ unsigned long long ygm_diag_ts[16384 * 8];
// (s_memrealtime: the chip-wide 100 MHz clock, comparable across waves and XCDs)
#define DIAGL_T0 if (threadIdx.x == 0) ygm_diag_ts[(blockIdx.x & 16383u) * 8] = __builtin_amdgcn_s_memrealtime();
#define DIAGL(i) do { if (threadIdx.x == 0) ygm_diag_ts[(blockIdx.x & 16383u) * 8 + 1 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define DIAG_NOW() __builtin_amdgcn_s_memrealtime()
#define DIAG_PUT(i, v) do { if (threadIdx.x == 0) ygm_diag_ts[(blockIdx.x & 16383u) * 8 + (i)] = (v); } while (0)
#define DIAG_C(...) __VA_ARGS__
// lean kernel, per wave: shader cycles spent at the vmcnt(0) a document's first staging write sits behind (the
// prefetch chunks -- and, the counter being in order, the previous document's output stores), and in the whole
// persistent loop: ygm_diag_sw[wave * 2 + {0, 1}]
static __device__ unsigned long long ygm_diag_sw[16384 * 2];
#define DIAGSW_T0 unsigned long long _sw = 0; const unsigned long long _sl = __builtin_amdgcn_s_memtime();
#define DIAGSW_WAIT do { const unsigned long long _a = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0x0F70); _sw += __builtin_amdgcn_s_memtime() - _a; } while (0)
#define DIAGSW_END do { if (threadIdx.x == 0) { ygm_diag_sw[(blockIdx.x & 16383u) * 2] = _sw; ygm_diag_sw[(blockIdx.x & 16383u) * 2 + 1] = __builtin_amdgcn_s_memtime() - _sl; } } while (0)
// narrow lean kernel: documents that reached the fast parse [0], and of them those that took it with the five-byte
// client id built in [1] (tools/diag_idlen.py sets the counts against the corpus)
static __device__ unsigned long long ygm_diag_id5[2];
#define DIAG_ID5(on) do { if (threadIdx.x == 0) { atomicAdd(&ygm_diag_id5[0], 1ull); if (on) atomicAdd(&ygm_diag_id5[1], 1ull); } } while (0)
#else
#define DIAG_ID5(on)
#define DIAGSW_T0
#define DIAGSW_WAIT
#define DIAGSW_END
#define DIAGL_T0
#define DIAGL(i)
#define DIAG_NOW() 0ull
#define DIAG_PUT(i, v)
#define DIAG_C(...)
#define DIAGW(i)
#define DIAG_T0
#define DIAG(i)
#endif
