// K split of the 256-row GEMM kernels (gemm256v3.hip, gemm256f8.hip): the workspace layout and the producer / finisher hand-off.
// A cut tile's pieces 1 .. S-1 (producers) leave fp32 partial sums in slabs and raise one flag each; piece 0 (the finisher) waits for
// the flags, adds the slabs and resets the flags.  Hand-off per guide G16: write-through slab stores, vmcnt(0) in every wave, barrier,
// one relaxed agent-scope flag store; finisher: relaxed poll, one agent-scope acquire, barrier, plain loads.
#pragma once
#include "dk_common.h"

// Workspace: DK_KSPLIT_SLABS slabs of 256 x 256 fp32, then the flag region -- one flag per producer piece, zero between launches (the
// finishers reset theirs) -- whose word DK_KSPLIT_ERROR_WORD is the error word: sticky 1 once a finisher gave up waiting (the flags it
// waited for are still reset; the tile's result is wrong).  The flag region must be zero before the first launch.
constexpr int DK_KSPLIT_SLABS = 256;
constexpr int DK_KSPLIT_SLAB_FLOATS = 256 * 256;
constexpr size_t DK_KSPLIT_FLAGS_OFF = (size_t)DK_KSPLIT_SLABS * DK_KSPLIT_SLAB_FLOATS * 4;  // bytes
constexpr size_t DK_KSPLIT_FLAG_BYTES = 4096;
constexpr int DK_KSPLIT_ERROR_WORD = 512;  // index into the flag region
constexpr size_t DK_KSPLIT_WS_BYTES = DK_KSPLIT_FLAGS_OFF + DK_KSPLIT_FLAG_BYTES;

// 16-byte write-through (sc1) store: the slab reaches memory without an agent-scope release fence
__device__ __forceinline__ void dk_ksplit_store_b128(float* ptr, f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(ptr), "v"(v) : "memory");
}

// Raw accumulators, thread-linear: quad (nf, mf) of the thread at float offset toff (4 * thread index; 0 when the caller has added it to
// `slab`) sits at (nf * 8 + mf) * 2048 + toff -- one coalesced 16-byte store / load per thread and quad
template <int MF>
__device__ __forceinline__ void dk_ksplit_store_acc(float* slab, unsigned toff, const f32x4 (&acc)[4][MF]) {
#pragma unroll
  for (int nf = 0; nf < 4; ++nf)
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) dk_ksplit_store_b128(slab + (size_t)(nf * 8 + mf) * 2048 + toff, acc[nf][mf]);
}
template <int MF>
__device__ __forceinline__ void dk_ksplit_add_acc(f32x4 (&acc)[4][MF], const float* slab, unsigned toff) {
#pragma unroll
  for (int nf = 0; nf < 4; ++nf)
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      const f32x4 o = *(const f32x4*)(slab + (size_t)(nf * 8 + mf) * 2048 + toff);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[nf][mf][e] += o[e];
    }
}

// `leader()`: true in the one thread that handles the flags (evaluated where it is used: a value carried across the barriers costs a register)
// Cut tile t has n producers and the flags flags[t * n .. t * n + n): producer piece p (1 .. n) raises flags[t * n + p - 1].
// producer: every wave's slab stores have completed, then the leader raises the piece's flag
template <class Leader>
__device__ __forceinline__ void dk_ksplit_publish(unsigned* flags, int tile, int n, int piece, Leader leader) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (leader()) __hip_atomic_store(flags + tile * n + piece - 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// finisher: the leader waits for the n flags of the tile's producers (after 2^24 polls it sets the error word and goes on), then acquires
template <class Leader>
__device__ __forceinline__ void dk_ksplit_wait(unsigned* flags, int tile, int n, unsigned* error_word, Leader leader) {
  if (leader()) {
    for (int pp = 0; pp < n; ++pp) {
      unsigned spins = 0;
      while (__hip_atomic_load(flags + tile * n + pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
        __builtin_amdgcn_s_sleep(4);
        if (++spins > (1u << 24)) {
          __hip_atomic_store(error_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
}

// finisher, behind its slab reads: every wave has read them, then the leader resets the n flags
template <class Leader>
__device__ __forceinline__ void dk_ksplit_release(unsigned* flags, int tile, int n, Leader leader) {
  __syncthreads();
  if (leader())
    for (int pp = 0; pp < n; ++pp) __hip_atomic_store(flags + tile * n + pp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
