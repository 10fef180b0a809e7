// kernarg.h — getting a kernel's argument records into registers in ONE scalar round trip.
//
// Left to itself the compiler fetches every field of a by-value argument struct where it is first used: a kernel that picks its
// problem record at run time (gemm_mfma.h, ops.hip, dw_adam.hip) started with 7-14 DEPENDENT s_load / s_waitcnt pairs — the fused
// optimiser launch spent 2.2 us there before its first operand request (round 5, tools/scalar_front.py counts them).  GCRL_PIN(x)
// makes x an input of an empty volatile asm: the value must be in a scalar register HERE, so the loads of everything pinned in a row
// are issued together and waited for once; the later uses are the same SSA values (a pointer stays a kernel-argument pointer, i.e.
// global memory: laundering it through an asm OUTPUT would turn its accesses into flat ones).
#pragma once

#define GCRL_PIN(x) asm volatile("" ::"s"(x))

// Every 64-byte line of the kernel's argument segment requested at once (scalar loads, one wait): afterwards the lines sit in the
// CU's scalar cache, which starts every launch empty.  For kernels that read hundreds of argument fields all along a dependent
// chain (rowchain.hip: 207 s_loads in ~110 groups; each first touch of a line was a trip to the L2 or beyond, ~0.3-1 us, in the
// middle of the chain).  BYTES: size of the kernel's (single, by-value) argument struct.
//
// kernarg_warm() folds the lines' first dwords into ONE value: the compiler forms that value eight loads at a time and waits after
// each eight — a 1.8 KB argument struct is warmed in FOUR round trips, one behind the other.  kernarg_warm_once() holds every
// line's dword in a register of its own at one point of the program (up to 32 lines, 2 KB): all loads are issued, then ONE wait.
__device__ __forceinline__ void kernarg_hold16(const unsigned int (&w)[32], int i) {
  asm volatile("" ::"s"(w[i]), "s"(w[i + 1]), "s"(w[i + 2]), "s"(w[i + 3]), "s"(w[i + 4]), "s"(w[i + 5]), "s"(w[i + 6]), "s"(w[i + 7]), "s"(w[i + 8]),
               "s"(w[i + 9]), "s"(w[i + 10]), "s"(w[i + 11]), "s"(w[i + 12]), "s"(w[i + 13]), "s"(w[i + 14]), "s"(w[i + 15]));
}
template <int BYTES>
__device__ __forceinline__ void kernarg_warm_once() {
  static_assert(BYTES <= 32 * 64, "at most 32 lines");
  typedef const unsigned int __attribute__((address_space(4))) cu32;
  cu32* kp = (cu32*)__builtin_amdgcn_kernarg_segment_ptr();
  constexpr int N = (BYTES + 63) / 64;
  unsigned int w[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) w[i] = kp[16 * (i < N ? i : N - 1)];
  kernarg_hold16(w, 0);
  kernarg_hold16(w, 16);
}

template <int BYTES>
__device__ __forceinline__ void kernarg_warm() {
  typedef const unsigned int __attribute__((address_space(4))) cu32;
  cu32* kp = (cu32*)__builtin_amdgcn_kernarg_segment_ptr();
  unsigned int acc = 0;
#pragma unroll
  for (int i = 0; i < BYTES / 4; i += 16) acc |= kp[i];
  asm volatile("" ::"s"(acc));
}
