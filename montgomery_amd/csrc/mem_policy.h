// Cache policy of the streaming global accesses of the tree and sort kernels: one load and one store helper of 4, 8 or 16 bytes that
// take the policy at compile time.  MemPol::NT marks the access non-temporal (__builtin_nontemporal_load / _store: the `nt` bit of
// global_load / global_store on gfx950, still one instruction of the same width); the value moved is the same either way -- a policy
// says where the bytes are cached, never what they are.  Each stream of a kernel names its policy ONCE as a constexpr next to the
// kernel, with the measurement that decided it.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace msm {

enum class MemPol : int { DEFAULT = 0, NT = 1 };

// clang's non-temporal builtins want scalars or native vectors, HIP's uint2 / uint4 are structs around them
typedef uint32_t mem_v2 __attribute__((ext_vector_type(2)));
typedef uint32_t mem_v4 __attribute__((ext_vector_type(4)));

template <MemPol P>
__device__ __forceinline__ uint32_t mem_load4(const void* p) {
  if constexpr (P == MemPol::NT) return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
  else return *reinterpret_cast<const uint32_t*>(p);
}
template <MemPol P>
__device__ __forceinline__ uint2 mem_load8(const void* p) {
  if constexpr (P == MemPol::NT) {
    const mem_v2 v = __builtin_nontemporal_load(reinterpret_cast<const mem_v2*>(p));
    return make_uint2(v.x, v.y);
  } else return *reinterpret_cast<const uint2*>(p);
}
template <MemPol P>
__device__ __forceinline__ uint4 mem_load16(const void* p) {
  if constexpr (P == MemPol::NT) {
    const mem_v4 v = __builtin_nontemporal_load(reinterpret_cast<const mem_v4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
  } else return *reinterpret_cast<const uint4*>(p);
}

template <MemPol P>
__device__ __forceinline__ void mem_store4(void* p, uint32_t v) {
  if constexpr (P == MemPol::NT) __builtin_nontemporal_store(v, reinterpret_cast<uint32_t*>(p));
  else *reinterpret_cast<uint32_t*>(p) = v;
}
template <MemPol P>
__device__ __forceinline__ void mem_store8(void* p, uint2 v) {
  if constexpr (P == MemPol::NT) {
    mem_v2 w;
    w.x = v.x; w.y = v.y;
    __builtin_nontemporal_store(w, reinterpret_cast<mem_v2*>(p));
  } else *reinterpret_cast<uint2*>(p) = v;
}
template <MemPol P>
__device__ __forceinline__ void mem_store16(void* p, uint4 v) {
  if constexpr (P == MemPol::NT) {
    mem_v4 w;
    w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    __builtin_nontemporal_store(w, reinterpret_cast<mem_v4*>(p));
  } else *reinterpret_cast<uint4*>(p) = v;
}

}  // namespace msm
