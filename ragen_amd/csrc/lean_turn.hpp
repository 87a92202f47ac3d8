// lean_turn.hpp — the action fetch of the cached Sokoban turn (sokoban_cached_turn_kernel,
// sokoban.hip) with the slot count K known at compile time.
//
// load_actions_at (common.hpp) serves any K at run time: three clamped dword loads, the third in
// its own exec region, and two 64-bit shifts.  With K a constant the dword holding the row's last
// byte, (sh + K - 1) >> 2 for a row starting at byte sh of its first dword, is at most 0 for
// K == 1, 1 for K <= 5 and 2 for K <= 8, so the kernel issues one, two or three loads and the K
// bytes come out of one or two byte-align funnels (v_alignbyte_b32).  The dwords addressed are
// exactly those load_actions_at reads, clamped the same way: never one past the dword holding the
// row's last byte.
//
// The file also builds for the host (tests/native/lean_turn_driver.cpp checks the offsets and the
// assembly against a byte-wise restatement).
#pragma once
#include <stdint.h>

#include "board_step.hpp"

namespace rmi {
namespace lean {

// the low dword of ({hi, lo} >> 8 * sh), sh = 0..3 (v_alignbyte_b32)
RMI_BS_FN uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8u * (sh & 3u)));
#endif
}

// dword loads a row of K action bytes can need
template <int K>
struct ActionLoads {
  static_assert(K >= 1 && K <= 8, "1..8 action slots");
  static constexpr int kDwords = K <= 1 ? 1 : (K <= 5 ? 2 : 3);
};

// Byte offsets, from the 4-aligned base `actions - mis` (mis = actions & 3), of the dwords that
// hold row b of a [B, K] byte array, and the row's byte shift in the first of them.  o1 / o2 repeat
// the dword of the row's last byte when the row ends before them (load_actions_at's clamping).
struct ActionAddr {
  uint32_t o0, o1, o2, sh;
};
template <int K>
RMI_BS_FN ActionAddr action_addr(uint32_t b, uint32_t mis) {
  const uint32_t o = b * (uint32_t)K + mis;
  ActionAddr a;
  a.sh = o & 3u;
  const uint32_t last = (a.sh + (uint32_t)K - 1u) >> 2;  // 0..2
  a.o0 = o & ~3u;
  a.o1 = a.o0 + (last >= 1u ? 4u : 0u);
  a.o2 = a.o0 + 4u * (last >= 2u ? 2u : last);
  return a;
}

// The K bytes sh .. sh + K - 1 of d0 | d1 | d2 as two dwords (byte k of lo | hi << 32 = slot k), the
// bytes from K on zero.  d1 is read for K >= 2 and d2 for K >= 6 only: pass anything for the rest.
template <int K>
RMI_BS_FN void action_bytes(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t sh, uint32_t& lo, uint32_t& hi) {
  constexpr int kN = ActionLoads<K>::kDwords;
  lo = kN == 1 ? d0 >> (8u * (sh & 3u)) : align_bytes(d1, d0, sh);
  hi = K > 4 ? align_bytes(kN == 3 ? d2 : d1, d1, sh) : 0u;
  if (K < 4) lo &= (1u << (8 * (K & 3))) - 1u;
  if (K > 4 && K < 8) hi &= (1u << (8 * (K & 3))) - 1u;
}

}  // namespace lean
}  // namespace rmi
