// Host check of ragen_amd/csrc/lean_turn.hpp and board_step.hpp's valid_slots (the cached Sokoban
// turn's action fetch and valid-byte vectors, both with K known at compile time).
//   1. action_addr<K> / action_bytes<K> against a byte-wise restatement: a [B, K] byte array placed
//      at every misalignment of its base, every row (so every byte shift 0..3), random bytes.  The
//      dwords addressed must be the ones load_actions_at (common.hpp) reads, restated here: never
//      before the row's first dword, never past the dword holding the row's last byte.
//   2. valid_slots<K> against board_step.hpp's own valid_bytes over the 64-bit slot range.
// Build + run: tests/test_lean_turn_cpu.py (g++ -O2).  Prints "ok <cases>" or the first mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "lean_turn.hpp"

namespace {

long g_cases = 0;

uint32_t dword_at(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}

template <int K>
bool check_actions(std::mt19937_64& rng) {
  constexpr int kRows = 37;  // b * K + mis runs through every shift for every K
  // the arena: a guard dword on both sides of the aligned span that holds the array
  std::vector<uint32_t> arena((kRows * K + 3 + 3) / 4 + 4);
  uint8_t* const a0 = reinterpret_cast<uint8_t*>(arena.data()) + 4;  // 4-aligned
  for (int rep = 0; rep < 200; ++rep) {
    for (auto& w : arena) w = (uint32_t)rng();
    for (uint32_t mis = 0; mis < 4; ++mis) {
      const uint8_t* acts = a0 + mis;  // the array's base, misaligned by `mis`
      const uint8_t* abase = acts - mis;
      for (uint32_t b = 0; b < (uint32_t)kRows; ++b) {
        const rmi::lean::ActionAddr ad = rmi::lean::action_addr<K>(b, mis);
        // load_actions_at's addressing, restated
        const uint32_t o = b * K + mis, o4 = o & ~3u, sh = o & 3u, last = (sh + K - 1) >> 2;
        const uint32_t w0 = o4, w1 = o4 + (last >= 1 ? 4u : 0u), w2 = o4 + 4u * (last >= 2 ? 2u : last);
        if (ad.o0 != w0 || ad.o1 != w1 || ad.o2 != w2 || ad.sh != sh) {
          printf("addr K=%d b=%u mis=%u: %u %u %u sh %u, want %u %u %u sh %u\n", K, b, mis, ad.o0, ad.o1, ad.o2, ad.sh,
                 w0, w1, w2, sh);
          return false;
        }
        // the footprint: inside the dwords that hold the row's bytes
        const uint32_t first_dw = (b * K + mis) & ~3u, last_dw = (b * K + mis + K - 1) & ~3u;
        const uint32_t offs[3] = {ad.o0, ad.o1, ad.o2};
        for (int i = 0; i < rmi::lean::ActionLoads<K>::kDwords; ++i)
          if (offs[i] < first_dw || offs[i] > last_dw) {
            printf("reach K=%d b=%u mis=%u load %d at %u outside [%u, %u]\n", K, b, mis, i, offs[i], first_dw, last_dw);
            return false;
          }
        // the loads the kernel issues for this K; the others are handed a poison value
        constexpr int kN = rmi::lean::ActionLoads<K>::kDwords;
        const uint32_t d0 = dword_at(abase + ad.o0);
        const uint32_t d1 = kN >= 2 ? dword_at(abase + ad.o1) : 0xDEADBEEFu;
        const uint32_t d2 = kN >= 3 ? dword_at(abase + ad.o2) : 0xDEADBEEFu;
        uint32_t lo, hi;
        rmi::lean::action_bytes<K>(d0, d1, d2, ad.sh, lo, hi);
        uint64_t want = 0;
        for (int k = 0; k < K; ++k) want |= (uint64_t)acts[b * K + k] << (8 * k);
        const uint64_t got = ((uint64_t)hi << 32) | lo;
        if (got != want) {
          printf("bytes K=%d b=%u mis=%u sh=%u: %016llx want %016llx\n", K, b, mis, sh, (unsigned long long)got,
                 (unsigned long long)want);
          return false;
        }
        ++g_cases;
      }
    }
  }
  return true;
}

template <int K>
bool check_valid(std::mt19937_64& rng) {
  for (int rep = 0; rep < 20000; ++rep) {
    uint64_t acts = rng();
    // mostly small ids and zeros, as the parser writes them; some arbitrary bytes
    if (rep % 4) {
      acts = 0;
      for (int k = 0; k < 8; ++k) acts |= (uint64_t)(rng() % 11) << (8 * k);
    }
    if (K < 8) acts &= (1ull << (8 * K)) - 1;
    for (int n_act = 0; n_act <= K; ++n_act) {
      const uint64_t range = n_act >= 8 ? ~0ull : (1ull << (8 * n_act)) - 1;
      const uint32_t xl = (uint32_t)acts, xh = (uint32_t)(acts >> 32);
      const uint32_t wl = rmi::bs::valid_bytes(xl, (uint32_t)range);
      const uint32_t wh = K > 4 ? rmi::bs::valid_bytes(xh, (uint32_t)(range >> 32)) : 0u;
      const rmi::bs::ValidSlots v = rmi::bs::valid_slots<K>(xl, xh, n_act);
      if (v.lo != wl || v.hi != wh) {
        printf("valid K=%d n_act=%d acts=%016llx: %08x %08x want %08x %08x\n", K, n_act, (unsigned long long)acts, v.lo,
               v.hi, wl, wh);
        return false;
      }
      ++g_cases;
    }
  }
  return true;
}

template <int K>
bool check_k(std::mt19937_64& rng) {
  return check_actions<K>(rng) && check_valid<K>(rng);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20251019);
  const bool ok = check_k<1>(rng) && check_k<2>(rng) && check_k<3>(rng) && check_k<4>(rng) && check_k<5>(rng) &&
                  check_k<6>(rng) && check_k<7>(rng) && check_k<8>(rng);
  if (!ok) return 1;
  printf("ok %ld\n", g_cases);
  return 0;
}
