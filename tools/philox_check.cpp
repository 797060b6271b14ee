// philox_check.cpp — csrc/philox.hpp's host-callable Philox-4x32-10 against the Random123 known answers, as a stand-alone
// program for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/philox_check.cpp -o philox_check && ./philox_check
// Exit status 0 when every answer matches.
#include <cstdio>

#include "../afldm_amd/csrc/philox.hpp"

int main() {
  struct Case {
    uint32_t c[4], k[2], want[4];
  };
  const Case cases[] = {
      {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
      {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
      {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
  };
  int bad = 0;
  for (const Case& t : cases) {
    const afldm::philox_words r = afldm::philox4x32_10(t.c[0], t.c[1], t.c[2], t.c[3], t.k[0], t.k[1]);
    for (int j = 0; j < 4; ++j) bad += r.w[j] != t.want[j];
    std::printf("%08x %08x %08x %08x\n", r.w[0], r.w[1], r.w[2], r.w[3]);
  }
  // the seeded form: key (seed & 0xffffffff, seed >> 32), counter (group, ordinal, slot, 0)
  const long long seed = (long long)(((unsigned long long)0x299f31d0u << 32) | 0xa4093822u);
  const afldm::philox_words a = afldm::philox_seeded(seed, 7u, 3u, 1u);
  const afldm::philox_words b = afldm::philox4x32_10(7u, 3u, 1u, 0u, 0xa4093822u, 0x299f31d0u);
  for (int j = 0; j < 4; ++j) bad += a.w[j] != b.w[j];
  // every group of a sample's stream near the wrap of the group index, and the largest seed
  unsigned acc = 0;
  for (uint32_t g = 0xfffffff0u; g != 0x10u; ++g) acc ^= afldm::philox_seeded(0x7fffffffffffffffLL, g, 0xffffffffu, 2u).w[g & 3];
  std::printf("%s (%u mismatches, fold %08x)\n", bad ? "FAILED" : "ok", (unsigned)bad, acc);
  return bad ? 1 : 0;
}
