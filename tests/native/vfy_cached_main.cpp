// Stand-alone host check of the cached verifier's bookkeeping (csrc/vfy_cached.h): offered / hit
// counts, the 2^32 - 1 bound of `origin`, the mode switch rule and the insert watermark. Built with
// -fsanitize=address,undefined by tests/test_verifier_cached_abi.py; prints "ok" and exits 0.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "vfy_cached.h"

using namespace edc;

#define REQUIRE(c)                                              \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

int main() {
  CachedState c;
  size_t a = 7, b = 7;
  // off: nothing is ever due, and the switch is allowed on a fresh verifier
  REQUIRE(!c.on && cached_can_switch(c, 0) && !cached_can_switch(c, 1));
  REQUIRE(!cached_insert_due(c, 10, &a, &b) && a == 7 && b == 7);
  c.on = true;

  // a model of the retained queue: origin[i] = offered position of retained item i
  std::vector<uint32_t> origin;
  uint64_t x = 0x9E3779B97F4A7C15ull;
  size_t retained = 0;
  for (int call = 0; call < 200; ++call) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    const size_t m = (size_t)((x >> 33) % 700);
    REQUIRE(cached_room(c, m));
    size_t miss = 0;
    const uint32_t base = (uint32_t)c.offered;
    for (size_t i = 0; i < m; ++i) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      if ((x >> 40) % 3 == 0) {
        origin.push_back(base + (uint32_t)i);
        ++miss;
      }
    }
    REQUIRE(!cached_offer(c, m, m + 1));          // refused and unchanged
    REQUIRE(c.offered == base);
    REQUIRE(cached_offer(c, m, miss));
    retained += miss;
    REQUIRE(c.offered - c.hits == retained && origin.size() == retained);
    REQUIRE(cached_can_switch(c, retained) == (c.offered == 0));
    if (call % 7 == 3) {                          // a verify that passed: insert what is new, once
      const bool due = cached_insert_due(c, retained, &a, &b);
      REQUIRE(due == (retained > c.inserted));
      if (due) {
        REQUIRE(a == c.inserted && b == retained && a < b);
        cached_insert_done(c, b);
      }
      REQUIRE(!cached_insert_due(c, retained, &a, &b));
    }
  }
  for (size_t i = 1; i < origin.size(); ++i) REQUIRE(origin[i - 1] < origin[i] && origin[i] < c.offered);

  // the bound of origin: offered may reach 2^32 - 1 and not pass it
  CachedState big;
  big.on = true;
  big.offered = 0xFFFFFFFFull - 5;
  REQUIRE(cached_room(big, 5) && !cached_room(big, 6) && !cached_room(big, (size_t)1 << 33));
  REQUIRE(cached_offer(big, 5, 5) && big.offered == 0xFFFFFFFFull && !cached_room(big, 1) && cached_room(big, 0));

  // reset: counts and watermark start over, the mode stays
  cached_reset(c);
  REQUIRE(c.on && c.offered == 0 && c.hits == 0 && c.inserted == 0 && cached_can_switch(c, 0));
  REQUIRE(cached_insert_due(c, 3, &a, &b) && a == 0 && b == 3);
  puts("ok");
  return 0;
}
