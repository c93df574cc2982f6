// Stand-alone host check of the templated-message checks (csrc/tmpl.h): a valid set and items
// pass, each malformed case is refused, and the arena bound is the hand-computed value. Built with
// -fsanitize=address,undefined by tests/test_tmpl_abi.py; prints "ok" and exits 0.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "tmpl.h"

using namespace edc;

#define REQUIRE(c)                                              \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

int main() {
  // three templates: heads of 5, 0 and 17 bytes, tails of 3, 9 and 0 bytes
  std::vector<uint8_t> head(22, 0xAA), tail(12, 0xBB);
  std::vector<uint32_t> head_off = {0, 5, 5, 22}, tail_off = {0, 3, 12, 12};
  TmplShape sh;
  REQUIRE(tmpl_check_set(3, head.data(), head_off.data(), tail.data(), tail_off.data(), &sh));
  REQUIRE(sh.head_bytes == 22 && sh.tail_bytes == 12 && sh.max_head == 17 && sh.max_tail == 9);

  // items: holes of 4, 0, 7 and 1 bytes
  std::vector<uint16_t> tpl = {0, 2, 1, 2};
  std::vector<uint32_t> var_off = {0, 4, 4, 11, 12};
  REQUIRE(tmpl_check_items(3, 4, tpl.data(), var_off.data()));
  REQUIRE(tmpl_check_items(3, 0, nullptr, nullptr));

  // the bound: every item at its longest, the holes, and the 16 bytes of padding
  REQUIRE(tmpl_arena_bound(4, sh, 12) == 4 * (17 + 9) + 12 + 16);
  REQUIRE(tmpl_arena_bound(0, sh, 0) == 16);
  REQUIRE(TMPL_PAD == 16);

  // a template index equal to count
  {
    std::vector<uint16_t> t = tpl;
    t[3] = 3;
    REQUIRE(!tmpl_check_items(3, 4, t.data(), var_off.data()));
  }
  // a decreasing var_off
  {
    std::vector<uint32_t> o = {0, 4, 3, 11, 12};
    REQUIRE(!tmpl_check_items(3, 4, tpl.data(), o.data()));
  }
  // var_off[0] != 0
  {
    std::vector<uint32_t> o = {1, 4, 4, 11, 12};
    REQUIRE(!tmpl_check_items(3, 4, tpl.data(), o.data()));
  }
  // missing arrays
  REQUIRE(!tmpl_check_items(3, 4, nullptr, var_off.data()) && !tmpl_check_items(3, 4, tpl.data(), nullptr));
  // a blob over 1 MiB (the offsets alone decide: the bytes are never read by the check)
  {
    std::vector<uint32_t> o = {0, 5, 5, (1u << 20) + 1};
    REQUIRE(!tmpl_check_set(3, head.data(), o.data(), tail.data(), tail_off.data(), &sh));
    std::vector<uint32_t> h1 = {0, 1u << 19}, t1 = {0, (1u << 19) + 1}, t0 = {0, 1u << 19};
    REQUIRE(!tmpl_check_set(1, head.data(), h1.data(), tail.data(), t1.data(), &sh));
    REQUIRE(tmpl_check_set(1, head.data(), h1.data(), tail.data(), t0.data(), &sh));   // exactly 1 MiB
    REQUIRE(sh.max_head == (1u << 19) && sh.max_tail == (1u << 19));
  }
  // a non-monotone head_off
  {
    std::vector<uint32_t> o = {0, 5, 4, 22};
    REQUIRE(!tmpl_check_set(3, head.data(), o.data(), tail.data(), tail_off.data(), &sh));
  }
  // count out of range, missing offsets, bytes without a blob
  REQUIRE(!tmpl_check_set(0, head.data(), head_off.data(), tail.data(), tail_off.data(), &sh));
  REQUIRE(!tmpl_check_set(65536, head.data(), head_off.data(), tail.data(), tail_off.data(), &sh));
  REQUIRE(!tmpl_check_set(3, head.data(), nullptr, tail.data(), tail_off.data(), &sh));
  REQUIRE(!tmpl_check_set(3, nullptr, head_off.data(), tail.data(), tail_off.data(), &sh));
  // all heads and tails empty needs no blob at all
  {
    std::vector<uint32_t> z = {0, 0};
    REQUIRE(tmpl_check_set(1, nullptr, z.data(), nullptr, z.data(), &sh));
    REQUIRE(tmpl_arena_bound(5, sh, 0) == 16);
  }
  puts("ok");
  return 0;
}
