// Stand-alone host check of the template-variant checks of a templated commit set
// (csrc/commits.h, commits_check_alt_span and commits_check_item_alt): alt_span 0 / 1 / 256 / 257,
// a window that ends exactly at the set's count and one past it, empty commits with a base whose
// window leaves the set, a variant byte equal to alt_span - 1 and to alt_span, and a null
// item_alt. Built with -fsanitize=address,undefined by tests/test_commits_alt_abi.py; prints "ok"
// and exits 0.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "commits.h"

using namespace edc;

#define REQUIRE(c)                                              \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

int main() {
  // ---- alt_span and the windows (exactly-sized heap arrays: one index too far is a report) ----
  {
    std::vector<uint16_t> t = {0, 4, 0, 4};                      // two heights of 4 variants in a set of 8
    REQUIRE(!commits_check_alt_span(8, 4, t.data(), 0));         // span 0
    REQUIRE(commits_check_alt_span(8, 4, t.data(), 1));          // span 1: the one-template call
    REQUIRE(commits_check_alt_span(8, 4, t.data(), 4));          // the windows [0, 4) and [4, 8): exactly at count
    REQUIRE(!commits_check_alt_span(8, 4, t.data(), 5));         // [4, 9): one past it
    REQUIRE(!commits_check_alt_span(7, 4, t.data(), 4));
    REQUIRE(commits_check_alt_span(8, 1, t.data(), 8));          // only nc entries are read
    REQUIRE(!commits_check_alt_span(8, 2, t.data(), 8));
    REQUIRE(!commits_check_alt_span(8, 4, nullptr, 4));
  }
  {
    std::vector<uint16_t> z = {0, 0, 0};
    REQUIRE(commits_check_alt_span(256, 3, z.data(), 256));      // span 256 in a set of 256
    REQUIRE(!commits_check_alt_span(255, 3, z.data(), 256));
    REQUIRE(!commits_check_alt_span(65535, 3, z.data(), 257));   // span 257, however large the set
    REQUIRE(!commits_check_alt_span(65535, 3, z.data(), 0xFFFFFFFFu));
    std::vector<uint16_t> top = {65535 - 256, 65535 - 255};
    REQUIRE(commits_check_alt_span(65535, 1, top.data(), 256));  // the last window of the largest set
    REQUIRE(!commits_check_alt_span(65535, 2, top.data(), 256)); // no 16-bit wrap: 65280 + 256 > 65535
    std::vector<uint16_t> last = {65535};
    REQUIRE(!commits_check_alt_span(65535, 1, last.data(), 1));  // commit_tpl[c] == count
  }
  {
    // empty commits own a window too: their base is checked although no item uses it
    const std::vector<uint32_t> off = {0, 0, 3, 3};
    size_t n = 99;
    REQUIRE(commits_check_offsets(3, off.data(), &n) && n == 3);
    std::vector<uint16_t> first = {6, 0, 0}, lastc = {0, 0, 5}, ok = {4, 0, 4};
    REQUIRE(!commits_check_alt_span(8, 3, first.data(), 4));     // the empty first commit's window is [6, 10)
    REQUIRE(!commits_check_alt_span(8, 3, lastc.data(), 4));     // the empty last commit's is [5, 9)
    REQUIRE(commits_check_alt_span(8, 3, ok.data(), 4));
    REQUIRE(commits_check_alt_span(8, 0, nullptr, 4) == false);  // no commit_tpl at all
  }

  // ---- the variant bytes ----
  {
    std::vector<uint8_t> a = {0, 3, 1, 0, 2, 3, 0, 0, 3};        // nine items: more than one 8-byte group
    REQUIRE(commits_check_item_alt(9, a.data(), 4));             // alt == span - 1
    REQUIRE(!commits_check_item_alt(9, a.data(), 3));            // alt == span
    a[8] = 4;
    REQUIRE(!commits_check_item_alt(9, a.data(), 4));            // the last item of all
    REQUIRE(commits_check_item_alt(8, a.data(), 4));             // only n entries are read
    a[8] = 0;
    a[0] = 4;
    REQUIRE(!commits_check_item_alt(9, a.data(), 4));            // the first
    a[0] = 255;
    REQUIRE(!commits_check_item_alt(9, a.data(), 255) && commits_check_item_alt(9, a.data(), 256));
    std::vector<uint8_t> z(5, 0);
    REQUIRE(commits_check_item_alt(5, z.data(), 1));             // span 1: only zeros
    z[2] = 1;
    REQUIRE(!commits_check_item_alt(5, z.data(), 1));
    REQUIRE(!commits_check_item_alt(5, z.data(), 0));            // span 0 is never right
    REQUIRE(commits_check_item_alt(5, nullptr, 1) && commits_check_item_alt(5, nullptr, 256));   // null: all zeros
    REQUIRE(!commits_check_item_alt(5, nullptr, 0));
    REQUIRE(commits_check_item_alt(0, nullptr, 4) && commits_check_item_alt(0, z.data(), 4));    // no items
  }
  puts("ok");
  return 0;
}
