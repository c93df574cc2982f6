// Stand-alone host check of the commit-set checks and reduction (csrc/commits.h): valid offsets
// pass, every refused shape is refused, and the reduction from per-item codes to per-commit
// verdicts is right on empty commits, on empty first and last commits, on a bad item as the first
// and as the last item of a commit, for one commit and for no items. Built with
// -fsanitize=address,undefined by tests/test_commits_abi.py; prints "ok" and exits 0.
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

// exactly-sized heap arrays, so that one index too far is a sanitizer report
static std::vector<uint8_t> reduce(const std::vector<uint32_t>& off, const std::vector<uint8_t>& codes, size_t* bad) {
  const size_t nc = off.size() - 1;
  std::vector<uint8_t> v(nc, 0xEE);
  *bad = commits_reduce(nc, off.data(), codes.empty() ? nullptr : codes.data(), v.data());
  return v;
}

int main() {
  size_t n = 99, bad = 99;

  // ---- offsets ----
  {
    std::vector<uint32_t> off = {0, 0, 1, 151, 151, 158, 158};   // empty first, middle and last commits
    REQUIRE(commits_check_offsets(6, off.data(), &n) && n == 158);
    std::vector<uint32_t> one = {0, 7};
    REQUIRE(commits_check_offsets(1, one.data(), &n) && n == 7);
    std::vector<uint32_t> none = {0, 0, 0};                      // n = 0: two empty commits
    REQUIRE(commits_check_offsets(2, none.data(), &n) && n == 0);
    std::vector<uint32_t> big = {0, (1u << 28) - 1};
    REQUIRE(commits_check_offsets(1, big.data(), &n) && n == (1u << 28) - 1);
  }
  {
    std::vector<uint32_t> first = {1, 2, 3};                     // commit_off[0] != 0
    REQUIRE(!commits_check_offsets(2, first.data(), &n));
    std::vector<uint32_t> down = {0, 5, 4, 9};                   // a decreasing offset
    REQUIRE(!commits_check_offsets(3, down.data(), &n));
    std::vector<uint32_t> down_last = {0, 5, 9, 8};
    REQUIRE(!commits_check_offsets(3, down_last.data(), &n));
    std::vector<uint32_t> big = {0, 1u << 28};                   // n >= 2^28
    REQUIRE(!commits_check_offsets(1, big.data(), &n));
    std::vector<uint32_t> huge = {0, 10, 0xFFFFFFFFu};
    REQUIRE(!commits_check_offsets(2, huge.data(), &n));
    std::vector<uint32_t> ok = {0, 1};
    REQUIRE(!commits_check_offsets(0, ok.data(), &n));           // nc = 0 is the caller's case
    REQUIRE(!commits_check_offsets(1, nullptr, &n));
  }

  // ---- one template per commit ----
  {
    std::vector<uint16_t> t = {0, 3, 1, 3};
    REQUIRE(commits_check_tpl(4, 4, t.data()));
    REQUIRE(!commits_check_tpl(3, 4, t.data()));                 // commit_tpl[c] == count
    t[3] = 65535;
    REQUIRE(!commits_check_tpl(4, 4, t.data()));
    REQUIRE(commits_check_tpl(4, 3, t.data()));                  // only nc entries are read
    REQUIRE(!commits_check_tpl(4, 4, nullptr));
  }

  // ---- holes ----
  {
    std::vector<uint32_t> v = {0, 12, 12, 24};
    REQUIRE(commits_check_holes(3, v.data()));
    REQUIRE(commits_check_holes(0, nullptr));
    std::vector<uint32_t> first = {1, 12, 12, 24}, down = {0, 12, 11, 24};
    REQUIRE(!commits_check_holes(3, first.data()) && !commits_check_holes(3, down.data()));
    REQUIRE(!commits_check_holes(3, nullptr));
  }

  // ---- reduction ----
  {
    // commits: empty | 3 items | empty | 2 items | 1 item | empty
    const std::vector<uint32_t> off = {0, 0, 3, 3, 5, 6, 6};
    std::vector<uint8_t> codes(6, 0);
    std::vector<uint8_t> v = reduce(off, codes, &bad);
    REQUIRE(bad == 0 && v == std::vector<uint8_t>({0, 0, 0, 0, 0, 0}));
    codes[0] = 1;                                                // first item of commit 1
    v = reduce(off, codes, &bad);
    REQUIRE(bad == 1 && v == std::vector<uint8_t>({0, 1, 0, 0, 0, 0}));
    codes[0] = 0;
    codes[2] = 2;                                                // last item of commit 1 (a malformed key)
    v = reduce(off, codes, &bad);
    REQUIRE(bad == 1 && v == std::vector<uint8_t>({0, 1, 0, 0, 0, 0}));   // InvalidSignature, as Verifier::verify
    codes[2] = 0;
    codes[3] = 1;                                                // first item of commit 3: its neighbours stay Ok
    v = reduce(off, codes, &bad);
    REQUIRE(bad == 1 && v == std::vector<uint8_t>({0, 0, 0, 1, 0, 0}));
    codes[5] = 1;                                                // the last item of all
    codes[4] = 1;
    v = reduce(off, codes, &bad);
    REQUIRE(bad == 2 && v == std::vector<uint8_t>({0, 0, 0, 1, 1, 0}));
    // a passing launch has no codes: every commit Ok
    v = reduce(off, {}, &bad);
    REQUIRE(bad == 0 && v == std::vector<uint8_t>(6, 0));
    // the verdict array is optional
    REQUIRE(commits_reduce(6, off.data(), codes.data(), nullptr) == 2);
  }
  {
    const std::vector<uint32_t> one = {0, 4};                    // nc = 1
    std::vector<uint8_t> v = reduce(one, {0, 0, 0, 0}, &bad);
    REQUIRE(bad == 0 && v == std::vector<uint8_t>({0}));
    v = reduce(one, {0, 0, 0, 1}, &bad);
    REQUIRE(bad == 1 && v == std::vector<uint8_t>({1}));
    v = reduce(one, {1, 0, 0, 0}, &bad);
    REQUIRE(bad == 1 && v == std::vector<uint8_t>({1}));
    const std::vector<uint32_t> none = {0, 0, 0, 0};             // n = 0: three empty commits
    v = reduce(none, {}, &bad);
    REQUIRE(bad == 0 && v == std::vector<uint8_t>({0, 0, 0}));
    REQUIRE(commits_reduce(0, nullptr, nullptr, nullptr) == 0);  // nc = 0
  }
  puts("ok");
  return 0;
}
