// Stand-alone host check of the quorum commit-set logic (csrc/quorum.h): the flag, power-bound and
// per-commit sum checks (the overflow cases included), the reference selection in full and in light
// mode over the edge shapes of the device scan (commits around a tile of 256, one long commit, many
// tiny and empty commits, thresholds that equal a running sum exactly), the tally after a failed
// union and the reduction to commit verdicts. Every selection is compared with a second,
// differently written evaluation (per item, from scratch). Built with -fsanitize=address,undefined
// by tests/test_quorum_abi.py; prints "ok <checks>" and exits 0.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "commits.h"
#include "quorum.h"

using namespace edc;

static size_t g_checks = 0;

#define REQUIRE(c)                                              \
  do {                                                          \
    ++g_checks;                                                 \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

typedef std::vector<uint32_t> U32;
typedef std::vector<uint64_t> U64;
typedef std::vector<uint8_t> U8;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

static U32 offsets(const U32& sizes) {
  U32 off(1, 0);
  for (uint32_t s : sizes) off.push_back(off.back() + s);
  return off;
}

// item i of commit c is checked iff ... evaluated from scratch for every item (quadratic on purpose)
static bool naive_checked(const U32& off, const U64& power, const U8& flag, const U64& thr, int mode, size_t c, size_t i) {
  if (mode == QUORUM_FULL) return flag[i] == QUORUM_COMMIT || flag[i] == QUORUM_NIL;
  if (flag[i] != QUORUM_COMMIT) return false;
  unsigned __int128 before = 0;
  for (size_t j = off[c]; j < i; ++j)
    if (flag[j] == QUORUM_COMMIT) before += power[j];
  return before <= thr[c];
}

// exactly-sized heap arrays, so that one index too far is a sanitizer report
static void compare(const U32& off, const U64& power, const U8& flag, const U64& thr) {
  const size_t nc = off.size() - 1, n = off.back();
  REQUIRE(quorum_check_flags(n, flag.data()));
  REQUIRE(quorum_check_powers(nc, off.data(), power.data(), flag.data()));
  for (int mode = 0; mode < 2; ++mode) {
    U8 chk(n, 0xEE);
    U64 planned(nc, 0xEEEE);
    const size_t total = quorum_select(nc, off.data(), power.data(), flag.data(), thr.data(), mode, chk.data(), planned.data());
    size_t cnt = 0;
    for (size_t c = 0; c < nc; ++c) {
      uint64_t p = 0;
      for (size_t i = off[c]; i < off[c + 1]; ++i) {
        const bool want = naive_checked(off, power, flag, thr, mode, c, i);
        REQUIRE(chk[i] == (want ? 1 : 0));
        cnt += want;
        if (want && flag[i] == QUORUM_COMMIT) p += power[i];
      }
      REQUIRE(planned[c] == p);
    }
    REQUIRE(total == cnt);
    REQUIRE(quorum_select(nc, off.data(), power.data(), flag.data(), thr.data(), mode, nullptr, nullptr) == cnt);
    // all checked items verify: the tally kernel's sums are the plan
    U8 codes(n), cor(nc, 0xEE);
    for (size_t i = 0; i < n; ++i) codes[i] = chk[i] ? 0 : QUORUM_NOT_CHECKED;
    U64 tally(nc, 0xEEEE);
    quorum_tally(nc, off.data(), power.data(), flag.data(), codes.data(), tally.data(), cor.data());
    for (size_t c = 0; c < nc; ++c) REQUIRE(tally[c] == planned[c] && cor[c] == 0);
  }
}

static void random_votes(size_t n, U64& power, U8& flag, uint64_t pmax) {
  power.resize(n);
  flag.resize(n);
  for (size_t i = 0; i < n; ++i) {
    power[i] = rnd() % (pmax + 1);
    const uint64_t r = rnd() % 10;
    flag[i] = r == 0 ? QUORUM_ABSENT : r == 1 ? QUORUM_NIL : QUORUM_COMMIT;
  }
}

int main() {
  // ---- saturating addition ----
  REQUIRE(quorum_sat_add(1, 2) == 3);
  REQUIRE(quorum_sat_add(UINT64_MAX, 1) == UINT64_MAX);
  REQUIRE(quorum_sat_add(QUORUM_MAX_POWER, QUORUM_MAX_POWER) == UINT64_MAX - 1);
  REQUIRE(quorum_sat_add(1ull << 63, 1ull << 63) == UINT64_MAX);
  for (int t = 0; t < 200; ++t) {      // associative, also across the saturation
    const uint64_t a = rnd() >> (rnd() % 3), b = rnd() >> (rnd() % 3), c = rnd() >> (rnd() % 3);
    REQUIRE(quorum_sat_add(quorum_sat_add(a, b), c) == quorum_sat_add(a, quorum_sat_add(b, c)));
  }
  REQUIRE(quorum_check_mode(QUORUM_FULL) && quorum_check_mode(QUORUM_LIGHT) && !quorum_check_mode(2) && !quorum_check_mode(-1));

  // ---- flags ----
  {
    U8 f = {0, 1, 2, 2, 1, 0};
    REQUIRE(quorum_check_flags(f.size(), f.data()));
    REQUIRE(quorum_check_flags(0, nullptr));
    REQUIRE(!quorum_check_flags(3, nullptr));
    for (size_t at = 0; at < f.size(); ++at) {
      U8 g = f;
      g[at] = 3;
      REQUIRE(!quorum_check_flags(g.size(), g.data()));
      g[at] = 255;
      REQUIRE(!quorum_check_flags(g.size(), g.data()));
    }
  }

  // ---- power bounds and per-commit sums ----
  {
    const U32 off = offsets({0, 3, 0, 2});
    U8 flag = {1, 1, 1, 1, 1};
    U64 power = {QUORUM_MAX_POWER, 0, 0, 1, 2};
    REQUIRE(quorum_check_powers(4, off.data(), power.data(), flag.data()));     // a single power of 2^63 - 1
    power[1] = 1;                                                              // the commit's sum is 2^63
    REQUIRE(!quorum_check_powers(4, off.data(), power.data(), flag.data()));
    flag[1] = QUORUM_NIL;                                                      // ... but a nil vote is not counted
    REQUIRE(quorum_check_powers(4, off.data(), power.data(), flag.data()));
    flag[1] = QUORUM_ABSENT;
    REQUIRE(quorum_check_powers(4, off.data(), power.data(), flag.data()));
    power[1] = 1ull << 63;                                                     // a power above the bound, counted or not
    REQUIRE(!quorum_check_powers(4, off.data(), power.data(), flag.data()));
    power[1] = UINT64_MAX;
    REQUIRE(!quorum_check_powers(4, off.data(), power.data(), flag.data()));
    power = {QUORUM_MAX_POWER, 0, 0, QUORUM_MAX_POWER, 0};                      // two commits at the bound each
    flag = {1, 1, 1, 1, 1};
    REQUIRE(quorum_check_powers(4, off.data(), power.data(), flag.data()));
    const U32 none = offsets({0, 0});
    REQUIRE(quorum_check_powers(2, none.data(), nullptr, nullptr));
    REQUIRE(!quorum_check_powers(4, off.data(), nullptr, flag.data()));
  }
  {   // a sum that would wrap 64 bits several times over, spread over two tiles of 256
    const U32 off = offsets({100, 400, 10});
    U8 flag(510, 1);
    U64 power(510, 1);
    for (size_t i = 200; i < 400; ++i) power[i] = QUORUM_MAX_POWER / 64;
    REQUIRE(!quorum_check_powers(3, off.data(), power.data(), flag.data()));
    for (size_t i = 200; i < 400; ++i) power[i] = QUORUM_MAX_POWER / 512;
    REQUIRE(quorum_check_powers(3, off.data(), power.data(), flag.data()));
    power[255] = power[256] = (QUORUM_MAX_POWER >> 1) + 1;                      // 2^62 + 2^62 = 2^63 over a tile edge
    for (size_t i = 200; i < 400; ++i)
      if (i != 255 && i != 256) power[i] = 0;
    for (size_t i = 100; i < 200; ++i) power[i] = 0;
    for (size_t i = 400; i < 500; ++i) power[i] = 0;
    REQUIRE(!quorum_check_powers(3, off.data(), power.data(), flag.data()));
    power[256] -= 1;
    REQUIRE(quorum_check_powers(3, off.data(), power.data(), flag.data()));
  }

  // ---- selection: shapes around the device tile ----
  {
    U64 power, thr;
    U8 flag;
    for (const U32& sizes : {U32{255}, U32{256}, U32{257}, U32{513}, U32{255, 1, 256, 64, 64, 128, 257}, U32{1},
                             U32{0}, U32{0, 0, 5, 0, 0, 3, 0}}) {
      const U32 off = offsets(sizes);
      for (int rep = 0; rep < 3; ++rep) {
        random_votes(off.back(), power, flag, 1000);
        thr.clear();
        for (size_t c = 0; c + 1 < off.size(); ++c) {
          uint64_t T = 0;
          for (size_t i = off[c]; i < off[c + 1]; ++i) T += power[i];
          thr.push_back(rep == 0 ? 2 * T / 3 : rep == 1 ? 0 : T);          // 2/3, threshold 0, never reached
        }
        compare(off, power, flag, thr);
      }
    }
  }
  {   // one commit of 5,000: the quorum inside the third tile (item 600), and never
    const U32 off = offsets({5000});
    U64 power(5000, 3);
    U8 flag(5000, 1);
    compare(off, power, flag, U64{3 * 600});
    U8 chk(5000);
    REQUIRE(quorum_select(1, off.data(), power.data(), flag.data(), U64{3 * 600}.data(), QUORUM_LIGHT, chk.data(), nullptr) == 601);
    REQUIRE(chk[600] == 1 && chk[601] == 0);
    compare(off, power, flag, U64{3 * 5000});
    compare(off, power, flag, U64{UINT64_MAX});
  }
  {   // 600 commits of 0..5 items, empty first, last and runs of empty ones
    U32 sizes(600);
    for (uint32_t& s : sizes) s = (uint32_t)(rnd() % 6);
    sizes[0] = sizes[599] = sizes[300] = sizes[301] = sizes[302] = 0;
    const U32 off = offsets(sizes);
    U64 power, thr(600);
    U8 flag;
    random_votes(off.back(), power, flag, 9);
    for (uint64_t& t : thr) t = rnd() % 12;
    compare(off, power, flag, thr);
  }
  {   // the threshold equal to the running sum exactly: the next item is still checked
    const U32 off = offsets({4});
    const U64 power = {5, 5, 5, 5};
    const U8 flag = {1, 1, 1, 1};
    U8 chk(4);
    U64 planned(1);
    REQUIRE(quorum_select(1, off.data(), power.data(), flag.data(), U64{10}.data(), QUORUM_LIGHT, chk.data(), planned.data()) == 3);
    REQUIRE(chk[0] && chk[1] && chk[2] && !chk[3] && planned[0] == 15);
    REQUIRE(quorum_select(1, off.data(), power.data(), flag.data(), U64{9}.data(), QUORUM_LIGHT, chk.data(), planned.data()) == 2);
    REQUIRE(planned[0] == 10);
    REQUIRE(quorum_select(1, off.data(), power.data(), flag.data(), U64{0}.data(), QUORUM_LIGHT, chk.data(), planned.data()) == 1);
    REQUIRE(quorum_select(1, off.data(), power.data(), flag.data(), U64{20}.data(), QUORUM_LIGHT, chk.data(), planned.data()) == 4);
    REQUIRE(planned[0] == 20);           // a tally equal to the threshold is short, below
    compare(off, power, flag, U64{10});
  }
  {   // a single power of 2^63 - 1, zero powers, all-absent and all-nil commits
    const U32 off = offsets({1, 3, 2, 2});
    const U64 power = {QUORUM_MAX_POWER, 0, 0, 0, 7, 7, 7, 7};
    const U8 flag = {1, 1, 1, 1, 0, 0, 2, 2};
    compare(off, power, flag, U64{QUORUM_MAX_POWER - 1, 0, 0, 0});
    compare(off, power, flag, U64{UINT64_MAX, UINT64_MAX, UINT64_MAX, UINT64_MAX});
    U8 chk(8);
    REQUIRE(quorum_select(4, off.data(), power.data(), flag.data(), U64{0, 0, 0, 0}.data(), QUORUM_LIGHT, chk.data(), nullptr) == 4);
    REQUIRE(quorum_select(4, off.data(), power.data(), flag.data(), U64{0, 0, 0, 0}.data(), QUORUM_FULL, chk.data(), nullptr) == 6);
    REQUIRE(!chk[4] && !chk[5] && chk[6] && chk[7]);
  }

  // ---- tally after a failed union, and the verdicts ----
  {
    const U32 off = offsets({0, 3, 3, 2, 0, 2});
    const U64 power = {4, 4, 4, 4, 4, 4, 9, 9, 5, 5};
    const U8 flag = {1, 1, 1, 1, 2, 1, 1, 0, 0, 2};
    //               commit 1: one bad vote  commit 2: a bad nil vote  commit 3: fine  commit 5: nothing counted
    const U8 codes = {0, 1, 0, 0, 1, 0, 0, 255, 255, 0};
    U64 tally(5, 0xEE);
    U8 cor(5, 0xEE), v(5, 0xEE);
    quorum_tally(5, off.data(), power.data(), flag.data(), codes.data(), tally.data(), cor.data());
    REQUIRE(tally == (U64{0, 8, 8, 9, 0}));
    REQUIRE(cor == (U8{0, 1, 1, 0, 0}));
    size_t bad = 99;
    const U64 thr = {0, 7, 7, 8, 0};
    REQUIRE(quorum_reduce(5, cor.data(), tally.data(), thr.data(), v.data(), &bad) == 1);
    REQUIRE(v == (U8{3, 1, 1, 0, 3}) && bad == 4);       // invalid wins over short; empty and all-absent are short at threshold 0
    REQUIRE(quorum_reduce(5, nullptr, tally.data(), thr.data(), v.data(), &bad) == 3);
    REQUIRE(v == (U8{3, 0, 0, 0, 3}) && bad == 2);
    const U64 eq = {0, 8, 8, 9, 0};                      // a tally equal to the threshold is short
    REQUIRE(quorum_reduce(5, nullptr, tally.data(), eq.data(), v.data(), &bad) == 3);
    REQUIRE(v == (U8{3, 3, 3, 3, 3}) && bad == 5);
    REQUIRE(quorum_reduce(5, nullptr, tally.data(), eq.data(), nullptr, nullptr) == 3);
    const U64 t1 = {9}, th1 = {8};
    REQUIRE(quorum_reduce(1, nullptr, t1.data(), th1.data(), v.data(), &bad) == 0 && bad == 0 && v[0] == 0);
    REQUIRE(quorum_reduce(0, nullptr, nullptr, nullptr, nullptr, &bad) == 0 && bad == 0);
    const U8 multi = {2};                                // any non-zero code makes the commit invalid
    REQUIRE(quorum_reduce(1, multi.data(), t1.data(), th1.data(), v.data(), &bad) == 1 && v[0] == 1);
  }

  // ---- the offsets are the commit sets' ----
  {
    size_t n = 99;
    const U32 off = offsets({0, 2, 0});
    REQUIRE(commits_check_offsets(3, off.data(), &n) && n == 2);
  }

  printf("ok %zu\n", g_checks);
  return 0;
}
