// Host test of csrc/devbuf.h alone (tests/test_devbuf.py builds it with ASan + UBSan): the owners
// and the two growth helpers over a malloc-backed allocator that counts live allocations and can
// be told to fail the k-th one. Prints "ok <checks>" and exits 0, or the first failed check.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "devbuf.h"

using namespace devbuf;

struct FakeAlloc {
  typedef int err_t;
  static constexpr int ok = 0;
  static long live, live_host, calls, fail_at, syncs;   // fail_at: 1-based allocation to fail, 0 = none
  static int take(void** p, size_t bytes, long& n) {
    if (++calls == fail_at) return 7;
    *p = malloc(bytes);
    if (!*p) return 2;
    ++n;
    return 0;
  }
  static int dev_alloc(void** p, size_t bytes) { return take(p, bytes, live); }
  static int host_alloc(void** p, size_t bytes) { return take(p, bytes, live_host); }
  static void dev_free(void* p) { free(p); --live; }
  static void host_free(void* p) { free(p); --live_host; }
  static void arm(long k) { calls = 0; fail_at = k; }
};
long FakeAlloc::live = 0, FakeAlloc::live_host = 0, FakeAlloc::calls = 0, FakeAlloc::fail_at = 0, FakeAlloc::syncs = 0;

static long g_checks = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    ++g_checks;                                                   \
    if (!(c)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      return 1;                                                   \
    }                                                             \
  } while (0)

template <typename T> using D = DevBuf<T, FakeAlloc>;
template <typename T> using P = PinnedBuf<T, FakeAlloc>;

static int sync_ok() { ++FakeAlloc::syncs; return 0; }

// a group of five buffers of four element types, sized from one capacity like the slots' arrays
struct Group {
  size_t cap = 0;
  D<uint8_t> a;
  D<uint32_t> b;
  D<uint64_t> c;
  D<uint16_t> d;
  D<uint8_t> e;
  static constexpr int members = 5;
  template <typename Policy>
  int room(size_t need, Policy pol) {
    return grow_group(cap, need, pol, sync_ok, [&](size_t k) {
      return alloc_all(sized(a, k * 32), sized(b, k * 8), sized(c, k + 1), sized(d, k / 64 + 2), sized(e, 2 * k));
    });
  }
  bool empty() const { return !a && !b && !c && !d && !e && !a.cap() && !b.cap() && !c.cap() && !d.cap() && !e.cap(); }
  bool sized_for(size_t k) const {
    return a && b && c && d && e && a.cap() == k * 32 && b.cap() == k * 8 && c.cap() == k + 1 && d.cap() == k / 64 + 2 &&
           e.cap() == 2 * k;
  }
};

typedef size_t (*Policy)(size_t);
static const size_t kEdges[] = {0, 1, 1023, 1024, 1025, 4095, 4096, 4097};

// what the policies must give, written out independently of devbuf.h
static size_t want_item(size_t n) { return n < 1024 ? 1024 : n + n / 8; }
static size_t want_byte(size_t b) { return b < 4096 ? 4096 : b + b / 8; }
static size_t want_off(size_t x) { return x < 1024 ? 1024 : x + (x - 1) / 8; }   // m + 1 + m / 8 with x = m + 1
static size_t want_entry(size_t e) { return e + e / 8 + 1024; }
static size_t want_term(size_t t) { return t + t / 8 + 64; }
static size_t want_exact(size_t x) { return x; }

static int test_buf() {
  {
    D<uint32_t> x;
    CHECK(!x && x.get() == nullptr && x.cap() == 0);
    CHECK(x.alloc(0) == 0 && x && x.cap() == 1);          // the count == 0 -> 1 rule
    CHECK(FakeAlloc::live == 1);
    CHECK(x.alloc(10) == 0 && x.cap() == 10 && FakeAlloc::live == 1);   // alloc frees what it held
    x[9] = 5;
    uint32_t* raw = x;                                     // implicit conversion
    CHECK(raw == x.get() && raw[9] == 5 && *(x + 9) == 5);
    FakeAlloc::arm(1);
    CHECK(x.alloc(20) == 7 && !x && x.cap() == 0 && FakeAlloc::live == 0);   // empty after a failure
    FakeAlloc::arm(0);
    CHECK(x.alloc(3) == 0);
    x.reset();
    CHECK(!x && x.cap() == 0 && FakeAlloc::live == 0);
    x.reset();                                             // twice is harmless
    CHECK(FakeAlloc::live == 0);
  }
  {
    P<uint64_t> h;
    CHECK(h.alloc(3) == 0 && FakeAlloc::live_host == 1 && FakeAlloc::live == 0);
    h[2] = 1;
  }
  CHECK(FakeAlloc::live_host == 0);                        // the destructor frees
  {
    // moves: ownership travels, the source is empty, an assigned-over buffer is freed once
    D<uint8_t> x, y;
    CHECK(x.alloc(8) == 0 && y.alloc(16) == 0 && FakeAlloc::live == 2);
    uint8_t* px = x;
    D<uint8_t> z(std::move(x));
    CHECK(z.get() == px && z.cap() == 8 && !x && x.cap() == 0 && FakeAlloc::live == 2);
    y = std::move(z);
    CHECK(y.get() == px && y.cap() == 8 && !z && z.cap() == 0 && FakeAlloc::live == 1);
    D<uint8_t>& self = y;
    y = std::move(self);                                   // self-assignment keeps the buffer
    CHECK(y.get() == px && FakeAlloc::live == 1);
    y = D<uint8_t>();                                      // assigning an empty one frees
    CHECK(!y && FakeAlloc::live == 0);
  }
  CHECK(FakeAlloc::live == 0);
  return 0;
}

static int test_policies() {
  const struct { Policy got, want; } pol[] = {{item_cap, want_item}, {byte_cap, want_byte}, {off_cap, want_off},
                                              {entry_cap, want_entry}, {term_cap, want_term}, {exact_cap, want_exact}};
  for (const auto& p : pol)
    for (size_t n : kEdges) {
      if (p.got == off_cap && n == 0) continue;            // offsets of m >= 0 items: x = m + 1 >= 1
      CHECK(p.got(n) == p.want(n));
      // the single helper: a fresh buffer gets exactly the policy's capacity ...
      D<uint32_t> x;
      const long s0 = FakeAlloc::syncs;
      CHECK(grow(x, n, p.got, sync_ok) == 0 && x && x.cap() == (p.want(n) ? p.want(n) : 1));
      CHECK(FakeAlloc::syncs == s0 + 1);                   // synchronized before (re)allocating
      // ... need <= cap neither reallocates nor synchronizes, and the pointer stays
      uint32_t* before = x;
      FakeAlloc::arm(0);
      CHECK(grow(x, x.cap(), p.got, sync_ok) == 0 && x.get() == before && FakeAlloc::calls == 0);
      CHECK(grow(x, 0, p.got, sync_ok) == 0 && x.get() == before && FakeAlloc::calls == 0);
      CHECK(FakeAlloc::syncs == s0 + 1);
      // ... one more than the capacity regrows to the policy's value for that need
      const size_t more = x.cap() + 1;
      CHECK(grow(x, more, p.got, sync_ok) == 0 && x.cap() == p.want(more) && FakeAlloc::live == 1);
      // the group helper with the same policy
      Group g;
      CHECK(g.room(n, p.got) == 0);
      const size_t k = p.want(n);
      if (k) {
        CHECK(g.cap == k && g.sized_for(k) && FakeAlloc::live == 1 + Group::members);
        const uint8_t* ga = g.a;
        FakeAlloc::arm(0);
        CHECK(g.room(k, p.got) == 0 && g.a.get() == ga && g.cap == k && FakeAlloc::calls == 0);
        CHECK(g.room(k + 1, p.got) == 0 && g.cap == p.want(k + 1) && g.sized_for(p.want(k + 1)));
        CHECK(FakeAlloc::live == 1 + Group::members);
      }
    }
  CHECK(FakeAlloc::live == 0);
  CHECK(next_pow2(0) == 1 && next_pow2(1) == 1 && next_pow2(2048) == 2048 && next_pow2(2049) == 4096);
  return 0;
}

static int test_failures() {
  // single helper: a failed sync frees nothing and keeps the buffer; a failed allocation empties it
  {
    D<uint32_t> x;
    CHECK(grow(x, 10, item_cap, sync_ok) == 0 && x.cap() == 1024);
    uint32_t* before = x;
    CHECK(grow(x, 5000, item_cap, [] { return 3; }) == 3 && x.get() == before && x.cap() == 1024);
    FakeAlloc::arm(1);
    CHECK(grow(x, 5000, item_cap, sync_ok) == 7 && !x && x.cap() == 0 && FakeAlloc::live == 0);
    FakeAlloc::arm(0);
    CHECK(grow(x, 5000, item_cap, sync_ok) == 0 && x.cap() == want_item(5000));
  }
  // group helper: the k-th allocation of a growth fails, for every k, from an empty and from a
  // populated group; bystander buffers are untouched
  D<uint8_t> bystander;
  CHECK(bystander.alloc(4) == 0);
  for (int populated = 0; populated < 2; ++populated)
    for (long k = 1; k <= Group::members; ++k) {
      Group g;
      if (populated) CHECK(g.room(100, item_cap) == 0 && g.cap == 1024);
      const long before = FakeAlloc::live;
      FakeAlloc::arm(k);
      CHECK(g.room(2500, item_cap) == 7);
      FakeAlloc::arm(0);
      CHECK(g.empty() && g.cap == 0);
      CHECK(FakeAlloc::live == before - (populated ? Group::members : 0));
      CHECK(bystander && bystander.cap() == 4);
      CHECK(g.room(96, item_cap) == 0 && g.cap == 1024 && g.sized_for(1024));   // the next call starts clean
      CHECK(g.room(2500, item_cap) == 0 && g.cap == want_item(2500) && g.sized_for(want_item(2500)));
    }
  {
    // a failed sync leaves the group as it was
    Group g;
    CHECK(g.room(100, item_cap) == 0);
    const uint8_t* ga = g.a;
    CHECK(grow_group(g.cap, 5000, item_cap, [] { return 3; }, [](size_t) { return 0; }) == 3);
    CHECK(g.cap == 1024 && g.a.get() == ga && g.sized_for(1024));
  }
  bystander.reset();
  CHECK(FakeAlloc::live == 0 && FakeAlloc::live_host == 0);
  return 0;
}

int main() {
  if (test_buf() || test_policies() || test_failures()) return 1;
  if (FakeAlloc::live != 0 || FakeAlloc::live_host != 0) {
    printf("FAILED leak: %ld device, %ld pinned allocations live at exit\n", FakeAlloc::live, FakeAlloc::live_host);
    return 1;
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
