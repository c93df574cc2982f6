// Stand-alone host check of the validator-set history logic (csrc/vhist.h): the rules of
// edc_vhist_set, the change lists, the per-version totals and the reference lookup. Reads cases
// from the file named on the command line (written by tests/test_vhist_abi.py from its random
// histories), builds each from exactly-sized heap arrays, so that one index too far is a sanitizer
// report, and prints one line per case for the test to compare with the Python model. Built with
// -fsanitize=address,undefined; ends with "ok <cases>" and exits 0.
//
// A case, whitespace-separated: list_m, list_m key identities; m, m base powers; the number of
// update offsets (nv + 1, or 0) and the offsets; the number of updates given, their positions,
// their powers; q, q pairs (position, version) to look up.
// Its line: "0 <reason>" for a refused history, else 1 off[m+1] ver[] pow[] total[nv+1]
// members[nv+1] and the q powers.
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <vector>

#include "vhist.h"

using namespace edc;

typedef std::vector<uint32_t> U32;
typedef std::vector<uint64_t> U64;

template <typename V>
static V read_vec(std::istream& in) {
  size_t count;
  in >> count;
  V v(count);
  for (auto& x : v) in >> x;
  return v;
}

template <typename V>
static void put(const V& v) {
  for (auto x : v) std::cout << ' ' << (unsigned long long)x;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  size_t cases = 0;
  for (;;) {
    const U32 key_id = read_vec<U32>(in);
    if (!in) break;
    const U64 base = read_vec<U64>(in);
    const U32 upd_off = read_vec<U32>(in), upd_pos = read_vec<U32>(in);
    U64 upd_power(upd_pos.size());
    for (uint64_t& w : upd_power) in >> w;
    const U32 query = read_vec<U32>(in);        // 2 q numbers
    if (!in || (query.size() & 1)) {
      fprintf(stderr, "truncated case %zu\n", cases);
      return 2;
    }
    ++cases;
    VHist h;
    h.m = 77;                                    // a refusal leaves *out as it was
    const char* why = nullptr;
    const size_t nv = upd_off.empty() ? 0 : upd_off.size() - 1;
    const bool ok = vhist_build(key_id.size(), key_id.empty() ? nullptr : key_id.data(), base.size(),
                                base.empty() ? nullptr : base.data(), nv, upd_off.empty() ? nullptr : upd_off.data(),
                                upd_pos.empty() ? nullptr : upd_pos.data(), upd_power.empty() ? nullptr : upd_power.data(), &h,
                                &why);
    if (!ok) {
      if (!why || h.m != 77 || !h.off.empty()) return 3;
      std::cout << "0 " << why << '\n';
      continue;
    }
    if (h.m != base.size() || h.nv != nv || h.off.size() != base.size() + 1 || h.ver.size() != h.off.back() ||
        h.pow.size() != h.ver.size() || h.total.size() != nv + 1 || h.members.size() != nv + 1)
      return 3;
    // the lookup against a replay of the updates, at every position and version of a small history
    if (base.size() * (nv + 1) <= 4096) {
      U64 cur(base);
      for (size_t v = 0; v <= nv; ++v) {
        if (v)
          for (size_t j = upd_off[v - 1]; j < upd_off[v]; ++j) cur[upd_pos[j]] = upd_power[j];
        for (size_t p = 0; p < base.size(); ++p)
          if (vhist_power_at(h, (uint32_t)p, (uint32_t)v) != cur[p]) return 4;
      }
    }
    std::cout << 1;
    put(h.off); put(h.ver); put(h.pow); put(h.total); put(h.members);
    for (size_t j = 0; j < query.size(); j += 2) std::cout << ' ' << (unsigned long long)vhist_power_at(h, query[j], query[j + 1]);
    std::cout << '\n';
  }
  std::cout << "ok " << cases << '\n';
  return 0;
}
