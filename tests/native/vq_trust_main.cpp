// Stand-alone host check of the trusting pair's reference (csrc/vhist.h: vq_trust_check_versions,
// vq_trust_union, vq_trust_tally, vq_trust_reduce, vq_trust_code) on top of quorum_select and
// valset_reduce. Reads cases from the file named on the command line (written by
// tests/test_vq_trust_abi.py from its random commit sets), builds each from exactly-sized heap arrays,
// so that one index too far is a sanitizer report, and prints one line per case for the test to
// compare with its Python model. Built with -fsanitize=address,undefined; ends with "ok <cases>".
//
// A case, whitespace-separated, every array led by its length: nv; commit_off (nc + 1); trust_ver
// (nc); power_a, flag_a, power_b, flag_b (n each; side B's already absent where trust_ver is the
// sentinel); threshold_a, threshold_b (nc); mode; codes (n: the code every item would get); dv_a, dv_b (nc).
// Its line: versions_ok | side[n] | counts[4] | per side: tally[nc] verdicts[nc] n_bad code | pair code.
#include <stdio.h>

#include <fstream>
#include <iostream>
#include <vector>

#include "valset.h"
#include "vhist.h"

using namespace edc;

typedef std::vector<uint8_t> U8;
typedef std::vector<uint32_t> U32;
typedef std::vector<uint64_t> U64;

template <typename V>
static V read_vec(std::istream& in) {
  size_t count;
  in >> count;
  V v(count);
  for (auto& x : v) {
    unsigned long long t;
    in >> t;
    x = (typename V::value_type)t;
  }
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
    uint32_t nv;
    in >> nv;
    if (!in) break;
    const U32 off = read_vec<U32>(in), tver = read_vec<U32>(in);
    const U64 pa = read_vec<U64>(in);
    const U8 fa = read_vec<U8>(in);
    const U64 pb = read_vec<U64>(in);
    const U8 fb = read_vec<U8>(in);
    const U64 ta = read_vec<U64>(in), tb = read_vec<U64>(in);
    int mode;
    in >> mode;
    const U8 codes = read_vec<U8>(in), dva = read_vec<U8>(in), dvb = read_vec<U8>(in);
    if (!in) {
      fprintf(stderr, "truncated case %zu\n", cases);
      return 2;
    }
    ++cases;
    const size_t nc = off.size() - 1, n = off[nc];
    std::cout << (vq_trust_check_versions(nc, tver.data(), nv) ? 1 : 0);
    U8 ca(n), cb(n), side(n), seen(n);
    quorum_select(nc, off.data(), pa.data(), fa.data(), ta.data(), mode, ca.data(), nullptr);
    quorum_select(nc, off.data(), pb.data(), fb.data(), tb.data(), mode, cb.data(), nullptr);
    uint64_t counts[4];
    const size_t u = vq_trust_union(n, ca.data(), cb.data(), side.data(), counts);
    if (u != counts[3]) return 3;
    for (size_t i = 0; i < n; ++i) seen[i] = side[i] ? codes[i] : QUORUM_NOT_CHECKED;    // the union's item codes
    put(side);
    put(U64(counts, counts + 4));
    U64 tal_a(nc), tal_b(nc);
    U8 cor_a(nc), cor_b(nc), va(nc), vb(nc);
    vq_trust_tally(nc, off.data(), side.data(), 0, pa.data(), fa.data(), seen.data(), tal_a.data(), cor_a.data());
    vq_trust_tally(nc, off.data(), side.data(), 1, pb.data(), fb.data(), seen.data(), tal_b.data(), cor_b.data());
    size_t bad_a = 0, bad_b = 0;
    const int ra = valset_reduce(nc, cor_a.data(), tal_a.data(), ta.data(), dva.data(), va.data(), &bad_a);
    const int rb = vq_trust_reduce(nc, tver.data(), cor_b.data(), tal_b.data(), tb.data(), dvb.data(), vb.data(), &bad_b);
    put(tal_a);
    put(va);
    std::cout << ' ' << bad_a << ' ' << ra;
    put(tal_b);
    put(vb);
    std::cout << ' ' << bad_b << ' ' << rb << ' ' << vq_trust_code(ra, rb) << '\n';
  }
  std::cout << "ok " << cases << '\n';
  return 0;
}
