// Stand-alone host check of the validator-set quorum logic (csrc/valset.h on top of csrc/quorum.h):
// the rules of the powers, the reference join by key bytes and by position, the double-vote scan
// and the reduction to commit verdicts and the set's code. Reads cases from the file named on the
// command line (written by tests/test_valset_abi.py from its random sets), evaluates each in
// exactly-sized heap arrays, so that one index too far is a sanitizer report, and prints one line
// of numbers per case for the test to compare with the Python model. Built with
// -fsanitize=address,undefined; ends with "ok <cases>" and exits 0.
//
// A case, whitespace-separated: m, m keys (64 hex digits each), m powers; nc, nc + 1 offsets; mode;
// form (0 key bytes, 1 positions); n keys or n positions; n flags; nc thresholds; n item codes.
// Its line: set_ok; then, if the set is accepted, args_ok; then, if the votes are accepted, pos[n]
// power[n] flag_out[n] checked[n] planned[nc] n_checked dv[nc] item_verdicts[n] tally[nc]
// commit_verdicts[nc] n_bad code.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "valset.h"

using namespace edc;

typedef std::vector<uint32_t> U32;
typedef std::vector<uint64_t> U64;
typedef std::vector<uint8_t> U8;

static U8 keys_of(std::istream& in, size_t count) {
  U8 out(32 * count);
  for (size_t j = 0; j < count; ++j) {
    std::string hex;
    in >> hex;
    if (hex.size() != 64) {
      fprintf(stderr, "bad key\n");
      exit(2);
    }
    for (size_t b = 0; b < 32; ++b) out[32 * j + b] = (uint8_t)strtoul(hex.substr(2 * b, 2).c_str(), nullptr, 16);
  }
  return out;
}

template <typename V>
static void put(const V& v) {
  for (auto x : v) std::cout << ' ' << (unsigned long long)x;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  size_t cases = 0, m;
  while (in >> m) {
    const U8 set_vk = keys_of(in, m);
    U64 set_power(m);
    for (uint64_t& p : set_power) in >> p;
    size_t nc;
    in >> nc;
    U32 off(nc + 1);
    for (uint32_t& o : off) in >> o;
    int mode, form;
    in >> mode >> form;
    const size_t n = off[nc];
    U8 vk;
    U32 key_idx;
    if (form == 0) {
      vk = keys_of(in, n);
    } else {
      key_idx.resize(n);
      for (uint32_t& x : key_idx) in >> x;
    }
    U8 flag(n), codes(n);
    U64 thr(nc);
    unsigned v;
    for (uint8_t& f : flag) { in >> v; f = (uint8_t)v; }
    for (uint64_t& t : thr) in >> t;
    for (uint8_t& c : codes) { in >> v; c = (uint8_t)v; }
    if (!in) {
      fprintf(stderr, "truncated case %zu\n", cases);
      return 2;
    }
    ++cases;
    const bool set_ok = m && valset_keys_distinct(m, set_vk.data()) && valset_check_powers(m, set_power.data());
    std::cout << (set_ok ? 1 : 0);
    if (!set_ok) {
      std::cout << '\n';
      continue;
    }
    U32 pos(n);
    U64 power(n);
    U8 flag_out(n);
    valset_resolve(m, set_vk.data(), set_power.data(), n, form == 0 ? vk.data() : nullptr, form == 0 ? nullptr : key_idx.data(),
                   flag.data(), pos.data(), power.data(), flag_out.data());
    const bool args_ok = quorum_check_mode(mode) && (!n || quorum_check_flags(n, flag.data())) &&
                         quorum_check_powers(nc, off.data(), n ? power.data() : nullptr, flag_out.data());
    std::cout << ' ' << (args_ok ? 1 : 0);
    if (!args_ok) {
      std::cout << '\n';
      continue;
    }
    U8 checked(n), dv(nc), item(n), cor(nc), verdicts(nc);
    U64 planned(nc), tally(nc);
    const size_t total = quorum_select(nc, off.data(), power.data(), flag_out.data(), thr.data(), mode, checked.data(), planned.data());
    const size_t ndv = valset_double_votes(nc, off.data(), pos.data(), checked.data(), dv.data());
    if (ndv != valset_double_votes(nc, off.data(), pos.data(), checked.data(), nullptr)) return 3;
    for (size_t i = 0; i < n; ++i) item[i] = checked[i] ? codes[i] : QUORUM_NOT_CHECKED;
    quorum_tally(nc, off.data(), power.data(), flag_out.data(), item.data(), tally.data(), cor.data());
    size_t bad = 0;
    const int code = valset_reduce(nc, cor.data(), tally.data(), thr.data(), dv.data(), verdicts.data(), &bad);
    if (code != valset_reduce(nc, cor.data(), tally.data(), thr.data(), dv.data(), nullptr, nullptr)) return 3;
    if (!ndv) {       // without a double vote the reduction is the quorum entries'
      U8 qv(nc);
      size_t qbad = 0;
      if (quorum_reduce(nc, cor.data(), tally.data(), thr.data(), qv.data(), &qbad) != code || qv != verdicts || qbad != bad) return 3;
      if (valset_reduce(nc, cor.data(), tally.data(), thr.data(), nullptr, qv.data(), &qbad) != code || qv != verdicts) return 3;
    }
    put(pos); put(power); put(flag_out); put(checked); put(planned);
    std::cout << ' ' << total;
    put(dv); put(item); put(tally); put(verdicts);
    std::cout << ' ' << bad << ' ' << code << '\n';
  }
  std::cout << "ok " << cases << '\n';
  return 0;
}
