// Stand-alone host check of the header hashes: csrc/hdrhash.h (the recursive root over leaves of any
// length, the four rules) and, compiled for the host, the streaming leaf hash of csrc/sha256.h
// reduced level by level as the root kernel reduces. tests/test_header_host.py feeds it cases and
// compares what it prints with the model (tests/header_model.py).
//
// One case per line of the file named by argv[1]; hex strings, "-" for the empty one:
//   hdr SKIP N LEAF*N  -> the recursive root, then the level-wise root through sha256.h. The
//                         leaves lie back to back behind SKIP bytes, so SKIP moves every start; the
//                         level-wise side reads them from a heap array of exactly the whole words
//                         the library stages, so a read past them is an error of the sanitizer.
//   bind NH (N LEAF*N)*NH  E (- | HASH*NH)  then three times  (- | LEAFIDX POS ENTRY*NH)  for the
//                         vals, next and link rules, then NS ROOT*NS, the set roots by version
//                       -> the bad bytes as hex ("-" for none), n_bad, then the roots
// The last line printed is "ok <cases>".
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hdrhash.h"
#include "sha256.h"

using namespace edc;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return out;
}

static std::string hex(const uint8_t* p, size_t n) {
  static const char d[] = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s.push_back(d[p[i] >> 4]);
    s.push_back(d[p[i] & 15]);
  }
  return s;
}

static std::string digest_hex(const uint32_t h[8]) {
  uint8_t b[32];
  for (int j = 0; j < 8; ++j) {
    const uint32_t w = sha256_bswap(h[j]);
    memcpy(b + 4 * j, &w, 4);            // a little-endian host, as the device is
  }
  return hex(b, 32);
}

// headers read from the stream into one byte array with its offsets
struct Packed {
  std::vector<uint32_t> leaf_off{0}, byte_off{0};
  std::vector<uint8_t> bytes;
  void skip(size_t n) {                  // n bytes in front that belong to an empty first leaf's place
    bytes.assign(n, 0xEE);
    byte_off[0] = (uint32_t)n;
  }
  bool header(std::istringstream& ss) {
    size_t n;
    if (!(ss >> n)) return false;
    for (size_t j = 0; j < n; ++j) {
      std::string x;
      if (!(ss >> x)) return false;
      const std::vector<uint8_t> b = unhex(x);
      bytes.insert(bytes.end(), b.begin(), b.end());
      byte_off.push_back((uint32_t)bytes.size());
    }
    leaf_off.push_back((uint32_t)byte_off.size() - 1);
    return true;
  }
  HdrSet set() const { return HdrSet{leaf_off.size() - 1, leaf_off.data(), byte_off.data(), bytes.data()}; }
};

// the root kernel's arithmetic on the host: every leaf through sha256_leaf_stream from whole
// aligned words, then level by level through sha256_node with a lone last node promoted
static std::string levelwise_root(const Packed& p) {
  const size_t n = p.leaf_off[1];
  uint32_t h[8];
  if (!n) {
    sha256_empty(h);
    return digest_hex(h);
  }
  const size_t nw = (p.bytes.size() + 3) / 4;
  uint32_t* words = new uint32_t[nw ? nw : 1]();     // exactly the staged words, zero behind the last byte
  if (!p.bytes.empty()) memcpy(words, p.bytes.data(), p.bytes.size());
  std::vector<std::vector<uint32_t>> level(n, std::vector<uint32_t>(8));
  for (size_t j = 0; j < n; ++j) sha256_leaf_stream(words, p.byte_off[j], p.byte_off[j + 1], level[j].data());
  delete[] words;
  while (level.size() > 1) {
    std::vector<std::vector<uint32_t>> up((level.size() + 1) / 2, std::vector<uint32_t>(8));
    for (size_t j = 0; j < up.size(); ++j) {
      if (2 * j + 1 < level.size()) sha256_node(level[2 * j].data(), level[2 * j + 1].data(), up[j].data());
      else up[j] = level[2 * j];
    }
    level.swap(up);
  }
  return digest_hex(level[0].data());
}

// "-" or LEAF POS ENTRY*nh
static bool read_rule(std::istringstream& ss, size_t nh, bool* have, uint32_t* leaf, uint32_t* pos, std::vector<uint32_t>* e) {
  std::string first;
  if (!(ss >> first)) return false;
  *have = first != "-";
  if (!*have) return true;
  *leaf = (uint32_t)strtoul(first.c_str(), nullptr, 10);
  unsigned long x;
  if (!(ss >> x)) return false;
  *pos = (uint32_t)x;
  for (size_t h = 0; h < nh; ++h) {
    if (!(ss >> x)) return false;
    e->push_back((uint32_t)x);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  size_t cases = 0;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    std::string op;
    ss >> op;
    if (op == "hdr") {
      size_t skip;
      ss >> skip;
      Packed p;
      p.skip(skip);
      if (!p.header(ss)) return 3;
      uint8_t d[32];
      hdrhash_root(p.set(), 0, d);
      printf("%s %s\n", hex(d, 32).c_str(), levelwise_root(p).c_str());
    } else if (op == "bind") {
      size_t nh;
      ss >> nh;
      Packed p;
      for (size_t h = 0; h < nh; ++h)
        if (!p.header(ss)) return 3;
      std::string tok;
      ss >> tok;
      if (tok != "E") return 4;
      std::vector<uint8_t> expect;
      ss >> tok;
      bool have_e = tok != "-";
      for (size_t h = 0; have_e && h < nh; ++h) {
        if (h) ss >> tok;
        const std::vector<uint8_t> b = unhex(tok);
        if (b.size() != 32) return 4;
        expect.insert(expect.end(), b.begin(), b.end());
      }
      HdrRules r{};
      bool have[3];
      std::vector<uint32_t> e[3];
      if (!read_rule(ss, nh, &have[0], &r.vals_leaf, &r.vals_pos, &e[0]) ||
          !read_rule(ss, nh, &have[1], &r.next_leaf, &r.next_pos, &e[1]) ||
          !read_rule(ss, nh, &have[2], &r.link_leaf, &r.link_pos, &e[2]))
        return 5;
      size_t ns;
      if (!(ss >> ns)) return 5;
      std::vector<uint8_t> set_roots;
      for (size_t v = 0; v < ns; ++v) {
        ss >> tok;
        const std::vector<uint8_t> b = unhex(tok);
        if (b.size() != 32) return 5;
        set_roots.insert(set_roots.end(), b.begin(), b.end());
      }
      r.expect = have_e ? expect.data() : nullptr;
      r.vals_ver = have[0] ? e[0].data() : nullptr;
      r.next_ver = have[1] ? e[1].data() : nullptr;
      r.link = have[2] ? e[2].data() : nullptr;
      r.set_roots = set_roots.data();
      std::vector<uint8_t> bad(nh ? nh : 1), roots(nh ? nh * 32 : 1);
      const size_t n_bad = hdrhash_bind(p.set(), r, bad.data(), roots.data());
      std::string out = nh ? hex(bad.data(), nh) : "-";
      out += " " + std::to_string(n_bad);
      for (size_t h = 0; h < nh; ++h) out += " " + hex(roots.data() + 32 * h, 32);
      printf("%s\n", out.c_str());
    } else {
      return 6;
    }
    ++cases;
  }
  printf("ok %zu\n", cases);
  return 0;
}
