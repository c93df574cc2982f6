// Stand-alone host check of the validator-set hashes (csrc/valhash.h: the SHA-256, the uvarint, the
// leaf, the order, the recursive root, the root of a history's version) and, compiled for the
// host, of the register-level SHA-256 the kernels use (csrc/sha256.h: key, leaf and node hashes),
// reduced level by level as the root kernel reduces. tests/test_valhash_host.py feeds it cases and
// compares what it prints with the model (tests/valhash_model.py).
//
// One case per line of the file named by argv[1]; hex strings, "-" for the empty one:
//   sha HEX              -> the digest
//   uv X                 -> the uvarint of X
//   root N (KEY POWER)*N -> the recursive root, then the level-wise root through sha256.h
//   hist M KEY*M BASE*M NV (CNT (POS POWER)*CNT)*NV -> the roots of versions 0..NV, powers as
//                           decimal, 18446744073709551615 for no member
// The last line printed is "ok <cases>".
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sha256.h"
#include "valhash.h"

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

static void key_words(const uint8_t* key, uint32_t kw[8]) {
  for (int j = 0; j < 8; ++j)
    kw[j] = (uint32_t)key[4 * j] | (uint32_t)key[4 * j + 1] << 8 | (uint32_t)key[4 * j + 2] << 16 | (uint32_t)key[4 * j + 3] << 24;
}

static std::string digest_hex(const uint32_t h[8]) {
  uint8_t b[32];
  for (int j = 0; j < 8; ++j) {
    const uint32_t w = sha256_bswap(h[j]);
    memcpy(b + 4 * j, &w, 4);            // a little-endian host, as the device is
  }
  return hex(b, 32);
}

// the root kernel's arithmetic on the host: rank by address through sha256_key32, order by
// (power descending, rank ascending), leaves and nodes through sha256_leaf / sha256_node, level by
// level with a lone last node promoted
static std::string levelwise_root(size_t n, const std::vector<std::vector<uint8_t>>& keys, const std::vector<uint64_t>& power) {
  uint32_t h[8];
  if (!n) {
    sha256_empty(h);
    return digest_hex(h);
  }
  std::vector<uint8_t> addrs(n * VALHASH_ADDR_BYTES);
  for (size_t p = 0; p < n; ++p) {
    uint32_t kw[8];
    key_words(keys[p].data(), kw);
    sha256_key32(kw, h);
    for (int j = 0; j < 5; ++j) {
      const uint32_t w = sha256_bswap(h[j]);
      memcpy(&addrs[p * VALHASH_ADDR_BYTES + 4 * j], &w, 4);
    }
  }
  std::vector<uint32_t> rank(n), order(n);
  valhash_rank(n, addrs.data(), rank.data());
  for (size_t p = 0; p < n; ++p) order[p] = (uint32_t)p;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return ~power[a] != ~power[b] ? ~power[a] < ~power[b] : rank[a] < rank[b];
  });
  std::vector<std::vector<uint32_t>> level(n, std::vector<uint32_t>(8));
  for (size_t i = 0; i < n; ++i) {
    uint32_t kw[8];
    key_words(keys[order[i]].data(), kw);
    sha256_leaf(kw, power[order[i]], level[i].data());
  }
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
    if (op == "sha") {
      std::string h;
      ss >> h;
      const std::vector<uint8_t> msg = unhex(h);
      uint8_t d[32];
      valhash_sha256(msg.data(), msg.size(), d);
      printf("%s\n", hex(d, 32).c_str());
    } else if (op == "uv") {
      unsigned long long x;
      ss >> x;
      uint8_t b[10];
      const size_t n = valhash_uvarint(x, b);
      printf("%s\n", hex(b, n).c_str());
    } else if (op == "root") {
      size_t n;
      ss >> n;
      std::vector<std::vector<uint8_t>> keys(n);
      std::vector<uint8_t> flat(n * 32);
      std::vector<uint64_t> power(n);
      std::vector<uint32_t> pos(n);
      for (size_t p = 0; p < n; ++p) {
        std::string k;
        unsigned long long w;
        ss >> k >> w;
        keys[p] = unhex(k);
        if (keys[p].size() != 32) return 3;
        memcpy(&flat[p * 32], keys[p].data(), 32);
        power[p] = w;
        pos[p] = (uint32_t)p;
      }
      uint8_t d[32];
      valhash_root_of(n, pos.data(), power.data(), flat.data(), d);
      printf("%s %s\n", hex(d, 32).c_str(), levelwise_root(n, keys, power).c_str());
    } else if (op == "hist") {
      size_t m, nv;
      ss >> m;
      std::vector<uint8_t> flat(m * 32);
      std::vector<uint32_t> ids(m);
      for (size_t p = 0; p < m; ++p) {
        std::string k;
        ss >> k;
        const std::vector<uint8_t> b = unhex(k);
        if (b.size() != 32) return 3;
        memcpy(&flat[p * 32], b.data(), 32);
        ids[p] = (uint32_t)p;
      }
      std::vector<uint64_t> base(m), upw;
      for (size_t p = 0; p < m; ++p) {
        unsigned long long w;
        ss >> w;
        base[p] = w;
      }
      ss >> nv;
      std::vector<uint32_t> off(1, 0), upos;
      for (size_t v = 0; v < nv; ++v) {
        size_t cnt;
        ss >> cnt;
        for (size_t j = 0; j < cnt; ++j) {
          unsigned long long p, w;
          ss >> p >> w;
          upos.push_back((uint32_t)p);
          upw.push_back(w);
        }
        off.push_back((uint32_t)upos.size());
      }
      VHist h;
      const char* why = nullptr;
      if (!vhist_build(m, ids.data(), m, base.data(), nv, off.data(), upos.data(), upw.data(), &h, &why)) {
        printf("refused %s\n", why);
      } else {
        // the addresses once for the whole history, as a caller hashing many versions would
        std::vector<uint8_t> addrs(m * VALHASH_ADDR_BYTES);
        for (size_t p = 0; p < m; ++p) valhash_addr(&flat[p * 32], &addrs[p * VALHASH_ADDR_BYTES]);
        std::string out;
        for (uint32_t v = 0; v <= h.nv; ++v) {
          uint8_t d[32], e[32];
          valhash_root(h, flat.data(), v, d);
          valhash_root(h, flat.data(), v, e, addrs.data());
          if (memcmp(d, e, 32)) return 4;
          out += (v ? " " : "") + hex(d, 32);
        }
        printf("%s\n", out.c_str());
      }
    } else {
      return 5;
    }
    ++cases;
  }
  printf("ok %zu\n", cases);
  return 0;
}
