// The host side of tools/valhash_bench.py: the reference of csrc/valhash.h on one thread, behind
// two C entry points. Built by the bench with the host compiler; not part of libedc.so.
#include <chrono>

#include "valhash.h"

using namespace edc;

extern "C" {

// The roots of every version 0..nv of a history over m keys (32 bytes each, by position), out =
// (nv + 1) x 32 bytes. The history's change lists are built first and not timed (edc_vhist_set
// builds the same lists before the device sees them). seconds[0]: the m addresses, once;
// seconds[1]: per version the lookups, the sort, the leaves and the recursive root.
// 0, or -1 if vhist_build refuses the history.
int valhash_host_roots(size_t m, const uint8_t* keys, const uint64_t* base, size_t nv, const uint32_t* upd_off,
                       const uint32_t* upd_pos, const uint64_t* upd_power, uint8_t* out, double seconds[2]) {
  typedef std::chrono::steady_clock clk;
  std::vector<uint32_t> ids(m);
  for (size_t p = 0; p < m; ++p) ids[p] = (uint32_t)p;
  VHist h;
  if (!vhist_build(m, ids.data(), m, base, nv, upd_off, upd_pos, upd_power, &h, nullptr)) return -1;
  const clk::time_point t0 = clk::now();
  std::vector<uint8_t> addrs(m * VALHASH_ADDR_BYTES);
  for (size_t p = 0; p < m; ++p) valhash_addr(keys + p * 32, &addrs[p * VALHASH_ADDR_BYTES]);
  const clk::time_point t1 = clk::now();
  for (uint32_t v = 0; v <= h.nv; ++v) valhash_root(h, keys, v, out + (size_t)32 * v, addrs.data());
  const clk::time_point t2 = clk::now();
  seconds[0] = std::chrono::duration<double>(t1 - t0).count();
  seconds[1] = std::chrono::duration<double>(t2 - t1).count();
  return 0;
}

}  // extern "C"
