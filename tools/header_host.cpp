// The host side of tools/header_bench.py: the reference of csrc/hdrhash.h on one thread, behind one
// C entry point. Built by the bench with the host compiler; not part of libedc.so.
#include <chrono>

#include "hdrhash.h"

using namespace edc;

extern "C" {

// The roots of nh headers (out, nh x 32) and, with rules (with_rules != 0), their bad bytes under
// expect, the two version rules at (7, 2) and (8, 2) and the link rule at (4, 2); set_roots holds
// the validator-set root of every version, hashed by the caller outside the timed part (the header
// side is what is measured). seconds[0]: the roots alone; seconds[1]: roots and rules.
// Returns the number of bad headers.
size_t header_host_run(size_t nh, const uint32_t* leaf_off, const uint32_t* byte_off, const uint8_t* bytes,
                       const uint8_t* expect, const uint32_t* vals_ver, const uint32_t* next_ver, const uint32_t* link,
                       const uint8_t* set_roots, uint8_t* out, uint8_t* bad, double seconds[2]) {
  typedef std::chrono::steady_clock clk;
  const HdrSet s{nh, leaf_off, byte_off, bytes};
  const clk::time_point t0 = clk::now();
  for (size_t h = 0; h < nh; ++h) hdrhash_root(s, h, out + 32 * h);
  const clk::time_point t1 = clk::now();
  const HdrRules r{expect, vals_ver, 7, 2, next_ver, 8, 2, link, 4, 2, set_roots};
  const size_t n_bad = hdrhash_bind(s, r, bad, out);
  const clk::time_point t2 = clk::now();
  seconds[0] = std::chrono::duration<double>(t1 - t0).count();
  seconds[1] = std::chrono::duration<double>(t2 - t1).count();
  return n_bad;
}

}  // extern "C"
