// Host-side bookkeeping of the eager verifier's folds (edc_vfy_begin_eager, include/edc.h): which
// queued items have their R term in the running point, and when the next fold is due. Plain C++
// with no HIP in it, so it can be compiled into a stand-alone host program.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace edc {

// fold granularity when edc_vfy_set_fold was not called (or called with 0); the sweep behind the
// value is in DESIGN.md ("Eager verifier") and profiles/verifier_eager_fold_sweep.log
constexpr size_t FOLD_DEFAULT_ITEMS = 131072;

struct FoldState {
  bool eager = false;     // a seed is committed for this block
  bool spent = false;     // a failed verify revealed a z-dependent point: nothing more under this seed
  size_t folded = 0;      // items [0, folded) are in the running point
  size_t min_items = 0;   // 0: FOLD_DEFAULT_ITEMS
  uint64_t folds = 0;     // folds since the last reset
};

inline size_t fold_min(const FoldState& f) { return f.min_items ? f.min_items : FOLD_DEFAULT_ITEMS; }

// After a queue call left n items queued: is a fold due, and over which range [*a, *b)?
inline bool fold_due(const FoldState& f, size_t n, size_t* a, size_t* b) {
  if (!f.eager || f.spent || n <= f.folded || n - f.folded < fold_min(f)) return false;
  *a = f.folded;
  *b = n;
  return true;
}

// The fold over [f.folded, b) was enqueued.
inline void fold_done(FoldState& f, size_t b) {
  f.folded = b;
  f.folds++;
}

// edc_verifier_reset: the block is over, the verifier leaves eager mode (the granularity stays).
inline void fold_reset(FoldState& f) {
  f.eager = f.spent = false;
  f.folded = 0;
  f.folds = 0;
}

}  // namespace edc
