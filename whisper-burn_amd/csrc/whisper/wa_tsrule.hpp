// wa_tsrule.hpp -- the device code of the timestamp rule record (TsRule,
// wa_pick.hpp): the history update and the masks read from a record.  The one
// definition of both, included by the kernels that pick under the rules
// (wa_pick.hip) and by the beam search's top-k and merge (wa_beam.hip).
// HIP sources only.
#pragma once
#include <hip/hip_runtime.h>

#include "wa_pick.hpp"

namespace wa {

constexpr int kTsEOT = 50257;

// The rule record's history update: the one statement of rules c and d,
// shared by the bookkeeping kernel, the beam merge and the host
// (ts_rule_next).
__host__ __device__ inline TsRule ts_rule_step(const TsRule& r, int tok, int ts0, int V) {
  TsRule n;
  n.first = 0;
  n.penult = (r.first || r.last) ? 1 : 0;
  n.last = tok >= ts0 ? 1 : 0;
  n.t_last = n.last ? tok : r.t_last;
  n.ts_hi = V - 1;
  if (n.last && n.penult) {  // a closed pair (or a lone first timestamp): text next, no timestamp
    n.text_ok = 1;
    n.ts_lo = V;
  } else if (n.last) {  // text then a timestamp: its partner (>= it) or EOT
    n.text_ok = 0;
    n.ts_lo = n.t_last;
  } else {  // text: more text, or a timestamp past the last one
    n.text_ok = 1;
    n.ts_lo = n.t_last >= 0 ? n.t_last + 1 : ts0;
  }
  n.pad = 0;
  return n;
}

// Masks a-e for one id of a row: r = the record's (text_ok, ts_lo, ts_hi,
// first).  The one statement of the masks, shared by the fused pick, the
// stored-logits pick and the beam search's top-k.
__device__ __forceinline__ bool ts_masked(int id, int ts0, const int4& r, bool suppress_eot) {
  if (id >= ts0) return id < r.y || id > r.z;         // timestamps: the allowed range only (c, d, e)
  if (id > kTsEOT) return true;                       // the specials (b)
  if (id == kTsEOT) return suppress_eot || r.w != 0;  // a, and the first pick (e)
  return r.x == 0;                                    // text (c, e)
}

// Whether a suppress mask (wa_pick.hpp; nullable: a kernel argument, the test
// is wave-uniform) lists `id`.
__device__ __forceinline__ bool sup_masked(const uint32_t* __restrict__ sup, int id) {
  return sup && ((sup[id >> 5] >> (id & 31)) & 1u);
}

}  // namespace wa
