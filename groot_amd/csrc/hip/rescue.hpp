// rescue.hpp -- what the counters behind the order stage (counters.hip) and the rescue family (rescue.hip: mismatch rescue, gapped rescue,
// their reads in the equivalence classes and in assigned coverage, rescued and gapped records) need of each other.  The family's state is
// part of groot_ctx::ct and Slot::ct (ctx.hpp); its part of the C ABI is in rescue.hip.
#pragma once

#include "ctx.hpp"

namespace groot {

struct SharedArgs;

// workgroups of a grid-stride launch over n items
inline uint32_t grid_for(uint32_t n) { return std::max<uint32_t>(1u, std::min<uint32_t>((n + kBlock - 1) / kBlock, 2048u)); }

// ---- rescue.hip, called by counters.hip ----
int rescue_launch(groot_ctx *c, Slot *s, const SharedArgs &sa, uint32_t tab);   // counters_launch: the family's kernels of slot s's batch on the tail stream; sa and tab (this batch's part of the set table) as counters_launch has just built them
int rescue_fetch(groot_ctx *c, Slot *s);                        // counters_fetch: the family's status words, on the copy-out stream
int rescue_collect_records(groot_ctx *c, Slot *s, bool redone); // counters_collect, ahead of ec_collect: the batch's rescued and gapped records into the slot's pinned memory
int rescue_collect_classes(groot_ctx *c, Slot *s, bool redone); // counters_collect, between ec_collect and acov_collect: the slow rescued and gap-rescued reads' bitmaps and logs into ec_host and acov_host
int rescue_acov_pairs_launch(groot_ctx *c, Slot *s, const SharedArgs &sa); // acov_launch, between acov_serial_paired_kernel and the count: the one-pass records of the fragments with a rescued mate
void rescue_acov_pairs_release(Counters &k);                    // groot_hip_acov_enable(0): the rescued mates leave assigned coverage over fragments (their rule in the classes stays)
void rescue_ec_release(Counters &k);                            // groot_hip_ec_enable(0), groot_hip_acov_enable(0): the family's reads leave the classes, and with them assigned coverage
int rescue_ec_reset(groot_ctx *c);                              // groot_hip_ec_reset: the counts of the family's reads in the classes start over
int rescue_acov_reset(groot_ctx *c);                            // groot_hip_acov_reset: the counts of the family's records in assigned coverage start over
int rescue_acov_dropped(groot_ctx *c);                          // groot_hip_acov_export, behind its drain: GROOT_E_NOSPACE when a record of the family found no room in the table
bool rescue_on(const groot_ctx *c);                             // groot_hip_assign_enable: mismatch rescue is on (it tells the unaligned reads by the records assignment rewrites)

// ---- counters.hip, called by rescue.hip ----
int acov_grow(groot_ctx *c, uint32_t factor);                   // groot_hip_rescue_acov_enable: min_slots of the assigned-coverage table

} // namespace groot
