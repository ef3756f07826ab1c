// counters.hpp -- how the pipeline (groot_hip.hip) reaches the counters behind the order stage (counters.hip): report coverage, shared
// reads, equivalence classes, assigned coverage, pairing, and through counters.hip the rescue family (rescue.hip, rescue.hpp).  Their state is groot_ctx::ct and Slot::ct (ctx.hpp).
#pragma once

#include "groot_hip.h"

struct Slot;

namespace groot {

void counters_init(groot_ctx *c, const groot_index_view *v);   // open: the host's position tables (nothing on the device until a counter comes on)
int counters_assign(groot_ctx *c, Slot *s);                    // launch_order_stage: assignment rewrites slot s's records right behind the order stage's last scatter (no-op while off; Slot::ct.assigned is set by enqueue, for every batch)
int counters_launch(groot_ctx *c, Slot *s);                    // run_batch_async: the counting kernels of slot s's batch, behind its order stage on the tail stream
int counters_fetch(groot_ctx *c, Slot *s);                     // enqueue: the batch's status words, on the copy-out stream ahead of its DeviceCounters
int counters_collect(groot_ctx *c, Slot *s, bool redone);      // finish_counters: slow-path reads and table growth, while s still owns its records (redone: fetch's copies are stale)

} // namespace groot
