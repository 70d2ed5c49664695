// ring_a2a.hip — the AllToAll ring kernel: byte-typed like AllGather's and
// Broadcast's, one kernel whose int8 element counts bytes (OpSum with one
// source is a copy).  The walk is ring_walk.h a2a_call, the route travels in
// each work element (ring_cfg.h MCCS_A2A_ROUTE).  No reference-named entry
// point: the reference has no all-to-all, and the function id is the
// library's own (MCCS_FUNC_ALLTOALL).
#include "ring_kernel.h"

namespace mccs {
const void* ring_a2a_kernel() { return (const void*)&ring_multi_kernel<MCCS_FUNC_ALLTOALL, mccsInt8, OpSum>; }
}  // namespace mccs

MCCS_RING_TU_ACCESSORS(a2a)
