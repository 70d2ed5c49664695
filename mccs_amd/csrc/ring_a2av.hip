// ring_a2av.hip — the AllToAllv ring kernel: per-peer byte counts on the
// one-hop route.  Byte-typed like AllToAll's (int8 counts bytes; OpSum with
// one source is a copy).  The walk is ring_walk.h a2av_next: a send walk and a
// receive walk of their own lengths per work element (ring_cfg.h
// MCCS_FUNC_ALLTOALLV).  The function id is the library's own.
#include "ring_kernel.h"

namespace mccs {
const void* ring_a2av_kernel() { return (const void*)&ring_multi_kernel<MCCS_FUNC_ALLTOALLV, mccsInt8, OpSum>; }
}  // namespace mccs

MCCS_RING_TU_ACCESSORS(a2av)
