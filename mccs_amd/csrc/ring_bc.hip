// ring_bc.hip — the Broadcast ring kernel: byte-typed like AllGather's, one
// kernel whose int8 element counts bytes.  No reference-named entry point (the
// reference declares mccsFuncBoadcast, devcomm.h:11, and ships no kernel).
#include "ring_kernel.h"

namespace mccs {
const void* ring_bc_kernel() { return (const void*)&ring_multi_kernel<mccsFuncBoadcast, mccsInt8, OpSum>; }
}  // namespace mccs

MCCS_RING_TU_ACCESSORS(bc)
