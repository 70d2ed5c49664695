// ring_sr.hip — the Send/Recv ring kernel: grouped point-to-point on the
// one-hop route.  A work element is an AllToAllv element with hops = 1 (ring_cfg.h
// MCCS_FUNC_SENDRECV): a send walk to the channel's successor and a receive
// walk from its predecessor, each of its own length, so the walk, the control
// wave and the step persistence are ring_a2av.hip's.  Which call becomes which
// element is the host's pairing rule (host/plan.cpp sendrecv_elements).
// Byte-typed; the function id is the library's own.
#include "ring_kernel.h"

namespace mccs {
const void* ring_sr_kernel() { return (const void*)&ring_multi_kernel<MCCS_FUNC_SENDRECV, mccsInt8, OpSum>; }
}  // namespace mccs

MCCS_RING_TU_ACCESSORS(sr)
