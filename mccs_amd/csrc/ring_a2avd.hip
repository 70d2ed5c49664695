// ring_a2avd.hip — the AllToAllvDev ring kernel: AllToAllv whose per-peer byte
// counts and displacements are read from a table in device memory when the
// kernel runs (ring_cfg.h MCCS_FUNC_ALLTOALLV_DEV), so a replayed graph takes
// the sizes of the moment.  run_elem resolves each element from the table
// (ring_walk.h a2avd_resolve) into the form ring_a2av.hip's elements have and
// then runs the same walk.  Byte-typed; the function id is the library's own.
#include "ring_kernel.h"

namespace mccs {
const void* ring_a2avd_kernel() {
  return (const void*)&ring_multi_kernel<MCCS_FUNC_ALLTOALLV_DEV, mccsInt8, OpSum>;
}
}  // namespace mccs

MCCS_RING_TU_ACCESSORS(a2avd)
