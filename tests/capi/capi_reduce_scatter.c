/*
 * capi_reduce_scatter.c — mccsReduceScatter and the host ring ReduceScatter
 * as a plain C binding of include/mccs_hip.h sees them.  Syntax-checked with
 * gcc -std=c11 by tests/test_reduce_scatter_plan.py (never run: the GPU cases
 * are tests/test_gpu_reduce_scatter.py).
 */
#include <stdint.h>

#include "mccs_hip.h"

enum { NR = 2, RECVCOUNT = 1024 };

/* two ranks on host memory: rank r's block D is filled with (r + 1) * (D + 1) */
int host_known_answer(void) {
  static int32_t in[NR][NR * RECVCOUNT], out[NR][RECVCOUNT];
  const void *send[NR];
  void *recv[NR];
  for (int r = 0; r < NR; ++r) {
    for (int i = 0; i < NR * RECVCOUNT; ++i) in[r][i] = (r + 1) * (i / RECVCOUNT + 1);
    send[r] = in[r];
    recv[r] = out[r];
  }
  mccsResult_t rc = mccs_host_ring_reduce_scatter(NR, send, recv, RECVCOUNT, mccsInt32, mccsDevSum, 1, 96, 1 << 22, NULL);
  if (rc != mccsSuccess) return 1;
  for (int r = 0; r < NR; ++r)
    for (int i = 0; i < RECVCOUNT; ++i)
      if (out[r][i] != (r + 1) * NR * (NR + 1) / 2) return 1;
  return 0;
}

/* in place: rank r's result lands in its own block of its send buffer */
mccsResult_t device_in_place(mccsComm_t comm, int rank, float *buf, hipStream_t stream) {
  return mccsReduceScatter(buf, buf + (size_t)rank * RECVCOUNT, RECVCOUNT, mccsFloat32, mccsDevSum, comm, stream);
}
