/*
 * capi_rooted.c — mccsBroadcast, mccsReduce and their host rings as a plain C
 * binding of include/mccs_hip.h sees them.  Syntax-checked with gcc -std=c11
 * by tests/test_rooted_plan.py (never run: the GPU cases are
 * tests/test_gpu_rooted.py).
 */
#include <stdint.h>

#include "mccs_hip.h"

enum { NR = 3, COUNT = 1024, ROOT = 1 };

/* three ranks on host memory: rank r's buffer is filled with r + 1 */
int host_known_answer(void) {
  static int32_t in[NR][COUNT], out[COUNT], copy[NR][COUNT];
  const void *send[NR];
  void *recv[NR];
  for (int r = 0; r < NR; ++r) {
    for (int i = 0; i < COUNT; ++i) in[r][i] = r + 1;
    send[r] = in[r];
    recv[r] = r == ROOT ? out : NULL; /* only the root's recvbuff is used */
  }
  if (mccs_host_ring_reduce(NR, send, recv, COUNT, mccsInt32, mccsDevSum, ROOT, 1, 96, 1 << 22, NULL) != mccsSuccess)
    return 1;
  for (int i = 0; i < COUNT; ++i)
    if (out[i] != NR * (NR + 1) / 2) return 1;
  for (int r = 0; r < NR; ++r) {
    send[r] = r == ROOT ? in[r] : NULL; /* only the root's sendbuff is read */
    recv[r] = copy[r];
  }
  if (mccs_host_ring_broadcast(NR, send, recv, sizeof(in[0]), ROOT, 1, 96, 1 << 22, NULL) != mccsSuccess) return 1;
  for (int r = 0; r < NR; ++r)
    for (int i = 0; i < COUNT; ++i)
      if (copy[r][i] != ROOT + 1) return 1;
  return 0;
}

/* parameter sync from rank 0, in place on the root; a metric reduced to rank 0 */
mccsResult_t device_calls(mccsComm_t comm, int rank, float *params, size_t nparams, float *metric, hipStream_t stream) {
  mccsResult_t rc = mccsBroadcast(rank == 0 ? params : NULL, params, nparams * sizeof(float), 0, comm, stream);
  if (rc != mccsSuccess) return rc;
  return mccsReduce(metric, rank == 0 ? metric : NULL, 1, mccsFloat32, mccsDevSum, 0, comm, stream);
}
