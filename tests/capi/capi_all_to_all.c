/*
 * capi_all_to_all.c — mccsAllToAll, its route inspection and the host helpers
 * as a plain C binding of include/mccs_hip.h sees them.  Syntax-checked with
 * gcc -std=c11 by tests/test_all_to_all_plan.py (never run: the GPU cases are
 * tests/test_gpu_all_to_all.py).
 */
#include <stdint.h>

#include "mccs_hip.h"

enum { NR = 3, B = 1000 };

/* three ranks on host memory over the two rings 0-1-2 and 0-2-1: one hop */
int host_known_answer(void) {
  static uint8_t in[NR][NR * B], out[NR][NR * B];
  static const int rings[2 * NR] = {0, 1, 2, 0, 2, 1};
  const void *send[NR];
  void *recv[NR];
  int hops = 0, m = 0, send_bid[NR * 2], recv_bid[NR * 2];
  if (mccs_alltoall_route(NR, 2, rings, 0, &hops, &m, send_bid, recv_bid) != mccsSuccess || hops != 1 || m != 1)
    return 1;
  for (int r = 0; r < NR; ++r) {
    for (int i = 0; i < NR * B; ++i) in[r][i] = (uint8_t)(31 * r + 7 * (i / B) + i % B);
    send[r] = in[r];
    recv[r] = out[r];
  }
  if (mccs_host_ring_all_to_all(NR, send, recv, B, 2, 96, 1 << 22, rings, 0) != mccsSuccess) return 1;
  for (int r = 0; r < NR; ++r)
    for (int s = 0; s < NR; ++s)
      for (int i = 0; i < B; ++i)
        if (out[r][s * B + i] != in[s][r * B + i]) return 1;
  return 0;
}

/* an expert-parallel exchange: tokens out, results back */
mccsResult_t device_calls(mccsComm_t comm, const void *tokens, void *inbox, void *outbox, size_t bytes_per_peer,
                          hipStream_t stream) {
  int route[2];
  mccsResult_t rc = mccsCommAllToAllRoute(comm, route);
  if (rc != mccsSuccess) return rc;
  rc = mccsAllToAll(tokens, inbox, bytes_per_peer, comm, stream);
  if (rc != mccsSuccess) return rc;
  return mccsAllToAll(inbox, outbox, bytes_per_peer, comm, stream);
}
