// gm_digest.h -- launch wrappers of the state digest (gm_digest.hip), called by gm_host_digest.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gm_partial.h"
#include "gm_scaled.h"

#define GM_DG_ESTATE 1u  // status word: a stored state whose escape lists disagree with its cells
#define GM_DG_EID 2u     // status word: PARTIAL, a view entry whose id is outside [1, n]

// SCALED: rows[n] += the row words of this context's columns, state as of tick T (lists of parity T & 1).
// rows zeroed on st before; status is only ever OR-ed into.
hipError_t gm_launch_digest_table(const SState &s, int T, uint64_t *rows, uint32_t *status, hipStream_t st);
// SCALED: nodes[n], 0 outside this context's columns. fail_t: device [n], read on a join ramp only
// (the tick a crashed node last ran; nullptr otherwise).
hipError_t gm_launch_digest_nodes(const SState &s, int T, const int32_t *fail_t, uint64_t *nodes, hipStream_t st);
// PARTIAL: rows[nloc] (the views of parity T & 1, plain stores) and nodes[nloc]; either may be nullptr.
hipError_t gm_launch_digest_views(const PState &p, int T, uint64_t *rows, uint64_t *nodes, uint32_t *status,
                                  hipStream_t st);
// sums[0] += sum of fold(r0 + i, rows[i]), sums[1] += sum of fold(r0 + i, nodes[i]) over i < count
hipError_t gm_launch_digest_fold(const uint64_t *rows, const uint64_t *nodes, int count, int r0, uint64_t *sums,
                                 hipStream_t st);
