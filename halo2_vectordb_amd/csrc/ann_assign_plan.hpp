// The tile plan of the fused assign (k_ann_assign, witness.hip; include/vdb.h vdb_ann_assign_dev): everything the driver decides before it
// touches a pointer — the tile of rows a workgroup owns, the chunk of centroids it walks, the chunk of the dim axis it stages, the LDS
// bytes, the grid and the refusals — in a header of its own, with no HIP runtime call and no allocation, as ntt_plan.hpp and
// msm_plan.hpp are, so that vdb_ann_assign_plan hands the very plan the driver launches with to tests/test_ann_assign_plan_cpu.py.
// What the kernel and the planner must agree on is defined here once.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vdb {

// A workgroup of ANN_ASSIGN_THREADS lanes holds R x C (row, centroid) pairs, ANN_ASSIGN_PAIRS a lane: lane t owns centroid t % C of the
// chunk and rows t / C + p (ANN_ASSIGN_THREADS / C), p < ANN_ASSIGN_PAIRS.  C is a power of two at most 64, so the C lanes of a row lie
// in one wavefront (the fold is a butterfly over them) and read one broadcast address of the row tile.
#define ANN_ASSIGN_THREADS 256
#define ANN_ASSIGN_PAIRS 4
#define ANN_ASSIGN_C_MAX 64
#define ANN_ASSIGN_C_MIN 16
#define ANN_ASSIGN_R_MAX (ANN_ASSIGN_THREADS * ANN_ASSIGN_PAIRS / ANN_ASSIGN_C_MIN)
#define ANN_ASSIGN_DC 16   // words of the dim axis staged at a time
// 32-byte words of LDS: the stage ((R + C) DC, at most (64 + 16) DC), reused for the R C = 1,024 sums of a chunk between head and tail
#define ANN_ASSIGN_STAGE_WORDS ((ANN_ASSIGN_R_MAX + ANN_ASSIGN_C_MIN) * ANN_ASSIGN_DC)
static_assert(ANN_ASSIGN_STAGE_WORDS >= ANN_ASSIGN_THREADS * ANN_ASSIGN_PAIRS, "the sums of a chunk reuse the stage");

// The return codes of ann_assign_plan: VDB_OK and VDB_ERR_ARG of include/vdb.h (witness.hip asserts the equality).
constexpr int ANN_ASSIGN_PLAN_OK = 0, ANN_ASSIGN_PLAN_REFUSED = -3;
constexpr size_t ANN_ASSIGN_LDS_MAX = 160 * 1024;   // what one CU has
constexpr size_t ANN_ASSIGN_MAX_ROWS = 0xffffffffull, ANN_ASSIGN_MAX_K = (size_t)1 << 24, ANN_ASSIGN_MAX_DIM = (size_t)1 << 24;

struct AnnAssignPlan {
  uint32_t R, C, DC;        // rows of a workgroup's tile, centroids of a chunk, words of a dim chunk
  uint32_t chunks, dchunks; // ceil(K / C), ceil(dim / DC)
  uint32_t grid;            // workgroups: ceil(n / R); workgroup b owns rows [b R, min(n, (b + 1) R))
  uint32_t lds_bytes;       // the stage, the running minimum and its index per row of the tile
  uint64_t work_bytes;      // device work space: the norms of the n rows and K centroids (cosine alone), 0 otherwise
};

// C follows K so that an index of few centroids does not idle most lanes: the smallest of 16, 32, 64 that holds K, 64 beyond.  R takes
// what is left of the workgroup's R C = 1,024 pairs; DC is the stage's depth, cut to dim where dim is shorter.
static inline int ann_assign_plan(size_t n, size_t K, size_t dim, bool cosine, AnnAssignPlan* p, const char** why) {
  if (n == 0 || K == 0 || dim == 0) {
    *why = "ann assign: no row, no centroid or dim = 0";
    return ANN_ASSIGN_PLAN_REFUSED;
  }
  if (n > ANN_ASSIGN_MAX_ROWS || K > ANN_ASSIGN_MAX_K || dim > ANN_ASSIGN_MAX_DIM) {
    *why = "ann assign: n at most 2^32 - 1, K and dim at most 2^24";
    return ANN_ASSIGN_PLAN_REFUSED;
  }
  uint32_t C = ANN_ASSIGN_C_MIN;
  while (C < ANN_ASSIGN_C_MAX && C < K) C *= 2;
  p->C = C;
  p->R = ANN_ASSIGN_THREADS * ANN_ASSIGN_PAIRS / C;
  p->DC = dim < ANN_ASSIGN_DC ? (uint32_t)dim : ANN_ASSIGN_DC;
  p->chunks = (uint32_t)((K + C - 1) / C);
  p->dchunks = (uint32_t)((dim + p->DC - 1) / p->DC);
  p->grid = (uint32_t)((n + p->R - 1) / p->R);
  p->lds_bytes = (uint32_t)(ANN_ASSIGN_STAGE_WORDS * 32 + ANN_ASSIGN_R_MAX * (32 + 4));
  p->work_bytes = cosine ? (uint64_t)(n + K) * 32 : 0;
  if (p->lds_bytes > ANN_ASSIGN_LDS_MAX) {
    *why = "ann assign: a workgroup needs more than 160 KiB of LDS";
    return ANN_ASSIGN_PLAN_REFUSED;
  }
  return ANN_ASSIGN_PLAN_OK;
}

}  // namespace vdb
