// The plan of a batched MSM: everything msm_batch_dev (msm.hip) decides before it touches a pointer — the window of a table, the range
// length, the capacities the kernels are given, the two-phase scatter's split of an entry's 31 bits, LDS sizes, the batch size under
// the memory budget and the layout of the work space — in a header of its own, with no HIP runtime call and no allocation, so that
// tools/msm_plan_probe.hip reaches the very functions the driver plans with and tests/test_msm_plan_cpu.py can hold them to a Python
// model (tests/msm_plan_model.py) and state what the kernels rely on: regions that are disjoint, aligned and inside the buffer,
// capacities below 2^31, LDS within a CU's.  What the kernels and the planner must agree on is defined here once.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace vdb {

#define MSM_SORT_THREADS 1024
// Range length (entries one thread of k_msm_accum adds up) is chosen per job: long ranges mean fewer segments, i.e.
// less work for k_msm_combine (256: 4 ms of combine on the k = 16 kmeans workload against 20 ms at 32, measured on the
// eight-word folding), short ranges keep small jobs parallel (a single 2^16 column has only ~130 k entries).
#define MSM_LCAP_MIN 32
#define MSM_LCAP_MAX 256

// A range is `lcap` consecutive entries of one column's bucket-sorted entry list.  Inside a range every change of
// bucket starts a new *segment*; each segment produces one partial sum.  Segment numbering follows the sorted order,
// so the partials of one bucket are contiguous: [seg_off[b], seg_off[b + 1]).
struct MsmRange {
  uint32_t col, bucket, start, len, seg0, pad;
};
struct MsmSegInfo {
  uint32_t idx, len;  // position of the segment among its bucket's segments, and how many the bucket has
};

// second phase of the two-phase scatter (k_msm_scatter2)
#define MSM_SCATTER2_THREADS 256
#define MSM_BIN_CAP (6 * 1024)   // entries of a bin a workgroup holds (24 registers per thread, 24 KB of LDS)

// a partial sum as k_msm_accum leaves it: raw limbs, 36 words (msm.hip, flush_l9)
#define MSM_RAW_WORDS 36

// The return codes of msm_window and msm_plan: VDB_OK and VDB_ERR_ARG of include/vdb.h (msm.hip asserts the equality).
constexpr int MSM_PLAN_OK = 0, MSM_PLAN_REFUSED = -3;

// what one CU has, and what the driver's launches may ask of it
constexpr size_t MSM_LDS_MAX = 160 * 1024;

// The process's settings (msm.hip reads them from the environment once).
struct MsmKnobs {
  uint32_t window = 0;   // VDB_MSM_C: the window of tables loaded without one of their own, 2..14 (any other value: 0, the measured choice)
};

// A table as vdb_srs_load_window builds it: W windows of c bits over table_n bases, B buckets per column.
struct MsmShape {
  uint32_t c, W, B;
  size_t table_n;
};

// The shape of the tables of 2^k bases.  `window_bits`: the caller's window, 0 for the default.
static inline int msm_window(uint32_t k, uint32_t window_bits, const MsmKnobs& kn, MsmShape* shape, const char** why) {
  // the counting sort keeps three counters per bucket in LDS: 2^(c-1) buckets must fit 160 KB (msm_plan holds every plan to it)
  if (!(window_bits == 0 || (window_bits >= 2 && window_bits <= 14))) {
    *why = "window_bits must be 0 (default) or 2..14";
    return MSM_PLAN_REFUSED;
  }
  uint32_t c = window_bits;
  if (!c) c = kn.window >= 2 && kn.window <= 14 ? kn.window : 0;
  // measured on the C4 witness columns (profiles/): per-task overhead of the many light buckets outweighs the
  // extra digits of a smaller window; c = 11 is the optimum for k = 16
  if (!c) c = k <= 8 ? 8 : 11;
  shape->c = c;
  shape->W = (254 + c - 1) / c;
  shape->B = 1u << (c - 1);
  shape->table_n = (size_t)1 << (k < 31 ? k : 31);
  // an entry of the sort is a table index in 31 bits and the sign
  if ((size_t)shape->W * shape->table_n > 0x7fffffffull) {
    *why = "srs: table index does not fit 31 bits";
    return MSM_PLAN_REFUSED;
  }
  return MSM_PLAN_OK;
}

struct MsmJob {
  size_t n_cols, n;   // n scalars per column, 1 .. table_n
};

// The card's memory as the driver sees it.
struct MsmMem {
  size_t free_bytes;   // hipMemGetInfo
  size_t held_bytes;   // what the work space's scratch slot holds already: free to this job too
  size_t cap_bytes;    // vdb_msm_set_scratch_cap; 0: none
};

// The regions of the work space, in the order they lie in it.
enum MsmRegion : uint32_t {
  MSM_ENTRIES,      // uint32_t: ent_cap per column, the sorted (table index | sign) entries
  MSM_RAW,          // uint4: one record of MSM_RAW_WORDS per segment, folded in place
  MSM_SUMS,         // uint4: one record per column, what k_msm_reduce leaves
  MSM_RANGES,       // MsmRange: range_cap_col per column
  MSM_SEGINFO,      // MsmSegInfo: one per segment
  MSM_SEG_OFF,      // uint32_t: B + 1 per column
  MSM_BUCKET_OFF,   // uint32_t: B + 1 per column
  MSM_COUNTERS,     // uint32_t: MSM_COUNTER_WORDS for the batch ([0]=segments, [1]=overflow, [2]=max segs/bucket, [3]=ranges)
  MSM_RECS,         // unsigned long long: n short-scalar records per column
  MSM_LONGQ,        // uint32_t: n queue entries per column
  MSM_N_REGIONS
};
constexpr size_t MSM_COUNTER_WORDS = 64;
// alignment of a region's elements; the work space itself starts on a multiple of all of them (hipMalloc: 256)
constexpr size_t MSM_REGION_ALIGN[MSM_N_REGIONS] = {4, 16, 16, 4, 4, 4, 4, 4, 8, 4};
// The work space is its per-column bytes times the batch size and MSM_SLACK: the counters and the padding in front of the aligned
// regions — below its alignment in front of each, and none in front of the first.
constexpr size_t MSM_SLACK = 512;
static_assert(MSM_COUNTER_WORDS * 4 + 15 + 15 + 7 + 6 * 3 <= MSM_SLACK, "the slack holds the counters and every region's padding");

struct MsmPlan {
  uint32_t lcap;              // range length, a power of two
  size_t ent_cap;             // entries of a column: every digit non-zero
  size_t range_cap_col, seg_cap_col;
  uint32_t seg_cap, range_cap;   // of a batch: below 2^31
  // two-phase scatter of the sort: bins of 2^fine_bits buckets; the table index and the fine bucket number share an entry's 31 bits.
  // fine_bits == 0: direct scatter, no k_msm_scatter2
  uint32_t idx_bits, fine_bits, bin_cap, scatter2_bins_x;
  uint32_t sort_lds, scatter2_lds;   // dynamic LDS of k_msm_sort and k_msm_scatter2, bytes
  uint32_t combine_passes;    // k_msm_combine launches per batch
  size_t nb, n_batches;       // columns per batch, batches
  size_t bytes;               // the work space
  size_t off[MSM_N_REGIONS];  // where each region starts in it
};

// MSM_PLAN_OK and the plan, or MSM_PLAN_REFUSED and the reason.  Allocates nothing.
static inline int msm_plan(const MsmShape& s, const MsmJob& j, const MsmMem& mem, MsmPlan* plan, const char** why) {
  const auto refuse = [why](const char* msg) {
    *why = msg;
    return MSM_PLAN_REFUSED;
  };
  const size_t n = j.n, n_cols = j.n_cols, B = s.B;
  // (the entry points refuse these before they plan)
  if (n_cols == 0 || n == 0 || n > s.table_n) return refuse("msm: the job does not fit the loaded table");
  MsmPlan& P = *plan;
  P.ent_cap = n * s.W;
  P.lcap = MSM_LCAP_MIN;
  while (P.lcap < MSM_LCAP_MAX && (n_cols * n) / P.lcap >= ((size_t)1 << 19)) P.lcap <<= 1;  // keep >= ~2^20 ranges in a large job
  P.range_cap_col = (P.ent_cap + P.lcap - 1) / P.lcap;  // worst case: every digit non-zero
  P.seg_cap_col = B + P.range_cap_col;
  // at most ceil(log2(max segments per bucket)) passes of k_msm_combine do work; the rest exit on the device-side maximum.  The range
  // length above follows from the whole job, so every batch runs the same passes
  P.combine_passes = 0;
  while (((size_t)1 << P.combine_passes) < P.range_cap_col + 1) P.combine_passes++;

  P.idx_bits = 1;
  while (P.idx_bits < 32 && ((uint64_t)1 << P.idx_bits) < (uint64_t)s.W * s.table_n) P.idx_bits++;
  P.fine_bits = 0;
  P.bin_cap = MSM_BIN_CAP;
  // (only where the direct scatter is what the sort waits for: thousands of buckets per column and dense scalars — the 14-bit windows
  //  of the product / quotient / fixed columns; with the 11-bit windows of the witness columns, 1,024 buckets and mostly short scalars,
  //  the second phase costs more than it saves: 15.4 + 4.2 against 15.2 ms per C4 step)
  if (s.c >= 13) {
    P.fine_bits = s.c - 1 - 8;              // 256 bins
    if (P.fine_bits + P.idx_bits > 31) P.fine_bits = P.idx_bits < 31 ? 31 - P.idx_bits : 0;
    if (P.fine_bits < 2) P.fine_bits = 0;
  }
  if (P.fine_bits + P.idx_bits > 31) return refuse("msm: table index and fine bucket number do not fit an entry's 31 bits");
  P.scatter2_bins_x = P.fine_bits ? ((B >> P.fine_bits) < 64 ? (uint32_t)(B >> P.fine_bits) : 64u) : 0;   // (16 .. 256 workgroups per column measure the same)
  const size_t sort_lds = (3 * B + 32) * sizeof(uint32_t);   // hist, cursor, ucnt of B words each and the scan's wave sums
  const size_t scatter2_lds = P.fine_bits ? ((size_t)P.bin_cap + ((size_t)1 << P.fine_bits)) * sizeof(uint32_t) : 0;
  if (sort_lds > MSM_LDS_MAX || scatter2_lds > MSM_LDS_MAX) return refuse("msm: a kernel needs more than 160 KiB of LDS");
  P.sort_lds = (uint32_t)sort_lds;
  P.scatter2_lds = (uint32_t)scatter2_lds;

  // a column's share of every region; the counters are the batch's
  size_t col_bytes[MSM_N_REGIONS];
  col_bytes[MSM_ENTRIES] = P.ent_cap * sizeof(uint32_t);
  col_bytes[MSM_RAW] = P.seg_cap_col * MSM_RAW_WORDS * 4;
  col_bytes[MSM_SUMS] = MSM_RAW_WORDS * 4;
  col_bytes[MSM_RANGES] = P.range_cap_col * sizeof(MsmRange);
  col_bytes[MSM_SEGINFO] = P.seg_cap_col * sizeof(MsmSegInfo);
  col_bytes[MSM_SEG_OFF] = col_bytes[MSM_BUCKET_OFF] = (B + 1) * sizeof(uint32_t);
  col_bytes[MSM_COUNTERS] = 0;
  col_bytes[MSM_RECS] = n * sizeof(unsigned long long);
  col_bytes[MSM_LONGQ] = n * sizeof(uint32_t);
  size_t per_col = 0;
  for (size_t b : col_bytes) per_col += b;

  // budget: half of what is free on the card (counting the slot this buffer already holds), between 8 and 96 GiB —
  // on a 288 GB MI355X the 8,146 columns of the kmeans k = 16 job go through in ONE batch (68 GB), so the whole
  // bucket-folding tail can run beside the NTTs (defer_tail).  Large batches keep thousands of independent column reductions in flight
  size_t budget = (mem.free_bytes + mem.held_bytes) / 2;
  if (budget < ((size_t)8 << 30)) budget = (size_t)8 << 30;
  if (budget > ((size_t)96 << 30)) budget = (size_t)96 << 30;
  // a caller that is about to allocate tens of GB of its own (keygen) bounds the work space: growing it to half of a still empty
  // card and releasing it again costs seconds of page mapping (vdb_msm_set_scratch_cap)
  if (mem.cap_bytes && budget > mem.cap_bytes) budget = mem.cap_bytes > mem.held_bytes ? mem.cap_bytes : mem.held_bytes;
  size_t nb = budget / per_col;
  if (nb < 1) nb = 1;
  if (nb > n_cols) nb = n_cols;
  if (nb > 16384) nb = 16384;
  // segment and range numbers are 32-bit in the kernels and their atomics; range_cap_col < seg_cap_col bounds the ranges too.
  // (seg_cap_col <= 2^13 + 2^31 / 32: at least one column always fits)
  if (nb * P.seg_cap_col > 0x7fffffffull) nb = 0x7fffffffull / P.seg_cap_col;
  P.nb = nb;
  P.n_batches = (n_cols + nb - 1) / nb;
  P.seg_cap = (uint32_t)(nb * P.seg_cap_col);
  P.range_cap = (uint32_t)(nb * P.range_cap_col);
  P.bytes = nb * per_col + MSM_SLACK;
  size_t at = 0;
  for (uint32_t r = 0; r < MSM_N_REGIONS; r++) {
    at = (at + MSM_REGION_ALIGN[r] - 1) / MSM_REGION_ALIGN[r] * MSM_REGION_ALIGN[r];
    P.off[r] = at;
    at += nb * col_bytes[r] + (r == MSM_COUNTERS ? MSM_COUNTER_WORDS * sizeof(uint32_t) : 0);
  }
  // (at <= bytes: the static_assert beside MSM_SLACK)
  return MSM_PLAN_OK;
}

}  // namespace vdb
