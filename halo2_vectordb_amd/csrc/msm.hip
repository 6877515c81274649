// Batched multi-scalar multiplication over BN254 G1 for gfx950.
//
// Replaces halo2 `arithmetic::best_multiexp` / `ParamsKZG::commit_lagrange` (third-party halo2-axiom,
// reached from /root/reference/src/scaffold/mod.rs:296 and :273): one exact
// group element per column, returned as canonical affine (identity = (0,0)).
//
// MI355X-first design (not the CPU's per-thread chunked Pippenger):
//  * The bases are fixed per circuit size, so vdb_srs_load precomputes T[j][i] = 2^(c*j) * G_i for every
//    c-bit window j (tens of MB in 288 GB of HBM, L2 / Infinity-Cache resident).  All windows of a column
//    then share ONE bucket set: a signed digit d of window j of scalar i adds +-T[j][i] to bucket |d|.
//    No per-window doubling chain, one bucket reduction per column.
//  * Scalars are sign-folded (s > r/2 -> r - s with the point negated) so the many "negative" witness
//    values become short; zero digits cost nothing.
//  * k_msm_sort: one workgroup per column does a counting sort of the (digit -> table index) pairs
//    entirely in LDS (histogram, scan, scatter) and cuts the sorted list into ranges of LCAP entries; bucket
//    changes inside a range open new segments (one partial sum each), which removes the skew of witness columns.
//    A scalar whose magnitude is a 32-bit value times 2^(c j0) — bits, limbs, and the fixed-point values of the circuits, small integers
//    times 2^48, 2^96, ... — is decomposed once and revisited through an 8-byte record (msm_digits.hpp); only the rest are reduced again.
//    Two workgroups share a CU (eight waves per SIMD).
//    With wide windows (thousands of buckets, dense scalars) the scatter goes in two phases: entries to the 256 runs of coarse bins
//    here, k_msm_scatter2 orders each bin in place through LDS — four-byte stores to 8,192 open runs per column do not merge in L2.
//  * k_msm_accum: one thread per range (every lane does exactly LCAP mixed additions), XYZZ accumulator in VGPRs.
//  * k_msm_combine: segmented tree reduction of the partials of every bucket, in the accumulator's nine-limb form.
//  * k_msm_reduce: one wavefront per column; each lane folds its slice of buckets with the running-sum
//    trick, lanes are combined with wavefront shuffles (nine-limb form throughout: ec_l9.hpp).
//  * k_msm_normalise: one lane per column brings the column's sum to canonical affine (the inversion).
//  * The driver, msm_batch_dev, decides nothing between its launches: the window of a table, the range length, the capacities, the
//    scatter's bit split, LDS sizes, the batch size under the memory budget and the layout of the work space are msm_plan.hpp's
//    (host-only; tools/msm_plan_probe.hip and tests/test_msm_plan_cpu.py hold it to a model on the CPU).  The entry points fill an
//    MsmCall by name and share one argument check, one deferred prologue and one copy-out.
// Roofline: algorithmic HBM traffic is 32 B per scalar (+ bases once); the kernels are bound by 32-bit
// integer multiply-add throughput (v_mad_u64_u32), see DESIGN.md.
#include "common.hpp"
#include "ec.hpp"
#include "ec_l9.hpp"
#include "limb9.hpp"
#include "msm_digits.hpp"
#include "msm_plan.hpp"

struct vdb_srs {
  uint32_t k;
  size_t n;
  uint32_t c, W, B;
  vdb::Affine* table[2];  // [0] monomial, [1] lagrange; each W * n points
  int device;             // the GPU whose HBM holds the tables
};
// a handle only works on the device it was loaded on (the calling thread's current one: vdb_set_device)
#define VDB_SRS_HERE(srs) VDB_ARG((srs)->device == vdb::ctx().device, "this srs handle was loaded on another device (vdb_set_device)")

namespace vdb {

// MSM_SORT_THREADS, the range length bounds, MsmRange and MsmSegInfo: msm_plan.hpp

// ---------------------------------------------------------------- table precompute
__global__ __launch_bounds__(256) void k_srs_table(const Affine* __restrict__ bases, Affine* __restrict__ table, size_t n, uint32_t c, uint32_t W) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine p = ld_affine(bases + i);
  // table entries are stored times 32, i.e. in Montgomery form with R' = 2^261: the form k_msm_accum computes in
  // (the identity (0, 0) is unaffected)
  const u256 m32 = to_mont<Fq>(u256_from_u64(32));
  for (uint32_t j = 0; j < W; j++) {
    Affine ps;
    ps.x = fq_mul(p.x, m32);
    ps.y = fq_mul(p.y, m32);
    st_affine(table + (size_t)j * n + i, ps);
    if (j + 1 < W) {
      XYZZ q = xyzz_double_affine(p);
      for (uint32_t d = 1; d < c; d++) q = xyzz_double(q);
      p = xyzz_to_affine(q);
    }
  }
}

// ---------------------------------------------------------------- digit decomposition
// fold_scalar, emit_digits, emit_digits32 and the short-scalar record: msm_digits.hpp
template <class F>
__device__ __forceinline__ void for_each_digit(const u256& mont_scalar, uint32_t c, uint32_t W, F&& f) {
  if (u256_is_zero(mont_scalar)) return;  // Montgomery form of zero is zero: skip the product for the ~1/3 zero cells
  u256 s = from_mont<Fr>(mont_scalar);
  bool neg = fold_scalar(s);
  emit_digits(s, neg, u256_bits(s), c, W, [&](uint32_t j, uint32_t d, bool ng, size_t) { f(j, d, ng); });
}
// Two-speed, two-pass walk over a column's scalars (the counting sort visits them twice: histogram, then scatter).
// Every lane of a wavefront pays for the longest path among its 64 scalars, and witness columns mix bits and 15-bit limbs with
// fixed-point values: small integers times 2^48, 2^96, ..., long by bit length but two or three windows wide.  First visit
// (`first`): the Montgomery reduction, the sign fold, the bit length and the first window j0 that holds a bit are computed once.
// A scalar whose magnitude is s' * 2^(c * j0) with s' below 2^32 and at most three windows wide is short: it leaves an 8-byte record
// {s', sign, j0, length of s'} (msm_digits.hpp) and is processed from registers.  Any other is long: it is appended to a queue
// (wavefront-aggregated), and all long ones are then processed densely, every lane holding one, with the full 256-bit walk.
// Second visit: the short scalars come straight from their records (no 32-byte load, no field arithmetic), the long ones from the
// queue.  `queue`, `rec`: n entries of this column each.
// The digits of a short scalar are those of the full walk over s: the windows below j0 are all zero and send no carry up; from
// window j0 on the signed recoding reads s' alone; and the full walk stops at min(nb / c + 2, W), which is
// j0 + min(nb' / c + 2, W - j0) because nb = nb' + c * j0.  So emit_digits32(s', ..., W - j0) with its window j handed on as j + j0
// meets the same (window, digit, sign) triples (tests/test_msm_digits_cpu.py holds both walks to big integers).
// `sc` (a materialised column) or `cs` (a column still lying in the witness stream, see ColSrc) supplies the scalars.
template <class F>
__device__ __forceinline__ void walk_scalars(const u256* __restrict__ sc, const ColSrc* __restrict__ cs, uint32_t n_blind, const uint8_t* __restrict__ mk,
                                             size_t n, uint32_t c, uint32_t W, uint32_t* __restrict__ queue, unsigned long long* __restrict__ rec,
                                             uint32_t* s_qcnt, bool first, F&& f, bool dense = false) {
  ColSrc src;
  if (cs) src = *cs;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  if (dense) {
    // columns of full-width scalars (products, quotient pieces, fixed columns: the wide-window tables): no short / long sorting, every
    // scalar is reduced and decomposed where it is met — one Montgomery reduction per visit instead of two on the first
    for (size_t i0 = 0; i0 < n; i0 += MSM_SORT_THREADS) {
      const size_t i = i0 + tid;
      if (i >= n || (mk && mk[i])) continue;
      u256 s = cs ? colsrc_fetch(src, i, n, n_blind) : ld256(sc + i);
      if (u256_is_zero(s)) continue;
      s = from_mont<Fr>(s);
      const bool neg = fold_scalar(s);
      emit_digits(s, neg, u256_bits(s), c, W, f, i);
    }
    return;
  }
  const uint32_t short_bits = msm_short_bits(c), inv_c = msm_recip16(c);
  if (first) {
    if (tid == 0) *s_qcnt = 0;
    __syncthreads();
    for (size_t i0 = 0; i0 < n; i0 += MSM_SORT_THREADS) {
      const size_t i = i0 + tid;
      bool live = i < n && !(mk && mk[i]);  // masked: constant cell, its term is part of the precomputed per-column point
      u256 s;
      bool neg = false;
      uint32_t nb = 0;
      if (live) {
        s = cs ? colsrc_fetch(src, i, n, n_blind) : ld256(sc + i);
        live = !u256_is_zero(s);  // Montgomery form of zero is zero: no reduction for the ~1/3 zero cells
      }
      if (live) {
        s = from_mont<Fr>(s);
        neg = fold_scalar(s);
        nb = u256_bits(s);
      }
      uint32_t mag = 0, nbs = 0, j0 = 0;
      const bool is_long = live && !msm_classify(s, nb, c, inv_c, short_bits, mag, nbs, j0);
      const unsigned long long m = __ballot(is_long);
      if (m) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(s_qcnt, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, 0, 64);
        if (is_long) queue[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)i;
      }
      const bool is_short = live && !is_long;
      if (i < n) rec[i] = is_short ? msm_rec_encode(mag, neg, nbs, j0) : 0ull;
      if (is_short) emit_digits_short(mag, neg, nbs, j0, c, W, f, i);
    }
  } else {
    for (size_t i0 = 0; i0 < n; i0 += MSM_SORT_THREADS) {
      const size_t i = i0 + tid;
      const unsigned long long r = i < n ? rec[i] : 0ull;
      if (r & MSM_REC_VALID) {
        const MsmRec sr = msm_rec_decode(r);
        emit_digits_short(sr.mag, sr.neg, sr.nbs, sr.j0, c, W, f, i);
      }
    }
  }
  __syncthreads();  // queue complete (written and read by this workgroup only)
  const uint32_t nq = *s_qcnt;
  for (uint32_t qi = tid; qi < nq; qi += MSM_SORT_THREADS) {
    const size_t i = queue[qi];
    u256 s = from_mont<Fr>(cs ? colsrc_fetch(src, i, n, n_blind) : ld256(sc + i));
    const bool neg = fold_scalar(s);
    emit_digits(s, neg, u256_bits(s), c, W, f, i);
  }
}

// block-wide exclusive scan of one value per thread (blockDim.x = MSM_SORT_THREADS); returns the
// exclusive prefix, *total gets the block sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wave_sums, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t t = __shfl_up(inc, o, 64);
    if ((int)lane >= o) inc += t;
  }
  if (lane == 63) wave_sums[wave] = inc;
  __syncthreads();
  if (wave == 0) {
    uint32_t ws = lane < (MSM_SORT_THREADS / 64) ? wave_sums[lane] : 0;
    uint32_t winc = ws;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      uint32_t t = __shfl_up(winc, o, 64);
      if ((int)lane >= o) winc += t;
    }
    if (lane < (MSM_SORT_THREADS / 64)) wave_sums[lane] = winc - ws;  // exclusive wave offsets
    if (lane == (MSM_SORT_THREADS / 64) - 1) wave_sums[MSM_SORT_THREADS / 64] = winc;
  }
  __syncthreads();
  uint32_t res = wave_sums[wave] + inc - v;
  *total = wave_sums[MSM_SORT_THREADS / 64];
  __syncthreads();
  return res;
}

// per column: the number of (scalar, window) entries its MSM sorts and accumulates — the non-zero signed digits of the
// cells that are not masked out
__global__ __launch_bounds__(256) void k_msm_count_entries(const u256* __restrict__ scalars, const uint8_t* __restrict__ mask, uint64_t rows, uint32_t c,
                                                           uint32_t W, unsigned long long* __restrict__ counts) {
  const uint64_t col = blockIdx.x;
  uint32_t n = 0;
  for (uint64_t r = threadIdx.x; r < rows; r += 256) {
    const uint64_t i = col * rows + r;
    if (mask && mask[i]) continue;
    for_each_digit(ld256(scalars + i), c, W, [&](uint32_t, uint32_t, bool) { n++; });
  }
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_down(n, o, 64);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&counts[col], (unsigned long long)n);
}

// One workgroup per column: counting sort of (bucket -> table index|sign), segment numbering and range cutting.
// Eight waves per SIMD (the second launch bound): the kernel waits — on its loads, its LDS atomics and its barriers — far more
// than it issues, and a 1,024-thread workgroup is four waves on every SIMD, so a CU takes a second workgroup only when all eight wave
// slots are usable.  Left alone the compiler took 106 scalar registers, which allows seven; held to eight it keeps 78 and parks 24 in
// vector lanes, no scratch.  With the 11-bit windows' 12 KB of LDS two columns then share a CU and fill each other's waits
// (15.3 -> 12.8 ms per k = 16 step, profiles/NOTES.md); the wide windows' histograms leave room for one workgroup as before.
__global__ __launch_bounds__(MSM_SORT_THREADS, 8) void k_msm_sort(const u256* __restrict__ scalars, const ColSrc* __restrict__ srcs, uint32_t n_blind, size_t n,
                                                               size_t table_n, uint32_t c, uint32_t W,
                                                               uint32_t* __restrict__ entries, size_t ent_cap,
                                                               uint32_t* __restrict__ seg_off, uint32_t* __restrict__ bucket_off, MsmRange* __restrict__ ranges,
                                                               uint32_t* __restrict__ counters /* [0]=segments, [1]=overflow, [2]=max segs/bucket, [3]=ranges */,
                                                               uint32_t seg_cap, uint32_t range_cap,
                                                               const uint8_t* __restrict__ skip_mask /* optional: n per column */,
                                                               uint32_t lcap /* range length, a power of two */,
                                                               uint32_t* __restrict__ longq /* n per column: queue of the long scalars */,
                                                               unsigned long long* __restrict__ recs /* n per column: short-scalar records */,
                                                               uint32_t fine_bits, uint32_t idx_bits, uint32_t bin_cap) {
  extern __shared__ uint32_t sh[];
  const uint32_t B = 1u << (c - 1);
  uint32_t* hist = sh;            // B
  uint32_t* cursor = sh + B;      // B
  uint32_t* ucnt = sh + 2 * B;    // B
  uint32_t* wave_sums = sh + 3 * B;  // 18
  __shared__ uint32_t s_base, s_rbase, s_qcnt;
  const uint32_t col = blockIdx.x, tid = threadIdx.x;
  const u256* sc = scalars ? scalars + (size_t)col * n : nullptr;
  const ColSrc* cs = srcs ? srcs + col : nullptr;
  const uint8_t* mk = skip_mask ? skip_mask + (size_t)col * n : nullptr;
  for (uint32_t b = tid; b < B; b += MSM_SORT_THREADS) hist[b] = 0;
  __syncthreads();
  uint32_t* queue = longq + (size_t)col * n;
  unsigned long long* rec = recs + (size_t)col * n;
  walk_scalars(sc, cs, n_blind, mk, n, c, W, queue, rec, &s_qcnt, true, [&](uint32_t, uint32_t d, bool, size_t) { atomicAdd(&hist[d - 1], 1u); }, fine_bits != 0);
  __syncthreads();
  // scan: thread owns buckets [tid*ipt, (tid+1)*ipt)
  const uint32_t ipt = (B + MSM_SORT_THREADS - 1) / MSM_SORT_THREADS;
  uint32_t cnt_local = 0;
  for (uint32_t q = 0; q < ipt; q++) {
    uint32_t b = tid * ipt + q;
    if (b < B) cnt_local += hist[b];
  }
  uint32_t total_cnt, total_ua;
  const uint32_t cnt_pre0 = block_exclusive_scan(cnt_local, wave_sums, &total_cnt);
  // buckets whose first entry is not LCAP-aligned open one extra segment
  uint32_t ua_local = 0;
  {
    uint32_t off = cnt_pre0;
    for (uint32_t q = 0; q < ipt; q++) {
      uint32_t b = tid * ipt + q;
      if (b < B) {
        if (hist[b] && (off % lcap)) ua_local++;
        off += hist[b];
      }
    }
  }
  const uint32_t ua_pre0 = block_exclusive_scan(ua_local, wave_sums, &total_ua);
  const uint32_t nranges = (total_cnt + lcap - 1) / lcap, nseg = nranges + total_ua;
  if (tid == 0) {
    uint32_t base = atomicAdd(&counters[0], nseg);
    uint32_t rb = atomicAdd(&counters[3], nranges);
    if (base + nseg > seg_cap || rb + nranges > range_cap || total_cnt > ent_cap) {
      atomicExch(&counters[1], 1u);
      base = 0xffffffffu;
    }
    s_base = base;
    s_rbase = rb;
  }
  __syncthreads();
  const uint32_t base = s_base, rbase = s_rbase;
  uint32_t* soff = seg_off + (size_t)col * (B + 1);
  uint32_t* boff = bucket_off + (size_t)col * (B + 1);
  if (base == 0xffffffffu) {  // overflow: publish an empty column so later kernels stay in bounds
    for (uint32_t b = tid; b <= B; b += MSM_SORT_THREADS) {
      soff[b] = 0;
      boff[b] = 0;
    }
    return;
  }
  {
    uint32_t off = cnt_pre0, ua = ua_pre0;
    for (uint32_t q = 0; q < ipt; q++) {
      uint32_t b = tid * ipt + q;
      if (b < B) {
        uint32_t cnt = hist[b];
        cursor[b] = off;
        ucnt[b] = ua;
        boff[b] = off;
        soff[b] = base + (off + lcap - 1) / lcap + ua;
        if (cnt) {
          uint32_t segs = (off + cnt + lcap - 1) / lcap - off / lcap;
          if (segs > 1) atomicMax(&counters[2], segs);  // lets k_msm_combine skip passes nobody needs
          if (off % lcap) ua++;
        }
        off += cnt;
      }
    }
  }
  if (tid == 0) {
    soff[B] = base + nseg;
    boff[B] = total_cnt;
  }
  __syncthreads();
  // range descriptors: starting bucket by binary search over the (monotone) bucket offsets in LDS
  for (uint32_t r = tid; r < nranges; r += MSM_SORT_THREADS) {
    const uint32_t x = r * lcap;
    uint32_t lo_b = 0, hi_b = B;  // last b with cursor[b] <= x
    while (hi_b - lo_b > 1) {
      uint32_t mid = (lo_b + hi_b) >> 1;
      if (cursor[mid] <= x) lo_b = mid;
      else hi_b = mid;
    }
    const uint32_t bo = cursor[lo_b];
    MsmRange rg;
    rg.col = col;
    rg.bucket = lo_b;
    rg.start = x;
    rg.len = total_cnt - x < lcap ? total_cnt - x : lcap;
    rg.seg0 = base + r + ucnt[lo_b] + ((bo % lcap) && bo < x ? 1u : 0u);
    rg.pad = 0;
    ranges[rbase + r] = rg;
  }
  __syncthreads();
  uint32_t* ent = entries + (size_t)col * ent_cap;
  // Two-phase scatter (fine_bits > 0): 1.2 M four-byte stores to 8,192 open bucket runs per column never merge in L2 (a workgroup per CU,
  // every one with thousands of partly written lines) and cost two thirds of this kernel.  Here the entries go to the few hundred runs of
  // the coarse bins — bucket >> fine_bits, contiguous because a bin is a range of buckets — carrying their fine bucket number above the
  // table index; k_msm_scatter2 then orders every bin in place through LDS.
  if (fine_bits) {
    const uint32_t n_bins = B >> fine_bits;
    for (uint32_t q = tid; q < n_bins; q += MSM_SORT_THREADS) {
      const uint32_t lo = cursor[q << fine_bits], hi = q + 1 < n_bins ? cursor[(q + 1) << fine_bits] : total_cnt;
      ucnt[q] = lo;                          // the bins' cursors (ucnt is free: the range descriptors are written)
      hist[q] = hi - lo > bin_cap ? 1u : 0u; // a bin too large for a workgroup of the second phase (the top window's few small digits;
                                             // one value repeated down a witness column) is scattered directly: its runs are few
    }
    __syncthreads();
    const uint32_t fmask = (1u << fine_bits) - 1u;
    walk_scalars(sc, cs, n_blind, mk, n, c, W, queue, rec, &s_qcnt, false, [&](uint32_t j, uint32_t d, bool neg, size_t i) {
      const uint32_t b = d - 1, bin = b >> fine_bits;
      const uint32_t payload = (uint32_t)(j * table_n + i) | (neg ? 0x80000000u : 0u);
      if (hist[bin]) {
        ent[atomicAdd(&cursor[b], 1u)] = payload;
      } else {
        ent[atomicAdd(&ucnt[bin], 1u)] = payload | ((b & fmask) << idx_bits);
      }
    }, true);
    return;
  }
  walk_scalars(sc, cs, n_blind, mk, n, c, W, queue, rec, &s_qcnt, false, [&](uint32_t j, uint32_t d, bool neg, size_t i) {
    uint32_t pos = atomicAdd(&cursor[d - 1], 1u);
    ent[pos] = (uint32_t)(j * table_n + i) | (neg ? 0x80000000u : 0u);
  });
}

// second phase of the two-phase scatter: one workgroup per (bin, column) loads the bin's entries (coarse order) into LDS and writes
// them back bucket by bucket — 2^fine_bits open runs per workgroup, which L2 merges into whole lines
// (MSM_SCATTER2_THREADS threads; MSM_BIN_CAP, the entries of a bin a workgroup holds: msm_plan.hpp)
__global__ __launch_bounds__(MSM_SCATTER2_THREADS) void k_msm_scatter2(uint32_t* __restrict__ entries, size_t ent_cap, const uint32_t* __restrict__ bucket_off,
                                                                       uint32_t B, uint32_t fine_bits, uint32_t idx_bits, uint32_t bin_cap,
                                                                       const uint32_t* __restrict__ counters) {
  extern __shared__ uint32_t sh2[];
  if (counters[1]) return;
  const uint32_t col = blockIdx.y, tid = threadIdx.x;
  const uint32_t* bo = bucket_off + (size_t)col * (B + 1);
  const uint32_t nf = 1u << fine_bits, n_bins = B >> fine_bits;
  uint32_t* outb = sh2;           // bin_cap: the bin in bucket order, written back in whole lines
  uint32_t* fcur = sh2 + bin_cap; // nf
  uint32_t* ent = entries + (size_t)col * ent_cap;
  const uint32_t fmask = nf - 1u, imask = (1u << idx_bits) - 1u;
  const uint32_t lane = tid & 63u;
  for (uint32_t bin = blockIdx.x; bin < n_bins; bin += gridDim.x) {   // (uniform per workgroup: the barriers below are reached by all)
    const uint32_t b0 = bin << fine_bits;
    const uint32_t lo = bo[b0], hi = bo[b0 + nf];
    const uint32_t S = hi - lo;
    if (S == 0 || S > bin_cap) continue;   // (a larger bin was scattered to its buckets directly)
    // the bin as it lies (coarse order), in registers: every load of the thread in flight at once (a loop of unknown length would
    // wait for each one: ~20 round trips to HBM per bin)
    uint32_t r[MSM_BIN_CAP / MSM_SCATTER2_THREADS];
#pragma unroll
    for (uint32_t q = 0; q < MSM_BIN_CAP / MSM_SCATTER2_THREADS; q++) {
      const uint32_t i = tid + q * MSM_SCATTER2_THREADS;
      r[q] = i < S ? ent[lo + i] : 0u;
    }
    for (uint32_t f = tid; f < nf; f += MSM_SCATTER2_THREADS) fcur[f] = bo[b0 + f] - lo;
    __syncthreads();
    // positions by wavefront-level ranking: the lanes that hold the same bucket are found with one ballot per bucket bit, their
    // leader draws the run of positions with one atomic, the others take theirs by rank
#pragma unroll
    for (uint32_t q = 0; q < MSM_BIN_CAP / MSM_SCATTER2_THREADS; q++) {
      const uint32_t i = tid + q * MSM_SCATTER2_THREADS;
      if (q * MSM_SCATTER2_THREADS >= S) break;        // uniform
      const bool active = i < S;
      const uint32_t e = r[q];
      const uint32_t f = (e >> idx_bits) & fmask;
      unsigned long long peers = __ballot(active);
      for (uint32_t bit = 0; bit < fine_bits; bit++) {
        const unsigned long long m = __ballot(active && ((f >> bit) & 1u));
        peers &= ((f >> bit) & 1u) ? m : ~m;
      }
      uint32_t base = 0;
      const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
      if (active && rank == 0) base = atomicAdd(&fcur[f], (uint32_t)__popcll(peers));
      base = (uint32_t)__shfl((int)base, active ? (int)__ffsll((long long)peers) - 1 : (int)lane, 64);
      if (active) outb[base + rank] = (e & 0x80000000u) | (e & imask);
    }
    __syncthreads();
    for (uint32_t i = tid; i < S; i += MSM_SCATTER2_THREADS) ent[lo + i] = outb[i];
    __syncthreads();
  }
}

// A segment's partial sum leaves k_msm_accum as raw limbs (36 words; zz = 0 encodes the identity): inside the accumulation
// loop a flush by ANY lane of a wavefront makes the whole wavefront walk the flush code, so it has to be cheap.  The bucket
// folding works on these records as they are (xyzz_add_l9 takes and leaves the accumulator's form): k_msm_combine folds them
// in place, k_msm_reduce reads them and leaves one such record per column, and only k_msm_normalise converts — one column's
// sum, not every segment (a conversion kernel used to bring all segments to eight-word XYZZ: four products and a canonical
// form each, which the folding then split into limbs again).  MSM_RAW_WORDS: msm_plan.hpp
__device__ __forceinline__ void flush_l9(uint4* dst, const AccL9& acc, bool ident) {
  const uint32_t z = ident ? 0u : 0xffffffffu;
  dst[0] = make_uint4(acc.x.l[0], acc.x.l[1], acc.x.l[2], acc.x.l[3]);
  dst[1] = make_uint4(acc.x.l[4], acc.x.l[5], acc.x.l[6], acc.x.l[7]);
  dst[2] = make_uint4(acc.y.l[0], acc.y.l[1], acc.y.l[2], acc.y.l[3]);
  dst[3] = make_uint4(acc.y.l[4], acc.y.l[5], acc.y.l[6], acc.y.l[7]);
  dst[4] = make_uint4(acc.zz.l[0] & z, acc.zz.l[1] & z, acc.zz.l[2] & z, acc.zz.l[3] & z);
  dst[5] = make_uint4(acc.zz.l[4] & z, acc.zz.l[5] & z, acc.zz.l[6] & z, acc.zz.l[7] & z);
  dst[6] = make_uint4(acc.zzz.l[0], acc.zzz.l[1], acc.zzz.l[2], acc.zzz.l[3]);
  dst[7] = make_uint4(acc.zzz.l[4], acc.zzz.l[5], acc.zzz.l[6], acc.zzz.l[7]);
  dst[8] = make_uint4(acc.x.l[8], acc.y.l[8], acc.zz.l[8] & z, acc.zzz.l[8]);
}
__device__ __forceinline__ void raw_l9_low8(L9& c, const uint4& a, const uint4& b) {
  c.l[0] = a.x; c.l[1] = a.y; c.l[2] = a.z; c.l[3] = a.w;
  c.l[4] = b.x; c.l[5] = b.y; c.l[6] = b.z; c.l[7] = b.w;
}
// the record back into registers (the identity carries no meaningful limbs besides its zero zz: a lazy zz of a point is never zero)
__device__ __forceinline__ void ld_raw_l9(const uint4* src, AccL9& acc, bool& ident) {
  uint4 w[9];
#pragma unroll
  for (int i = 0; i < 9; i++) w[i] = src[i];
  raw_l9_low8(acc.x, w[0], w[1]);
  raw_l9_low8(acc.y, w[2], w[3]);
  raw_l9_low8(acc.zz, w[4], w[5]);
  raw_l9_low8(acc.zzz, w[6], w[7]);
  acc.x.l[8] = w[8].x; acc.y.l[8] = w[8].y; acc.zz.l[8] = w[8].z; acc.zzz.l[8] = w[8].w;
  uint32_t zz_any = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) zz_any |= acc.zz.l[k];
  ident = zz_any == 0;
}

// One thread per range: exactly `lcap` mixed additions per lane (full lane utilisation); the accumulator is
// flushed to the next segment slot whenever the sorted entry list moves on to another bucket.
__global__ __launch_bounds__(256) void k_msm_accum(const Affine* __restrict__ table, const uint32_t* __restrict__ entries, size_t ent_cap,
                                                   const MsmRange* __restrict__ ranges, const uint32_t* __restrict__ bucket_off, uint32_t B,
                                                   const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ counters, uint4* __restrict__ raw,
                                                   MsmSegInfo* __restrict__ seginfo, uint32_t range_cap, MsmL9Consts K) {
  if (counters[1]) return;  // sort overflowed (never expected: capacities are worst-case)
  const uint32_t total = counters[3] < range_cap ? counters[3] : range_cap;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    MsmRange rg = ranges[t];
    const uint32_t* e = entries + (size_t)rg.col * ent_cap;
    const uint32_t* bo = bucket_off + (size_t)rg.col * (B + 1);
    const uint32_t* so = seg_off + (size_t)rg.col * (B + 1);
    uint32_t b = rg.bucket, seg = rg.seg0, next = bo[b + 1];
    AccL9 acc;
    bool ident = true;
    // software prefetch: the gather of the next table point is in flight during the current addition
    uint32_t v = e[rg.start];
    Affine nxt = ld_affine(table + (v & 0x7fffffffu));
    for (uint32_t q = 0; q < rg.len; q++) {
      const uint32_t pos = rg.start + q;
      if (pos == next) {  // bucket boundary: close the segment
        flush_l9(raw + (size_t)seg * (MSM_RAW_WORDS / 4), acc, ident);
        {
          const uint32_t s0 = so[b];
          seginfo[seg].idx = seg - s0;
          seginfo[seg].len = so[b + 1] - s0;
        }
        seg++;
        ident = true;
        do {
          b++;
          next = bo[b + 1];
        } while (next == pos);  // skip empty buckets
      }
      Affine p = nxt;
      bool neg = (v >> 31) != 0;
      if (q + 1 < rg.len) {
        v = e[pos + 1];
        nxt = ld_affine(table + (v & 0x7fffffffu));
      }
      if (!affine_is_identity(p)) madd_l9(acc, ident, p, neg, K);
    }
    flush_l9(raw + (size_t)seg * (MSM_RAW_WORDS / 4), acc, ident);
    {
      const uint32_t s0 = so[b];
      seginfo[seg].idx = seg - s0;
      seginfo[seg].len = so[b + 1] - s0;
    }
  }
}

// Segmented tree reduction of the partial sums of every bucket: in pass p a bucket that still holds
// len_p = ceil(len / 2^p) > 1 partials folds its upper half onto its lower half.  A thread needs only its own
// (idx, len) record — no lookups — so a pass in which a segment has nothing to do costs one coalesced 8-byte read, and
// the lanes that do work are contiguous.  After ceil(log2(max segments per bucket)) passes the sum of bucket b sits in
// its first segment slot.  This is what removes the witness-column skew from the reduce kernel.
// (Measured alternatives: radix-8 in-place folding — 2x slower, one active lane in eight; one thread per bucket — 8x
// slower, serial tails of the heavy buckets.)
__global__ __launch_bounds__(256) void k_msm_combine(uint4* __restrict__ raw, const MsmSegInfo* __restrict__ seginfo, const uint32_t* __restrict__ counters,
                                                     uint32_t pass, uint32_t task_cap, MsmL9Consts K) {
  if (counters[1]) return;
  if ((1u << pass) >= counters[2]) return;  // every bucket is already folded to one partial
  const uint32_t total = counters[0] < task_cap ? counters[0] : task_cap;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const MsmSegInfo si = seginfo[t];
    const uint32_t len = (si.len + (1u << pass) - 1) >> pass, half = (len + 1) >> 1;
    if (len <= 1 || si.idx + half >= len) continue;
    AccL9 a, b;
    bool a_id, b_id;
    ld_raw_l9(raw + (size_t)t * (MSM_RAW_WORDS / 4), a, a_id);
    ld_raw_l9(raw + (size_t)(t + half) * (MSM_RAW_WORDS / 4), b, b_id);
    xyzz_add_l9(a, a_id, b, b_id, K);
    flush_l9(raw + (size_t)t * (MSM_RAW_WORDS / 4), a, a_id);
  }
}

__device__ __forceinline__ L9 shfl_l9(const L9& v, int src) {
  L9 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = (uint32_t)__shfl((int)v.l[i], src, 64);
  return r;
}
__device__ __forceinline__ AccL9 shfl_acc_l9(const AccL9& p, int src) {
  AccL9 r;
  r.x = shfl_l9(p.x, src);
  r.y = shfl_l9(p.y, src);
  r.zz = shfl_l9(p.zz, src);
  r.zzz = shfl_l9(p.zzz, src);
  return r;
}
__device__ __forceinline__ AccL9 acc_l9_zero() {
  AccL9 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.x.l[i] = r.y.l[i] = r.zz.l[i] = r.zzz.l[i] = 0;
  return r;
}

// One wavefront per column: result = sum_b b * B_b with B_b = sum of the partials of bucket b.  Everything stays in the
// accumulator's nine-limb form (xyzz_add_l9); the column's sum leaves as one raw record, k_msm_normalise makes it affine.
__global__ __launch_bounds__(64) void k_msm_reduce(const uint4* __restrict__ raw, const uint32_t* __restrict__ task_off, uint32_t c,
                                                   const uint32_t* __restrict__ counters, const Affine* __restrict__ add_points, uint4* __restrict__ sums,
                                                   MsmL9Consts K) {
  if (counters[1]) return;
  const uint32_t B = 1u << (c - 1);
  const uint32_t col = blockIdx.x, lane = threadIdx.x;
  const uint32_t log_per = c - 1 >= 6 ? c - 7 : 0, per = 1u << log_per;
  const uint32_t* toff = task_off + (size_t)col * (B + 1);
  AccL9 running = acc_l9_zero(), total = acc_l9_zero();
  bool run_id = true, tot_id = true;
  const uint32_t lo = lane * per;  // bucket indices [lo, lo+per) <-> bucket ids lo+1 .. lo+per
  if (lo < B) {
    for (int b = (int)(lo + per) - 1; b >= (int)lo; b--) {
      uint32_t t0 = toff[b], t1 = toff[b + 1];
      if (t1 > t0) {  // bucket sum was folded into its first slot by k_msm_combine
        AccL9 p;
        bool p_id;
        ld_raw_l9(raw + (size_t)t0 * (MSM_RAW_WORDS / 4), p, p_id);
        xyzz_add_l9(running, run_id, p, p_id, K);
      }
      xyzz_add_l9(total, tot_id, running, run_id, K);  // (a doubling whenever total still equals running: one bucket so far)
    }
  }
  // total_L = sum (b - lo) * B_b over the lane's ids; running_L = sum B_b.
  // result = sum_L total_L + per * sum_L L * running_L = sum_L (total_L + per * [L >= 1] suf_L)
  // suffix scan of running over lanes: suf_L = sum_{L' >= L} running_L', and sum_{L >= 1} suf_L = sum_L L * running_L
  for (int o = 1; o < 64; o <<= 1) {
    const int src = (int)lane + o < 64 ? (int)lane + o : (int)lane;
    const AccL9 other = shfl_acc_l9(running, src);
    const bool other_id = __shfl((int)run_id, src, 64) != 0;
    if ((int)lane + o < 64) xyzz_add_l9(running, run_id, other, other_id, K);
  }
  // every lane scales its own suffix sum (all lanes double together) and folds it into its total: one accumulator, not two, goes
  // through the tree
  if (lane == 0) run_id = true;
  for (uint32_t d = 0; d < log_per; d++) xyzz_dbl_l9(running, run_id, K);
  xyzz_add_l9(total, tot_id, running, run_id, K);
  for (int o = 32; o >= 1; o >>= 1) {
    const int src = (int)lane + o < 64 ? (int)lane + o : (int)lane;
    const AccL9 other = shfl_acc_l9(total, src);
    const bool other_id = __shfl((int)tot_id, src, 64) != 0;
    if ((int)lane < o) xyzz_add_l9(total, tot_id, other, other_id, K);
  }
  if (lane == 0) {
    if (add_points) {  // + precomputed constant-cell part: a canonical affine point in standard form, times 32 for the accumulator's R'
      Affine ap = ld_affine(add_points + col);
      if (!affine_is_identity(ap)) {
        ap.x = fq_mul(ap.x, K.one_rp);
        ap.y = fq_mul(ap.y, K.one_rp);
        madd_l9(total, tot_id, ap, false, K);
      }
    }
    flush_l9(sums + (size_t)col * (MSM_RAW_WORDS / 4), total, tot_id);
  }
}

// One LANE per column: the column's sum out of the accumulator's form (four products by 2^256: R' -> R, canonical) and to the canonical
// affine point, identity (0, 0).  The Fermat inversion — some 380 dependent products — runs in 64 columns per wavefront here; at the end of
// k_msm_reduce it held a whole wavefront and its registers for one lane's chain.
__global__ __launch_bounds__(64) void k_msm_normalise(const uint4* __restrict__ sums, uint32_t n_cols, const uint32_t* __restrict__ counters, u256 to_std,
                                                      Affine* __restrict__ out) {
  if (counters[1]) return;
  const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= n_cols) return;
  AccL9 a;
  bool ident;
  ld_raw_l9(sums + (size_t)col * (MSM_RAW_WORDS / 4), a, ident);
  XYZZ p = xyzz_identity();
  if (!ident) {
    const L9 ts = l9_split(to_std);
    p.x = l9_canon<Fq>(l9_mul<Fq>(a.x, ts));
    p.y = l9_canon<Fq>(l9_mul<Fq>(a.y, ts));
    p.zz = l9_canon<Fq>(l9_mul<Fq>(a.zz, ts));
    p.zzz = l9_canon<Fq>(l9_mul<Fq>(a.zzz, ts));
  }
  st_affine(out + col, xyzz_to_affine(p));
}


// ---------------------------------------------------------------- test / bench SRS ("unsafe" setup with a known tau)
// g[i] = tau^i * G,  g_lagrange[i] = L_i(tau) * G with L_i(tau) = omega^i (tau^n - 1) / (n (tau - omega^i))
__global__ __launch_bounds__(64) void k_srs_setup(u256 tau, u256 omega, u256 tn_minus_1_over_n, uint64_t n, Affine* __restrict__ g, Affine* __restrict__ gl) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine gen;
  gen.x = to_mont<Fq>(u256_from_u64(1));
  gen.y = to_mont<Fq>(u256_from_u64(2));
  u256 e = u256_from_u64(i);
  u256 ti = mont_pow<Fr>(tau, e), wi = mont_pow<Fr>(omega, e);
  u256 li = fr_mul(fr_mul(wi, tn_minus_1_over_n), mont_inv<Fr>(fr_sub(tau, wi)));
  for (int which = 0; which < 2; which++) {
    u256 k = from_mont<Fr>(which == 0 ? ti : li);
    XYZZ acc = xyzz_identity();
    for (int b = (int)u256_bits(k) - 1; b >= 0; b--) {
      acc = xyzz_double(acc);
      if (u256_bit(k, (unsigned)b)) xyzz_add_mixed(acc, gen, false);
    }
    st_affine((which == 0 ? g : gl) + i, xyzz_to_affine(acc));
  }
}

// out[c] = sum_m parts[m][c]: the combine step of a point-sharded MSM (each rank commits its slice of the rows of every
// column; the partial commitments are gathered and added — SURVEY §8e "alternative")
__global__ __launch_bounds__(64) void k_g1_sum(const Affine* __restrict__ parts, uint32_t m, uint64_t n, Affine* __restrict__ out) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  XYZZ acc = xyzz_identity();
  for (uint32_t i = 0; i < m; i++) xyzz_add_mixed(acc, ld_affine(parts + (uint64_t)i * n + c), false);
  st_affine(out + c, xyzz_to_affine(acc));
}

static_assert(MSM_PLAN_OK == VDB_OK && MSM_PLAN_REFUSED == VDB_ERR_ARG, "msm_plan.hpp returns the C ABI's codes");

// the process's knobs, read from the environment once
static const MsmKnobs& msm_knobs() {
  static const MsmKnobs knobs = [] {
    MsmKnobs k;
    if (const char* e = getenv("VDB_MSM_C")) k.window = (uint32_t)atoi(e);
    return k;
  }();
  return knobs;
}

// One batched MSM: n_cols columns of n scalars against the tables of `srs`, one affine point per column.  A caller sets what it asks
// for by name.
struct MsmCall {
  const vdb_srs* srs = nullptr;
  int basis = 0;
  const u256* scalars = nullptr;       // n_cols x n, contiguous; null with `srcs`
  const ColSrc* srcs = nullptr;        // per column: where it still lies in a witness stream
  uint32_t n_blind = 0;
  size_t n_cols = 0, n = 0;
  Affine* out = nullptr;               // device: n_cols points
  const uint8_t* skip_mask = nullptr;  // n per column: cells left out (their terms are part of add_points)
  const Affine* add_points = nullptr;  // per column: added to its sum
  // the bucket folding of the LAST batch (k_msm_combine, k_msm_reduce, k_msm_normalise) goes to the context's auxiliary stream and
  // the driver returns without waiting; msm_collect() joins
  bool defer_tail = false;
};

// the work space of a batch: the plan's regions as pointers
struct MsmWork {
  uint32_t* entries;
  uint4 *raw, *sums;
  MsmRange* ranges;
  MsmSegInfo* seginfo;
  uint32_t *seg_off, *bucket_off, *counters;
  unsigned long long* recs;
  uint32_t* longq;
  template <class T>
  static T* at(uint8_t* buf, const MsmPlan& P, MsmRegion r) {
    return reinterpret_cast<T*>(buf + P.off[r]);
  }
  MsmWork(uint8_t* buf, const MsmPlan& P)
      : entries(at<uint32_t>(buf, P, MSM_ENTRIES)), raw(at<uint4>(buf, P, MSM_RAW)), sums(at<uint4>(buf, P, MSM_SUMS)),
        ranges(at<MsmRange>(buf, P, MSM_RANGES)), seginfo(at<MsmSegInfo>(buf, P, MSM_SEGINFO)), seg_off(at<uint32_t>(buf, P, MSM_SEG_OFF)),
        bucket_off(at<uint32_t>(buf, P, MSM_BUCKET_OFF)), counters(at<uint32_t>(buf, P, MSM_COUNTERS)),
        recs(at<unsigned long long>(buf, P, MSM_RECS)), longq(at<uint32_t>(buf, P, MSM_LONGQ)) {}
};

// Device-level batched MSM.  Plans the job (msm_plan.hpp: range length, capacities, scatter, batch size under the memory budget, the
// layout of the work space), fetches the work space and runs the batches.
// With `defer_tail` the scalars are no longer read when the function returns, so the caller may overwrite them (NTT in place).  The
// folding is not free on the auxiliary stream: it fills the chip's issue slots
// and registers like any other kernel, and the transform launches that run beside it take longer by most of what it costs
// alone (profiles/NOTES.md, "bucket folding beside the transforms": the first two launches of lagrange_to_coeff, 2.3 and
// 2.1 ms alone, took 4.9 and 6.5 ms beside the eight-word folding and its 213-register k_msm_reduce, 5.1 and 3.4 ms beside
// this one).  What it saves is the dependency: the transforms need not wait for the commitments.
static int msm_batch_dev(const MsmCall& m) {
  Context& cx = ctx();
  const bool defer_tail = m.defer_tail && g_prof_mode != 1;  // per-kernel timing serialises on the main stream
  if (cx.msm_pending) {
    set_error("msm: a deferred batch has not been collected (vdb_msm_batch_end)");
    return VDB_ERR_ARG;
  }
  const size_t n_cols = m.n_cols, n = m.n;
  if (n_cols == 0) return VDB_OK;
  const vdb_srs* srs = m.srs;
  const Affine* table = srs->table[m.basis];
  const uint32_t c = srs->c, W = srs->W, B = srs->B;
  MsmMem mem = {0, cx.scratch_bytes[2], cx.msm_scratch_cap};
  size_t total_b = 0;
  if (hipMemGetInfo(&mem.free_bytes, &total_b) != hipSuccess) mem.free_bytes = (size_t)80 << 30;
  MsmPlan P;
  const char* why = nullptr;
  if (int rc = msm_plan(MsmShape{c, W, B, srs->n}, MsmJob{n_cols, n}, mem, &P, &why)) {
    set_error("%s", why);
    return rc;
  }
  uint8_t* buf = (uint8_t*)scratch_get(2, P.bytes);
  if (!buf) return VDB_ERR_OOM;
  const MsmWork w(buf, P);
  MsmL9Consts l9k;
  l9_offset_limbs<FqParams>(2, l9k.c2);
  l9_offset_limbs<FqParams>(8, l9k.c8);
  l9k.one_rp = to_mont<Fq>(u256_from_u64(32));
  l9k.to_std = mont_one<Fq>();
  l9k.to_rp = to_mont<Fq>(u256_from_u64(1024));
  for (size_t c0 = 0; c0 < n_cols; c0 += P.nb) {
    size_t nc = n_cols - c0 < P.nb ? n_cols - c0 : P.nb;
    // counters[1], the overflow flag, is read once after the last batch: cleared before the first batch only, so that an overflow
    // in any batch (whose k_msm_reduce leaves its points unwritten) still fails the call; the other three words are per batch
    if (c0 == 0) {
      VDB_HIP(hipMemsetAsync(w.counters, 0, 4 * sizeof(uint32_t), cx.stream));
    } else {
      VDB_HIP(hipMemsetAsync(w.counters, 0, sizeof(uint32_t), cx.stream));
      VDB_HIP(hipMemsetAsync(w.counters + 2, 0, 2 * sizeof(uint32_t), cx.stream));
    }
    {
      VDB_PROF("k_msm_sort");
      hipLaunchKernelGGL(k_msm_sort, dim3((unsigned)nc), dim3(MSM_SORT_THREADS), P.sort_lds, cx.stream, m.scalars ? m.scalars + c0 * n : nullptr,
                       m.srcs ? m.srcs + c0 : nullptr, m.n_blind, n, srs->n, c, W, w.entries,
                       P.ent_cap, w.seg_off, w.bucket_off, w.ranges, w.counters, P.seg_cap, P.range_cap, m.skip_mask ? m.skip_mask + c0 * n : nullptr,
                       P.lcap, w.longq, w.recs, P.fine_bits, P.idx_bits, P.bin_cap);
    }
    VDB_LAUNCH_CHECK();
    if (P.fine_bits) {
      VDB_PROF("k_msm_scatter2");
      hipLaunchKernelGGL(k_msm_scatter2, dim3(P.scatter2_bins_x, (unsigned)nc), dim3(MSM_SCATTER2_THREADS), P.scatter2_lds, cx.stream,
                       w.entries, P.ent_cap, w.bucket_off, B, P.fine_bits, P.idx_bits, P.bin_cap, w.counters);
    }
    VDB_LAUNCH_CHECK();
    {
      VDB_PROF("k_msm_accum");
      hipLaunchKernelGGL(k_msm_accum, dim3((unsigned)(cx.cu_count * 8)), dim3(256), 0, cx.stream, table, w.entries, P.ent_cap, w.ranges, w.bucket_off, B,
                       w.seg_off, w.counters, w.raw, w.seginfo, P.range_cap, l9k);
    }
    VDB_LAUNCH_CHECK();
    hipStream_t ts = cx.stream;
    if (defer_tail && c0 + nc == n_cols) {
      VDB_HIP(hipEventRecord(cx.ev_tail, cx.stream));
      VDB_HIP(hipStreamWaitEvent(cx.aux, cx.ev_tail, 0));
      ts = cx.aux;
    }
    for (uint32_t ps = 0; ps < P.combine_passes; ps++) {
      VDB_PROF_ON("k_msm_combine", ts);
      hipLaunchKernelGGL(k_msm_combine, dim3((unsigned)(cx.cu_count * 8)), dim3(256), 0, ts, w.raw, w.seginfo, w.counters, ps, P.seg_cap, l9k);
    }
    VDB_LAUNCH_CHECK();
    {
      VDB_PROF_ON("k_msm_reduce", ts);
      hipLaunchKernelGGL(k_msm_reduce, dim3((unsigned)nc), dim3(64), 0, ts, w.raw, w.seg_off, c, w.counters, m.add_points ? m.add_points + c0 : nullptr, w.sums, l9k);
    }
    VDB_LAUNCH_CHECK();
    {
      VDB_PROF_ON("k_msm_normalise", ts);
      hipLaunchKernelGGL(k_msm_normalise, dim3((unsigned)((nc + 63) / 64)), dim3(64), 0, ts, w.sums, (uint32_t)nc, w.counters, l9k.to_std, m.out + c0);
    }
    VDB_LAUNCH_CHECK();
  }
  if (defer_tail) {
    cx.msm_pending = true;
    cx.msm_counters = w.counters;
    return VDB_OK;
  }
  uint32_t h_counters[2] = {0, 0};
  VDB_HIP(hipMemcpyAsync(h_counters, w.counters, sizeof(h_counters), hipMemcpyDeviceToHost, cx.stream));
  VDB_HIP(hipStreamSynchronize(cx.stream));
  if (h_counters[1]) {
    set_error("msm: internal task buffer overflow");
    return VDB_ERR_HIP;
  }
  return VDB_OK;
}

// joins a deferred batch: both streams drained, overflow flag checked
static int msm_collect() {
  Context& cx = ctx();
  if (!cx.msm_pending) return VDB_OK;
  cx.msm_pending = false;
  if (!cx.msm_counters) {  // the batch ran synchronously (profiling): nothing left to check
    VDB_HIP(hipStreamSynchronize(cx.aux));
    VDB_HIP(hipStreamSynchronize(cx.stream));
    return VDB_OK;
  }
  // the auxiliary stream is ordered after the batch's main-stream kernels (ev_tail): reading the flag there does not wait
  // for whatever the caller queued on the main stream behind the MSM (the NTTs of the same columns)
  uint32_t h_counters[2] = {0, 0};
  VDB_HIP(hipMemcpyAsync(h_counters, cx.msm_counters, sizeof(h_counters), hipMemcpyDeviceToHost, cx.aux));
  cx.msm_counters = nullptr;
  VDB_HIP(hipStreamSynchronize(cx.aux));
  if (h_counters[1]) {
    set_error("msm: internal task buffer overflow");
    return VDB_ERR_HIP;
  }
  return VDB_OK;
}

}  // namespace vdb

using namespace vdb;

extern "C" {

int vdb_srs_setup_unsafe(uint32_t k, const vdb_fr* tau, vdb_g1* g_out, vdb_g1* g_lagrange_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(tau && g_out && g_lagrange_out && k >= 1 && k <= 22, "bad argument");
  Context& cx = ctx();
  const uint64_t n = 1ull << k;
  u256 t;
  memcpy(&t, tau, 32);
  u256 omega = host_root_of_unity(k);
  u256 tn = mont_pow<Fr>(t, u256_from_u64(n));
  u256 c = fr_mul(fr_sub(tn, mont_one<Fr>()), mont_inv<Fr>(host_fr_from_u64(n)));
  Affine* d = (Affine*)scratch_get(0, 2 * n * sizeof(Affine));
  if (!d) return VDB_ERR_OOM;
  {
    VDB_PROF("k_srs_setup");
    hipLaunchKernelGGL(k_srs_setup, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, cx.stream, t, omega, c, n, d, d + n);
  }
  VDB_LAUNCH_CHECK();
  VDB_HIP(hipMemcpyAsync(g_out, d, n * sizeof(Affine), hipMemcpyDeviceToHost, cx.stream));
  VDB_HIP(hipMemcpyAsync(g_lagrange_out, d + n, n * sizeof(Affine), hipMemcpyDeviceToHost, cx.stream));
  VDB_HIP(hipStreamSynchronize(cx.stream));
  return VDB_OK;
}

int vdb_srs_load(uint32_t k, const vdb_g1* g, const vdb_g1* g_lagrange, vdb_srs** out) { return vdb_srs_load_window(k, g, g_lagrange, 0, out); }
int vdb_srs_load_window(uint32_t k, const vdb_g1* g, const vdb_g1* g_lagrange, uint32_t window_bits, vdb_srs** out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(out && (g || g_lagrange) && k >= 1 && k <= 24, "bad argument");
  MsmShape shape;
  const char* why = nullptr;
  if (int rc = msm_window(k, window_bits, msm_knobs(), &shape, &why)) {
    set_error("%s", why);
    return rc;
  }
  Context& cx = ctx();
  vdb_srs* s = new vdb_srs();
  s->device = cx.device;
  s->k = k;
  s->n = shape.table_n;
  s->c = shape.c;
  s->W = shape.W;
  s->B = shape.B;
  s->table[0] = s->table[1] = nullptr;
  const vdb_g1* src[2] = {g, g_lagrange};
  for (int b = 0; b < 2; b++) {
    if (!src[b]) continue;
    Affine* bases = (Affine*)scratch_get(0, s->n * sizeof(Affine));
    if (!bases) {
      vdb_srs_free(s);
      return VDB_ERR_OOM;
    }
    hipError_t e = hipMalloc(&s->table[b], (size_t)s->W * s->n * sizeof(Affine));
    if (e != hipSuccess) {
      vdb_srs_free(s);
      return hip_fail(e, "hipMalloc(srs table)", __FILE__, __LINE__);
    }
    VDB_HIP(hipMemcpyAsync(bases, src[b], s->n * sizeof(Affine), hipMemcpyHostToDevice, cx.stream));
    {
      VDB_PROF("k_srs_table");
      hipLaunchKernelGGL(k_srs_table, dim3((unsigned)((s->n + 255) / 256)), dim3(256), 0, cx.stream, bases, s->table[b], s->n, s->c, s->W);
    }
    VDB_LAUNCH_CHECK();
    VDB_HIP(hipStreamSynchronize(cx.stream));
  }
  *out = s;
  return VDB_OK;
}
int vdb_g1_sum(const vdb_g1* parts, size_t m, size_t n, vdb_g1* out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(parts && out && m >= 1 && m <= 0xffffffffull, "bad argument");
  if (n == 0) return VDB_OK;
  Context& cx = ctx();
  Affine* d = (Affine*)scratch_get(0, (m + 1) * n * sizeof(Affine));
  if (!d) return VDB_ERR_OOM;
  VDB_HIP(hipMemcpyAsync(d, parts, m * n * sizeof(Affine), hipMemcpyHostToDevice, cx.stream));
  {
    VDB_PROF("k_g1_sum");
    hipLaunchKernelGGL(k_g1_sum, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, cx.stream, d, (uint32_t)m, (uint64_t)n, d + m * n);
  }
  VDB_LAUNCH_CHECK();
  VDB_HIP(hipMemcpyAsync(out, d + m * n, n * sizeof(Affine), hipMemcpyDeviceToHost, cx.stream));
  VDB_HIP(hipStreamSynchronize(cx.stream));
  return VDB_OK;
}
void vdb_srs_free(vdb_srs* s) {
  if (!s) return;
  int cur = -1;
  const bool hop = hipGetDevice(&cur) == hipSuccess && cur != vdb::phys_of(s->device) && hipSetDevice(vdb::phys_of(s->device)) == hipSuccess;
  for (int b = 0; b < 2; b++)
    if (s->table[b]) (void)hipFree(s->table[b]);
  if (hop) (void)hipSetDevice(cur);
  delete s;
}
int vdb_srs_device(const vdb_srs* s, int* device) {
  VDB_ARG(s && device, "null pointer");
  *device = s->device;
  return VDB_OK;
}
int vdb_srs_info(const vdb_srs* s, uint32_t* k, uint32_t* window_bits, uint32_t* windows) {
  VDB_ARG(s, "null srs");
  if (k) *k = s->k;
  if (window_bits) *window_bits = s->c;
  if (windows) *windows = s->W;
  return VDB_OK;
}

// The results of a deferred batch stay in a buffer of their own until vdb_msm_batch_end: the shared scratch slots remain
// free for whatever the caller queues in between (slot 2, where the batch's bucket folding is still at work on the second
// stream, is refused to everybody else while the batch is open: scratch_get).
static void* deferred_out(size_t bytes) {
  Context& c = ctx();
  if (c.msm_out_bytes >= bytes && c.msm_out_buf) return c.msm_out_buf;
  if (c.msm_out_buf) (void)hipFree(c.msm_out_buf);
  c.msm_out_buf = nullptr;
  c.msm_out_bytes = 0;
  hipError_t e = hipMalloc(&c.msm_out_buf, bytes + bytes / 8 + 64);
  if (e != hipSuccess) {
    hip_fail(e, "hipMalloc(deferred MSM output)", __FILE__, __LINE__);
    return nullptr;
  }
  c.msm_out_bytes = bytes + bytes / 8 + 64;
  return c.msm_out_buf;
}
// What the device entry points refuse, in this order.  `ptrs_ok`: the entry point's own pointers are given; `n_msg`: its words for a bad n.
static int msm_check_call(const MsmCall& m, bool ptrs_ok, const char* n_msg = "n exceeds the loaded SRS size") {
  VDB_REQUIRE_INIT();
  VDB_ARG(m.srs && ptrs_ok && (m.basis == 0 || m.basis == 1), "bad argument");
  VDB_SRS_HERE(m.srs);
  VDB_ARG(m.srs->table[m.basis], "srs was loaded without this basis");
  VDB_ARG(m.n <= m.srs->n && m.n > 0 && m.n_blind <= m.n, n_msg);
  VDB_ARG((m.skip_mask == nullptr) == (m.add_points == nullptr), "mask and constant points go together");
  return VDB_OK;
}
// the synchronous forms: the points go through scratch slot 1 to the host
static int msm_to_host(MsmCall m, vdb_g1* out_host) {
  if (m.n_cols == 0) return VDB_OK;
  m.out = (Affine*)scratch_get(1, m.n_cols * sizeof(Affine));
  if (!m.out) return VDB_ERR_OOM;
  int rc = msm_batch_dev(m);
  if (rc) return rc;
  VDB_HIP(hipMemcpyAsync(out_host, m.out, m.n_cols * sizeof(Affine), hipMemcpyDeviceToHost, ctx().stream));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}
// the _begin forms: the points go to the deferred batch's own buffer, the tail of the last batch to the auxiliary stream
static int msm_begin(MsmCall m) {
  if (m.n_cols == 0) return VDB_OK;
  // refused before the output buffer is touched: a wider second batch would re-allocate it under the batch that is still open
  VDB_ARG(!ctx().msm_pending, "msm: a deferred batch has not been collected (vdb_msm_batch_end)");
  m.out = (Affine*)deferred_out(m.n_cols * sizeof(Affine));
  if (!m.out) return VDB_ERR_OOM;
  ctx().msm_out = m.out;
  m.defer_tail = true;
  int rc = msm_batch_dev(m);
  if (rc == VDB_OK && !ctx().msm_pending) ctx().msm_pending = true;  // profiling mode ran it synchronously: _end still copies out
  return rc;
}
static MsmCall msm_call(const vdb_srs* srs, int basis, const vdb_fr* scalars_dev, size_t n_cols, size_t n, const uint8_t* skip_mask_dev = nullptr,
                        const vdb_g1* const_points_dev = nullptr) {
  MsmCall m;
  m.srs = srs;
  m.basis = basis;
  m.scalars = as_u256(scalars_dev);
  m.n_cols = n_cols;
  m.n = n;
  m.skip_mask = skip_mask_dev;
  m.add_points = reinterpret_cast<const Affine*>(const_points_dev);
  return m;
}
int vdb_msm_batch_dev(const vdb_srs* srs, int basis, const vdb_fr* scalars_dev, size_t n_cols, size_t n, vdb_g1* out_host) {
  const MsmCall m = msm_call(srs, basis, scalars_dev, n_cols, n);
  if (int rc = msm_check_call(m, scalars_dev && out_host, "n exceeds the loaded SRS size (shorter columns are allowed)")) return rc;
  return msm_to_host(m, out_host);
}
int vdb_msm_count_entries_dev(const vdb_srs* srs, const vdb_fr* scalars_dev, size_t n_cols, size_t n, const uint8_t* skip_mask_dev, uint64_t* counts_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(srs && scalars_dev && counts_out && n <= srs->n, "bad argument");
  VDB_SRS_HERE(srs);
  if (n_cols == 0) return VDB_OK;
  Context& cx = ctx();
  unsigned long long* d = (unsigned long long*)scratch_get(2, n_cols * sizeof(unsigned long long));
  if (!d) return VDB_ERR_OOM;
  VDB_HIP(hipMemsetAsync(d, 0, n_cols * sizeof(unsigned long long), cx.stream));
  {
    VDB_PROF("k_msm_count_entries");
    hipLaunchKernelGGL(k_msm_count_entries, dim3((unsigned)n_cols), dim3(256), 0, cx.stream, as_u256(scalars_dev), skip_mask_dev, (uint64_t)n, srs->c, srs->W, d);
  }
  VDB_LAUNCH_CHECK();
  VDB_HIP(hipMemcpyAsync(counts_out, d, n_cols * sizeof(uint64_t), hipMemcpyDeviceToHost, cx.stream));
  VDB_HIP(hipStreamSynchronize(cx.stream));
  return VDB_OK;
}
int vdb_msm_batch_masked_dev_begin(const vdb_srs* srs, int basis, const vdb_fr* scalars_dev, size_t n_cols, size_t n, const uint8_t* skip_mask_dev,
                                   const vdb_g1* const_points_dev) {
  const MsmCall m = msm_call(srs, basis, scalars_dev, n_cols, n, skip_mask_dev, const_points_dev);
  if (int rc = msm_check_call(m, scalars_dev)) return rc;
  return msm_begin(m);
}
int vdb_msm_batch_src_dev_begin(const vdb_srs* srs, int basis, const vdb_colsrc* src_dev, size_t n_cols, size_t n, uint32_t n_blind,
                                const uint8_t* skip_mask_dev, const vdb_g1* const_points_dev) {
  MsmCall m = msm_call(srs, basis, nullptr, n_cols, n, skip_mask_dev, const_points_dev);
  m.srcs = reinterpret_cast<const ColSrc*>(src_dev);
  m.n_blind = n_blind;
  if (int rc = msm_check_call(m, src_dev)) return rc;
  return msm_begin(m);
}
int vdb_msm_batch_end(vdb_g1* out_host, size_t n_cols) {
  VDB_REQUIRE_INIT();
  VDB_ARG(out_host || n_cols == 0, "null pointer");
  int rc = msm_collect();
  if (rc) return rc;
  if (n_cols == 0) return VDB_OK;
  const void* dout = ctx().msm_out;
  VDB_ARG(dout, "no deferred MSM to collect");
  // on the auxiliary stream, where the points were produced: work queued on the main stream after _begin keeps running
  VDB_HIP(hipMemcpyAsync(out_host, dout, n_cols * sizeof(Affine), hipMemcpyDeviceToHost, ctx().aux));
  VDB_HIP(hipStreamSynchronize(ctx().aux));
  return VDB_OK;
}
int vdb_msm_batch_masked_dev(const vdb_srs* srs, int basis, const vdb_fr* scalars_dev, size_t n_cols, size_t n, const uint8_t* skip_mask_dev,
                             const vdb_g1* const_points_dev, vdb_g1* out_host) {
  const MsmCall m = msm_call(srs, basis, scalars_dev, n_cols, n, skip_mask_dev, const_points_dev);
  if (int rc = msm_check_call(m, scalars_dev && out_host && skip_mask_dev && const_points_dev)) return rc;
  return msm_to_host(m, out_host);
}
int vdb_msm_batch(const vdb_srs* srs, int basis, const vdb_fr* const* cols, size_t n_cols, size_t n, vdb_g1* out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(srs && cols && out, "null pointer");
  if (n_cols == 0) return VDB_OK;
  u256* d = (u256*)scratch_get(0, n_cols * n * sizeof(u256));
  if (!d) return VDB_ERR_OOM;
  for (size_t i = 0; i < n_cols; i++) VDB_HIP(hipMemcpyAsync(d + i * n, cols[i], n * sizeof(u256), hipMemcpyHostToDevice, ctx().stream));
  return vdb_msm_batch_dev(srs, basis, reinterpret_cast<const vdb_fr*>(d), n_cols, n, out);
}
int vdb_msm(const vdb_srs* srs, int basis, const vdb_fr* scalars, size_t n, vdb_g1* out) {
  const vdb_fr* cols[1] = {scalars};
  return vdb_msm_batch(srs, basis, cols, 1, n, out);
}

}  // extern "C"
