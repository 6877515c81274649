// The verifier's two data-parallel steps (the Verify arm; halo2's verify_proof / read_snark):
//   * vdb_g1_decompress_dev: every compressed point of a proof, one lane per point — y = (x^3 + 3)^((q+1)/4), q = 3 mod 4;
//   * vdb_msm_points_dev: one multi-scalar multiplication over arbitrary affine points (the folded-h commitment and the SHPLONK
//     left-hand side together).  The bases are used once, so unlike msm.hip there are no precomputed window tables: a plain
//     variable-base Pippenger with c-bit unsigned windows and c doublings between windows.
// Stages of the MSM (all on ctx().stream):
//   k_vmsm_count    one lane per point: canonical scalar, histogram of the (window, digit) buckets it falls in
//   k_vmsm_scan     one workgroup: exclusive scan of the histogram -> each bucket's slice of the entry list
//   k_vmsm_scatter  one lane per point: its index into the slice of each of its buckets
//   k_vmsm_accum    one lane per bucket: the sum of its points (mixed XYZZ additions; every exceptional case exact, ec.hpp)
//   k_vmsm_segment  one lane per run of SEG buckets of a window: sum_d d B_d over the run (running sums + a short scalar multiple)
//   k_vmsm_window   one lane per window: the sum of its runs
//   k_vmsm_final    one lane: Horner over the windows, c doublings each, then affine
// The result is a group element; the order in which a bucket's points arrive does not change it.
#include "common.hpp"
#include "ec.hpp"

using namespace vdb;

namespace {

constexpr uint32_t SCALAR_BITS = 254;   // r < 2^254
constexpr uint32_t SEG = 32;            // buckets per lane of k_vmsm_segment
constexpr uint32_t SCAN_THREADS = 1024;

// (q + 1) / 4, canonical
__device__ __forceinline__ u256 sqrt_exponent() {
  u256 e;
  const uint32_t P[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
  // (q + 1) >> 2 limb by limb: q + 1 has no carry out of limb 0 (q is odd and its low limb is not 0xffffffff)
  uint32_t lo0 = P[0] + 1u;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t cur = i == 0 ? lo0 : P[i];
    const uint32_t nxt = i < 7 ? P[i + 1] : 0u;
    e.w[i] = (cur >> 2) | (nxt << 30);
  }
  return e;
}

__global__ __launch_bounds__(256) void k_g1_decompress(const uint8_t* __restrict__ enc, size_t n, uint32_t sign_bit, Affine* __restrict__ out,
                                                       uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* e = enc + 32 * i;
  u256 x;
#pragma unroll
  for (int k = 0; k < 8; k++)
    x.w[k] = (uint32_t)e[4 * k] | ((uint32_t)e[4 * k + 1] << 8) | ((uint32_t)e[4 * k + 2] << 16) | ((uint32_t)e[4 * k + 3] << 24);
  const uint32_t sign_mask = 1u << (24 + sign_bit);       // the flag's bit in the top limb
  const bool odd = (x.w[7] & sign_mask) != 0;
  x.w[7] &= ~sign_mask;
  Affine p;
  p.x = u256_zero();
  p.y = u256_zero();
  uint8_t st = VDB_G1_OK;
  if (u256_is_zero(x)) {
    // x = 0 is on no point of the curve (3 is not a square mod q): only the all-zero encoding, the identity, is valid
    if (odd) st = VDB_G1_BAD_IDENTITY;
  } else if ((x.w[7] >> 30) != 0 || u256_geq(x, mod_p<Fq>())) {
    st = u256_is_zero(u256_low_bits(x, 254)) ? VDB_G1_BAD_IDENTITY : VDB_G1_NONCANONICAL;
  } else {
    const u256 xm = to_mont<Fq>(x);
    const u256 rhs = fq_add(fq_mul(fq_sqr(xm), xm), to_mont<Fq>(u256_from_u64(3)));
    u256 y = mont_pow<Fq>(rhs, sqrt_exponent());
    if (!u256_eq(fq_sqr(y), rhs)) {
      st = VDB_G1_NOT_ON_CURVE;
    } else {
      if (((from_mont<Fq>(y).w[0] & 1u) != 0) != odd) y = fq_neg(y);
      p.x = xm;
      p.y = y;
    }
  }
  st_affine(out + i, p);
  status[i] = st;
}

__device__ __forceinline__ uint32_t digit(const u256& s, uint32_t w, uint32_t c) {
  const uint32_t bit = w * c, limb = bit >> 5, off = bit & 31;
  uint64_t v = s.w[limb];
  if (limb + 1 < 8) v |= (uint64_t)s.w[limb + 1] << 32;
  return (uint32_t)(v >> off) & ((1u << c) - 1u);
}

__global__ __launch_bounds__(256) void k_vmsm_count(const Affine* __restrict__ pts, const u256* __restrict__ scalars, size_t n, uint32_t c, uint32_t W,
                                                    u256* __restrict__ canon, uint32_t* __restrict__ counts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u256 s = from_mont<Fr>(ld256(scalars + i));
  if (affine_is_identity(ld_affine(pts + i))) s = u256_zero();   // contributes nothing: keep it out of every bucket
  st256(canon + i, s);
  const uint32_t nb = 1u << c;
  for (uint32_t w = 0; w < W; w++) {
    const uint32_t d = digit(s, w, c);
    if (d) atomicAdd(counts + (size_t)w * nb + d, 1u);
  }
}

// exclusive scan of m counters in one workgroup: off[b] = sum of counts[< b], cursor[b] = off[b]
__global__ __launch_bounds__(SCAN_THREADS) void k_vmsm_scan(const uint32_t* __restrict__ counts, size_t m, uint32_t* __restrict__ off,
                                                            uint32_t* __restrict__ cursor) {
  __shared__ uint32_t part[SCAN_THREADS];
  const size_t per = (m + SCAN_THREADS - 1) / SCAN_THREADS, lo = threadIdx.x * per, hi = lo + per < m ? lo + per : m;
  uint32_t sum = 0;
  for (size_t b = lo; b < hi; b++) sum += counts[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < SCAN_THREADS; d <<= 1) {     // Hillis–Steele inclusive scan of the per-lane totals
    const uint32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - sum;
  for (size_t b = lo; b < hi; b++) {
    off[b] = run;
    cursor[b] = run;
    run += counts[b];
  }
}

__global__ __launch_bounds__(256) void k_vmsm_scatter(const u256* __restrict__ canon, size_t n, uint32_t c, uint32_t W, uint32_t* __restrict__ cursor,
                                                      uint32_t* __restrict__ entries) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u256 s = ld256(canon + i);
  const uint32_t nb = 1u << c;
  for (uint32_t w = 0; w < W; w++) {
    const uint32_t d = digit(s, w, c);
    if (d) entries[atomicAdd(cursor + (size_t)w * nb + d, 1u)] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(256) void k_vmsm_accum(const Affine* __restrict__ pts, const uint32_t* __restrict__ entries, const uint32_t* __restrict__ off,
                                                    const uint32_t* __restrict__ counts, size_t m, XYZZ* __restrict__ buckets) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= m) return;
  XYZZ acc = xyzz_identity();
  const uint32_t o = off[b], cnt = counts[b];
  for (uint32_t k = 0; k < cnt; k++) xyzz_add_mixed(acc, ld_affine(pts + entries[o + k]), false);
  st_xyzz(buckets + b, acc);
}

// lane (w, g): buckets d in [lo, hi) = [max(1, g SEG), min(nb, (g + 1) SEG)) of window w;
// sum_{d in run} d B_d = sum_{j} (running sums from the top) + (lo - 1) (sum of the run)
__global__ __launch_bounds__(64) void k_vmsm_segment(const XYZZ* __restrict__ buckets, uint32_t c, uint32_t W, uint32_t n_seg, XYZZ* __restrict__ seg_out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W * n_seg) return;
  const uint32_t w = t / n_seg, g = t % n_seg, nb = 1u << c;
  const uint32_t lo = g * SEG > 1u ? g * SEG : 1u, hi = (g + 1) * SEG < nb ? (g + 1) * SEG : nb;
  XYZZ running = xyzz_identity(), acc = xyzz_identity();
  for (uint32_t d = hi; d-- > lo;) {
    xyzz_add(running, ld_xyzz(buckets + (size_t)w * nb + d));
    xyzz_add(acc, running);
  }
  // + (lo - 1) running, double-and-add from the top bit
  const uint32_t k = lo - 1;
  XYZZ mul = xyzz_identity();
  for (int bit = 13; bit >= 0; bit--) {          // lo - 1 < nb <= 2^13
    mul = xyzz_double(mul);
    if ((k >> bit) & 1u) xyzz_add(mul, running);
  }
  xyzz_add(acc, mul);
  st_xyzz(seg_out + t, acc);
}

__global__ __launch_bounds__(64) void k_vmsm_window(const XYZZ* __restrict__ seg_out, uint32_t W, uint32_t n_seg, XYZZ* __restrict__ win_out) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  XYZZ acc = xyzz_identity();
  for (uint32_t g = 0; g < n_seg; g++) xyzz_add(acc, ld_xyzz(seg_out + (size_t)w * n_seg + g));
  st_xyzz(win_out + w, acc);
}

__global__ __launch_bounds__(64) void k_vmsm_final(const XYZZ* __restrict__ win_out, uint32_t c, uint32_t W, Affine* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  XYZZ acc = xyzz_identity();
  for (uint32_t w = W; w-- > 0;) {
    for (uint32_t k = 0; k < c; k++) acc = xyzz_double(acc);
    xyzz_add(acc, ld_xyzz(win_out + w));
  }
  st_affine(out, xyzz_to_affine(acc));
}

// the window width: ~log2(n) - 3 bits (two bucket additions per bucket against ~W n / 2^c point additions), 4 .. 13
uint32_t vmsm_window(size_t n) {
  uint32_t lg = 0;
  while (lg < 63 && (size_t(1) << (lg + 1)) <= n) lg++;
  const uint32_t c = lg > 7 ? lg - 3 : 4;
  return c > 13 ? 13 : c;
}

}  // namespace

extern "C" {

int vdb_g1_decompress_dev(const uint8_t* enc_dev, size_t n, uint32_t sign_bit, vdb_g1* out_dev, uint8_t* status_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(sign_bit == 6 || sign_bit == 7, "sign_bit must be 6 or 7");
  if (n == 0) return VDB_OK;
  VDB_ARG(enc_dev && out_dev && status_dev, "null pointer");
  Context& cx = ctx();
  VDB_LAUNCH(k_g1_decompress, dim3((unsigned)((n + 255) / 256)), dim3(256), enc_dev, n, sign_bit, reinterpret_cast<Affine*>(out_dev), status_dev);
  VDB_HIP(hipStreamSynchronize(cx.stream));
  return VDB_OK;
}

int vdb_msm_points_dev(const vdb_g1* points_dev, const vdb_fr* scalars_dev, size_t n, vdb_g1* out_host) {
  VDB_REQUIRE_INIT();
  VDB_ARG(out_host, "null pointer");
  if (n == 0) {
    memset(out_host, 0, sizeof(vdb_g1));
    return VDB_OK;
  }
  VDB_ARG(points_dev && scalars_dev, "null pointer");
  Context& cx = ctx();
  const uint32_t c = vmsm_window(n), W = (SCALAR_BITS + c - 1) / c, nb = 1u << c;
  const uint32_t n_seg = (nb + SEG - 1) / SEG;
  const size_t m = (size_t)W * nb;
  VDB_ARG(n * W < (size_t(1) << 32), "too many points for 32-bit entry offsets");
  const size_t b_canon = n * sizeof(u256), b_counts = m * 4, b_entries = n * W * 4, b_buckets = m * sizeof(XYZZ),
               b_seg = (size_t)W * n_seg * sizeof(XYZZ), b_win = W * sizeof(XYZZ);
  const size_t total = b_canon + 3 * b_counts + b_entries + b_buckets + b_seg + b_win + sizeof(Affine) + 16 * 256;   // nine slices, each rounded up to 256 bytes
  char* base = nullptr;
  VDB_HIP(timed_malloc(reinterpret_cast<void**>(&base), total));
  size_t at = 0;
  auto carve = [&](size_t bytes) {
    char* p = base + at;
    at += (bytes + 255) & ~size_t(255);
    return p;
  };
  u256* canon = reinterpret_cast<u256*>(carve(b_canon));
  uint32_t* counts = reinterpret_cast<uint32_t*>(carve(b_counts));
  uint32_t* off = reinterpret_cast<uint32_t*>(carve(b_counts));
  uint32_t* cursor = reinterpret_cast<uint32_t*>(carve(b_counts));
  uint32_t* entries = reinterpret_cast<uint32_t*>(carve(b_entries));
  XYZZ* buckets = reinterpret_cast<XYZZ*>(carve(b_buckets));
  XYZZ* seg_out = reinterpret_cast<XYZZ*>(carve(b_seg));
  XYZZ* win_out = reinterpret_cast<XYZZ*>(carve(b_win));
  Affine* res = reinterpret_cast<Affine*>(carve(sizeof(Affine)));
  const Affine* pts = reinterpret_cast<const Affine*>(points_dev);
  const unsigned blocks = (unsigned)((n + 255) / 256);
  int rc = VDB_OK;
  auto launch_check = [&]() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess && rc == VDB_OK) rc = hip_fail(e, "kernel launch", __FILE__, __LINE__);
  };
  if (hipMemsetAsync(counts, 0, b_counts, cx.stream) != hipSuccess) rc = hip_fail(hipGetLastError(), "hipMemsetAsync", __FILE__, __LINE__);
  if (rc == VDB_OK) {
    {
      VDB_PROF("k_vmsm_count");
      hipLaunchKernelGGL(k_vmsm_count, dim3(blocks), dim3(256), 0, cx.stream, pts, as_u256(scalars_dev), n, c, W, canon, counts);
      launch_check();
    }
    {
      VDB_PROF("k_vmsm_scan");
      hipLaunchKernelGGL(k_vmsm_scan, dim3(1), dim3(SCAN_THREADS), 0, cx.stream, counts, m, off, cursor);
      launch_check();
    }
    {
      VDB_PROF("k_vmsm_scatter");
      hipLaunchKernelGGL(k_vmsm_scatter, dim3(blocks), dim3(256), 0, cx.stream, canon, n, c, W, cursor, entries);
      launch_check();
    }
    {
      VDB_PROF("k_vmsm_accum");
      hipLaunchKernelGGL(k_vmsm_accum, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, cx.stream, pts, entries, off, counts, m, buckets);
      launch_check();
    }
    {
      VDB_PROF("k_vmsm_segment");
      hipLaunchKernelGGL(k_vmsm_segment, dim3((W * n_seg + 63) / 64), dim3(64), 0, cx.stream, buckets, c, W, n_seg, seg_out);
      launch_check();
    }
    {
      VDB_PROF("k_vmsm_window");
      hipLaunchKernelGGL(k_vmsm_window, dim3((W + 63) / 64), dim3(64), 0, cx.stream, seg_out, W, n_seg, win_out);
      launch_check();
    }
    {
      VDB_PROF("k_vmsm_final");
      hipLaunchKernelGGL(k_vmsm_final, dim3(1), dim3(64), 0, cx.stream, win_out, c, W, res);
      launch_check();
    }
  }
  if (rc == VDB_OK) {
    hipError_t e = hipMemcpyAsync(out_host, res, sizeof(Affine), hipMemcpyDeviceToHost, cx.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(cx.stream);
    if (e != hipSuccess) rc = hip_fail(e, "msm_points result", __FILE__, __LINE__);
  }
  (void)hipStreamSynchronize(cx.stream);
  (void)hipFree(base);
  return rc;
}

}  // extern "C"
