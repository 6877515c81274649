// The SRS from a params file (include/vdb.h b1): what halo2's ParamsKZG::read and ParamsKZG::downsize do to the points.
//   * vdb_g1_check_dev: the checks of the RawBytes point reader — both coordinates below q, y^2 = x^3 + 3, (0, 0) the identity —
//     one lane per point.
//   * vdb_g1_lagrange_from_monomial_dev (halo2 g_to_lagrange): g_lagrange[i] = n^-1 sum_j omega^-ij g[j] for n = 2^k affine
//     points, an inverse DFT over G1 in which every twiddle product is a scalar multiplication.
// The DFT is a radix-2 Stockham transform, one launch per stage, points in XYZZ form (ec.hpp) in two ping-pong buffers:
//   stage Ns = 1, 2, 4, .. n/2, butterfly t < n/2:  R = n / (2 Ns), jmod = t / R, q = t % R, j = q Ns + jmod
//       a = in[j], b = in[j + n/2] * omega^-(jmod R);  out[2 q Ns + jmod] = a + b, out[2 q Ns + jmod + Ns] = a - b
// which leaves the result in natural order (no bit reversal).  Consecutive lanes take consecutive q, so the R butterflies of one
// twiddle share a wavefront and the double-and-add runs on a wave-uniform scalar while R >= 64 (all stages but the last six).
// The first stage (Ns = 1: every twiddle is one) also converts the affine input; the last kernel multiplies by n^-1 and
// returns canonical affine points.  Every exceptional case of the group law (identity inputs, equal or opposite points,
// results equal to the identity) is exact in ec.hpp, so arbitrary inputs give the group element halo2 computes.
#include "common.hpp"
#include "ec.hpp"

using namespace vdb;

namespace {

constexpr unsigned DFT_BLOCK = 128;
constexpr uint32_t MAX_K = 26;

__global__ __launch_bounds__(256) void k_g1_check(const Affine* __restrict__ pts, size_t n, unsigned long long* __restrict__ counters) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Affine p = ld_affine(pts + i);
  bool ok = !u256_geq(p.x, mod_p<Fq>()) && !u256_geq(p.y, mod_p<Fq>());
  if (ok && !affine_is_identity(p))
    ok = u256_eq(fq_sqr(p.y), fq_add(fq_mul(fq_sqr(p.x), p.x), to_mont<Fq>(u256_from_u64(3))));
  if (!ok) {
    atomicAdd(counters, 1ull);
    atomicMin(counters + 1, (unsigned long long)i);
  }
}

// tw[e] = omega^e as a canonical integer (the scalar of a double-and-add), e < m
__global__ __launch_bounds__(256) void k_g1_dft_twiddles(u256 omega, size_t m, u256* __restrict__ tw) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  st256(tw + e, from_mont<Fr>(mont_pow<Fr>(omega, u256_from_u64(e))));
}

// stage Ns = 1 from the affine input: out[2t] = g[t] + g[t + n/2], out[2t + 1] = g[t] - g[t + n/2]
__global__ __launch_bounds__(DFT_BLOCK) void k_g1_dft_first(const Affine* __restrict__ g, uint64_t half, XYZZ* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= half) return;
  const XYZZ a = xyzz_from_affine(ld_affine(g + t));
  const Affine b = ld_affine(g + t + half);
  XYZZ c = a, d = a;
  xyzz_add_mixed(c, b, false);
  xyzz_add_mixed(d, b, true);
  st_xyzz(out + 2 * t, c);
  st_xyzz(out + 2 * t + 1, d);
}

// stage Ns = 2^log_ns, R = 2^log_r = n / (2 Ns)
__global__ __launch_bounds__(DFT_BLOCK) void k_g1_dft_stage(const XYZZ* __restrict__ in, XYZZ* __restrict__ out, const u256* __restrict__ tw, uint64_t half,
                                                            uint32_t log_ns, uint32_t log_r) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= half) return;
  const uint64_t ns = 1ull << log_ns, jmod = t >> log_r, q = t & ((1ull << log_r) - 1);
  const uint64_t j = q * ns + jmod;
  const XYZZ a = ld_xyzz(in + j);
  XYZZ b = ld_xyzz(in + j + half);
  if (jmod) b = xyzz_mul(b, ld256(tw + (jmod << log_r)));
  XYZZ c = a, d = a;
  xyzz_add(c, b);
  xyzz_add(d, xyzz_neg(b));
  const uint64_t dst = (q << (log_ns + 1)) + jmod;
  st_xyzz(out + dst, c);
  st_xyzz(out + dst + ns, d);
}

// out[i] = affine([n^-1] in[i]); n_inv canonical
__global__ __launch_bounds__(DFT_BLOCK) void k_g1_dft_finish(const XYZZ* __restrict__ in, uint64_t n, u256 n_inv, Affine* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st_affine(out + i, xyzz_to_affine(xyzz_mul(ld_xyzz(in + i), n_inv)));
}

// device allocations of one call, released (after the stream has drained) when it returns
struct CallBuffers {
  std::vector<void*> ptrs;
  ~CallBuffers() {
    if (ptrs.empty()) return;
    (void)hipStreamSynchronize(ctx().stream);
    for (void* p : ptrs) (void)hipFree(p);
  }
  void* get(size_t bytes) {
    void* p = nullptr;
    if (timed_malloc(&p, bytes) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return p;
  }
};

// g_to_lagrange on the library stream; g and out may be the same buffer (the input is read by the first launch only)
int lagrange_from_monomial(uint32_t k, const Affine* g, Affine* out) {
  Context& cx = ctx();
  const uint64_t n = 1ull << k, half = n >> 1;
  CallBuffers bufs;
  XYZZ* buf[2] = {(XYZZ*)bufs.get(n * sizeof(XYZZ)), (XYZZ*)bufs.get(n * sizeof(XYZZ))};
  u256* tw = (u256*)bufs.get(half * sizeof(u256));
  if (!buf[0] || !buf[1] || !tw) {
    set_error("g_to_lagrange: out of device memory (2^%u points)", k);
    return VDB_ERR_OOM;
  }
  const u256 omega_inv = mont_inv<Fr>(host_root_of_unity(k));
  const unsigned blocks = (unsigned)((half + DFT_BLOCK - 1) / DFT_BLOCK);
  VDB_LAUNCH(k_g1_dft_twiddles, dim3((unsigned)((half + 255) / 256)), dim3(256), omega_inv, (size_t)half, tw);
  VDB_LAUNCH(k_g1_dft_first, dim3(blocks), dim3(DFT_BLOCK), g, half, buf[0]);
  int cur = 0;
  for (uint32_t s = 1; s < k; s++) {
    VDB_LAUNCH(k_g1_dft_stage, dim3(blocks), dim3(DFT_BLOCK), buf[cur], buf[cur ^ 1], tw, half, s, k - 1 - s);
    cur ^= 1;
  }
  const u256 n_inv = from_mont<Fr>(mont_inv<Fr>(host_fr_from_u64(n)));
  VDB_LAUNCH(k_g1_dft_finish, dim3((unsigned)((n + DFT_BLOCK - 1) / DFT_BLOCK)), dim3(DFT_BLOCK), buf[cur], n, n_inv, out);
  VDB_HIP(hipStreamSynchronize(cx.stream));
  return VDB_OK;
}

}  // namespace

extern "C" {

int vdb_g1_check_dev(const vdb_g1* pts_dev, size_t n, uint64_t* n_bad, uint64_t* first_bad) {
  VDB_REQUIRE_INIT();
  VDB_ARG(n_bad && first_bad, "null pointer");
  *n_bad = 0;
  *first_bad = n;
  if (n == 0) return VDB_OK;
  VDB_ARG(pts_dev, "null pointer");
  Context& cx = ctx();
  CallBuffers bufs;
  unsigned long long* counters = (unsigned long long*)bufs.get(2 * sizeof(unsigned long long));
  if (!counters) return VDB_ERR_OOM;
  VDB_HIP(hipMemsetAsync(counters, 0, sizeof(unsigned long long), cx.stream));
  VDB_HIP(hipMemsetAsync(counters + 1, 0xff, sizeof(unsigned long long), cx.stream));
  VDB_LAUNCH(k_g1_check, dim3((unsigned)((n + 255) / 256)), dim3(256), reinterpret_cast<const Affine*>(pts_dev), n, counters);
  unsigned long long res[2];
  VDB_HIP(hipMemcpyAsync(res, counters, sizeof(res), hipMemcpyDeviceToHost, cx.stream));
  VDB_HIP(hipStreamSynchronize(cx.stream));
  *n_bad = res[0];
  if (res[0]) *first_bad = res[1];
  return VDB_OK;
}

int vdb_g1_lagrange_from_monomial_dev(uint32_t k, const vdb_g1* g_dev, vdb_g1* g_lagrange_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(g_dev && g_lagrange_dev, "null pointer");
  VDB_ARG(k >= 1 && k <= MAX_K, "k must be 1 .. 26");
  return lagrange_from_monomial(k, reinterpret_cast<const Affine*>(g_dev), reinterpret_cast<Affine*>(g_lagrange_dev));
}

int vdb_srs_downsize(uint32_t k, const vdb_g1* g_host, vdb_g1* g_lagrange_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(g_host && g_lagrange_out, "null pointer");
  VDB_ARG(k >= 1 && k <= MAX_K, "k must be 1 .. 26");
  Context& cx = ctx();
  const size_t bytes = ((size_t)1 << k) * sizeof(Affine);
  CallBuffers bufs;
  Affine* d = (Affine*)bufs.get(bytes);
  if (!d) return VDB_ERR_OOM;
  VDB_HIP(hipMemcpyAsync(d, g_host, bytes, hipMemcpyHostToDevice, cx.stream));
  if (int rc = lagrange_from_monomial(k, d, d)) return rc;
  VDB_HIP(hipMemcpyAsync(g_lagrange_out, d, bytes, hipMemcpyDeviceToHost, cx.stream));
  VDB_HIP(hipStreamSynchronize(cx.stream));
  return VDB_OK;
}

}  // extern "C"
