// Witness generation (b5) and fixed-point staging (a2/a3/a18) on gfx950: every kernel that emits cells of a witness stream, with
// its layout and its driver.
//   * fixed-point staging and the FixedPointChip tables (vdb_fp_*, get_fp, witness_release);
//   * the call's context: Streams, set_winv (which publishes g_winv of gadgets.hpp before a call's launches) and make_ctx.  Every
//     kernel of this file may read that context, and only kernels of this file can: the value-only code of the committed tree and
//     index (resident.hip) and the layout stage (layout.hip) do not include gadgets.hpp;
//   * the circuits: distances, FixedPointChip operations, nearest_vector / top-k, kmeans, merkle_commitment, Merkle path updates
//     (with their value pass, which produces the assigned witnesses), Merkle openings, the ANN query and the ANN update;
//   * HostStreams / DevStreams and the vdb_wit_*, vdb_fp_* and vdb_wit_set_window entry points.
//
// Every kernel writes cells of the flat advice stream at statically known offsets (gadgets.hpp), so
// independent gadget instances — distance evaluations, Poseidon permutations, per-dimension folds —
// run as independent threads; long sequential gadgets are cut into position windows, one window per
// wavefront of 64 instances.  The stream is written once (32 B per cell: the HBM-write roofline of
// this stage) and read once by the layout kernel (layout.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ann_update_host.hpp"
#include "common.hpp"
#include "gadgets.hpp"
#include "hostglue.hpp"
#include "poseidon.hpp"
#include "resident.hpp"

namespace vdb {

// ------------------------------------------------------------------ fixed-point staging (host)
// fixed_point.rs:104-119: round(|x| * 2^P) as u128 (saturating), negative -> r - q
static u256 quantize_host(uint32_t P, double x) {
  bool neg = !std::isnan(x) && std::signbit(x);
  double y = std::round(std::fabs(x) * std::ldexp(1.0, (int)P));
  unsigned __int128 q;
  if (std::isnan(y) || y <= 0.0) q = 0;
  else if (y >= 340282366920938463463374607431768211456.0) q = ~(unsigned __int128)0;
  else q = (unsigned __int128)y;
  u256 c = u256_zero();
  for (int i = 0; i < 4; i++) c.w[i] = (uint32_t)(q >> (32 * i));
  u256 m = to_mont<Fr>(c);
  return neg ? fr_neg(m) : m;
}
// fixed_point.rs:121-136 (including the "-(|v| - 2)" quirk for negatives)
static double dequantize_host(uint32_t P, const u256& x) {
  u256 c = from_mont<Fr>(x);
  u256 np, t, one = u256_from_u64(1);
  u256_sub(np, mod_p<Fr>(), u256_shl(one, 2 * P + 1));
  double sign = 1.0;
  if (!u256_geq(np, c)) {  // x > negative_point
    u256 bm;
    u256_sub(bm, mod_p<Fr>(), one);                // bn254_max
    u256 xm = fr_sub(fr_sub(to_mont<Fr>(bm), x), mont_one<Fr>());
    c = from_mont<Fr>(xm);
    sign = -1.0;
  }
  (void)t;
  unsigned __int128 lo = 0;
  for (int i = 0; i < 4; i++) lo |= (unsigned __int128)c.w[i] << (32 * i);
  unsigned __int128 sc = (unsigned __int128)1 << P;
  double xi = (double)(lo / sc);
  double xf = (double)(lo % sc) / (double)sc;
  return sign * (xi + xf);
}

// ------------------------------------------------------------------ FixedPointChip tables
struct FpEntry {
  FpTables host;
  FpTables* dev;
  u256* limb_tab;
};
// cached per device in Context::fp_tables (released by witness_release on vdb_shutdown)
void witness_release(Context& c) {
  for (auto& kv : c.fp_tables) {
    FpEntry* e = static_cast<FpEntry*>(kv.second);
    if (e->limb_tab) (void)hipFree(e->limb_tab);
    if (e->dev) (void)hipFree(e->dev);
    delete e;
  }
  c.fp_tables.clear();
}

__global__ void k_limb_table(u256* tab, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) tab[i] = to_mont<Fr>(u256_from_u64(i));
}

static int get_fp(uint32_t P, uint32_t L, FpEntry** out) {
  if (P < 32 || P > 63) {
    set_error("PRECISION_BITS must be in [32, 63] (fixed_point.rs:55-56)");
    return VDB_ERR_ARG;
  }
  if (L < 2 || L > 20) {
    set_error("lookup_bits must be in [2, 20]");
    return VDB_ERR_ARG;
  }
  uint64_t key = ((uint64_t)P << 32) | L;
  auto& cache = ctx().fp_tables;
  auto it = cache.find(key);
  if (it != cache.end()) {
    *out = static_cast<FpEntry*>(it->second);
    return VDB_OK;
  }
  // owned by the cache from here on, so that an error path below leaks nothing (vdb_shutdown frees what was allocated)
  FpEntry* e = new FpEntry();
  e->dev = nullptr;
  e->limb_tab = nullptr;
  cache[key] = e;
  struct Guard {
    std::map<uint64_t, void*>& cache;
    uint64_t key;
    FpEntry* e;
    bool keep = false;
    ~Guard() {
      if (keep) return;
      if (e->limb_tab) (void)hipFree(e->limb_tab);
      if (e->dev) (void)hipFree(e->dev);
      cache.erase(key);
      delete e;
    }
  } guard{cache, key, e};
  FpTables& T = e->host;
  memset(&T, 0, sizeof(T));
  T.P = P;
  T.L = L;
  T.one = mont_one<Fr>();
  T.pow2[0] = T.one;
  for (int i = 1; i < 254; i++) T.pow2[i] = fr_add(T.pow2[i - 1], T.pow2[i - 1]);
  T.scale = T.pow2[P];
  static const double exp2c[13] = {3.6240421303547230336183979205877e-11, 4.1284327467833130245549169910389e-10,
                                   0.0000000071086385644026346316624185550542, 0.00000010172297085296590958930245291448,
                                   0.0000013215904023658396206789543841996, 0.000015252713316417140696221389106544,
                                   0.00015403531076657894204857389177279, 0.0013333558131297097698435464957392,
                                   0.0096181291078409107025643582456283, 0.055504108664804181586140094858174,
                                   0.24022650695910142332414229540187, 0.69314718055994529934452147700678, 1.0};
  static const double logc[15] = {-3.319586265362338e-08, 1.4957235315170112e-06, -3.1350053389526744e-05,
                                  0.00040554177582512901, -0.0036218342998850703, 0.023663846121538389,
                                  -0.11691877183255484, 0.44524062371564499, -1.3195777548208449,
                                  3.0518128028712077, -5.4904626000399528, 7.6298580090181591,
                                  -8.1653313719804235, 7.1389971101896279, -3.1937385492842112};
  for (int i = 0; i < 13; i++) T.exp2_poly[i] = quantize_host(P, exp2c[i]);
  for (int i = 0; i < 15; i++) T.log_poly[i] = quantize_host(P, logc[i]);
  T.c_half = quantize_host(P, 0.5);
  T.c_ln2 = quantize_host(P, 0.693147180559945309417232121458176568);
  T.c_log2e = quantize_host(P, 1.44269504088896340735992468100189214);
  T.c_one_q = quantize_host(P, 1.0);
  // generate_sin_poly (fixed_point.rs:189-211: "lolremez -d 14 -r 0:pi sin(x)", highest power first) and the constants of qsin, qcos, qsinh
  static const double sinc[15] = {-1.1008071636607462e-11, 2.4208013888629323e-10, -3.8584805817996712e-10, -2.3786993104309845e-08,
                                  -2.9795813710683115e-09, 2.7608543130047009e-06, -6.4467066994122565e-09, -0.00019840680551418068,
                                  -3.839555844512214e-09, 0.0083333350601673614, -5.0943769725466814e-10, -0.16666666657583049,
                                  -8.5029878414113731e-12, 1.0000000000003146, -1.9323057584419828e-15};
  for (int i = 0; i < 15; i++) T.sin_poly[i] = quantize_host(P, sinc[i]);
  const double pi = 3.14159265358979323846264338327950288;
  T.c_pi = quantize_host(P, pi);
  T.c_two_pi = quantize_host(P, pi * 2.0);
  T.c_half_pi = quantize_host(P, 1.57079632679489661923132169163975144);
  T.c_two = quantize_host(P, 2.0);
  for (uint32_t i = 0; i < 260; i++) {
    T.small[i] = host_fr_from_u64(i);
    T.small_inv[i] = i ? mont_inv<Fr>(T.small[i]) : u256_zero();
  }
  compute_sizes(T);
  VDB_HIP(hipMalloc(&e->limb_tab, ((size_t)1 << L) * sizeof(u256)));
  VDB_LAUNCH(k_limb_table, dim3((unsigned)(((1u << L) + 255) / 256)), dim3(256), e->limb_tab, 1u << L);
  T.limb_tab = e->limb_tab;
  VDB_HIP(hipMalloc(&e->dev, sizeof(FpTables)));
  VDB_HIP(hipMemcpyAsync(e->dev, &T, sizeof(FpTables), hipMemcpyHostToDevice, ctx().stream));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  guard.keep = true;
  *out = e;
  return VDB_OK;
}

// ------------------------------------------------------------------ distance layout
enum { M_EUCLID = 0, M_COSINE = 1, M_MANHATTAN = 2, M_HAMMING = 3 };
struct DistLayout {
  uint32_t metric, D;
  uint64_t head_cells, head_lk, tail_cells, tail_lk, total_cells, total_lk;
};
static int dist_layout(const FpTables& T, int metric, size_t D, DistLayout* o) {
  const Sizes& z = T.sz;
  o->metric = (uint32_t)metric;
  o->D = (uint32_t)D;
  uint64_t ip_c = 4 + D * ((uint64_t)z.qmul[0] + 4), ip_l = D * (uint64_t)z.qmul[1];
  switch (metric) {
    case M_EUCLID:
      o->head_cells = 4 * D + ip_c;
      o->head_lk = ip_l;
      o->tail_cells = z.qsqrt[0];
      o->tail_lk = z.qsqrt[1];
      break;
    case M_COSINE:
      o->head_cells = 3 * ip_c;
      o->head_lk = 3 * ip_l;
      o->tail_cells = 2ull * z.qsqrt[0] + z.qmul[0] + z.qdiv[0] + 1 + 4;
      o->tail_lk = 2ull * z.qsqrt[1] + z.qmul[1] + z.qdiv[1];
      break;
    case M_MANHATTAN:
      o->head_cells = 4 * D + D * (uint64_t)z.qabs[0] + (D == 0 ? 0 : (D == 1 ? 1 : 1 + 3 * (D - 1)));
      o->head_lk = D * (uint64_t)z.qabs[1];
      o->tail_cells = 0;
      o->tail_lk = 0;
      break;
    case M_HAMMING:  // distance.rs:146-175: is_equal per element (sub + is_zero), gate().sum, two load_witness, qdiv, load_constant, qsub
      o->head_cells = 12 * D + (D == 0 ? 0 : (D == 1 ? 1 : 1 + 3 * (D - 1)));
      o->head_lk = 0;
      o->tail_cells = 2ull + z.qdiv[0] + 1 + 4;
      o->tail_lk = z.qdiv[1];
      break;
    default:
      set_error("unsupported metric %d (0 euclidean, 1 cosine, 2 manhattan, 3 hamming)", metric);
      return VDB_ERR_ARG;
  }
  o->total_cells = o->head_cells + o->tail_cells;
  o->total_lk = o->head_lk + o->tail_lk;
  return VDB_OK;
}

// where instance t lives in the streams and which operand vectors it uses
struct InstMap {
  uint64_t adv_base, lk_base;
  uint32_t grp;                       // instances per group
  uint64_t grp_adv_stride, grp_lk_stride;
  uint32_t a_mod, b_div;              // a = A[(t % a_mod)], b = B[(t / b_div)]
  __device__ __forceinline__ uint64_t adv(uint32_t t, const DistLayout& dl) const { return adv_base + (uint64_t)(t / grp) * grp_adv_stride + (uint64_t)(t % grp) * dl.total_cells; }
  __device__ __forceinline__ uint64_t lk(uint32_t t, const DistLayout& dl) const { return lk_base + (uint64_t)(t / grp) * grp_lk_stride + (uint64_t)(t % grp) * dl.total_lk; }
};

struct Streams {
  u256* adv;
  uint8_t* sel;
  u256* lk;
  int* err;
  // deferred-inversion list (see WCtx)
  uint64_t* inv_pos;
  u256* inv_val;
  uint32_t* inv_cnt;
  uint32_t inv_cap;
  // rank window in the coordinates of adv / lk (see WCtx); full range by default
  uint64_t rlo, rhi, rllo, rlhi;
  __device__ __forceinline__ bool touches(uint64_t a0, uint64_t a1, uint64_t l0, uint64_t l1) const {
    return (a0 < rhi && a1 > rlo) || (l0 < rlhi && l1 > rllo && l1 > l0);
  }
};

// (the streams, the rank window, the tables and the inversion list are not part of the context: they are the call's g_winv, set_winv)
__device__ __forceinline__ WCtx make_ctx(const Streams&, const FpTables*, uint64_t pos, uint64_t lpos) {
  WCtx c;
  c.pos = pos;
  c.lpos = lpos;
  c.lo = 0;
  c.hi = ~0ull;
  c.count_only = false;
  c.err = 0;
  return c;
}
// every host entry publishes its call's invariant context before it launches a kernel (stream ordered: kernels of an earlier call
// still read the earlier one)
static int set_winv(const Streams& st, const FpTables* T) {
  // (the source outlives the call: a pageable source is staged before hipMemcpyToSymbolAsync returns on this runtime, as the other
  //  small uploads of this file rely on too; the ring only makes that assumption harmless should a runtime ever defer the read)
  static thread_local WInv ring[8];
  static thread_local unsigned slot = 0;
  WInv& h = ring[slot++ & 7u];
  h = WInv{};
  h.adv = st.adv;
  h.sel = st.sel;
  h.lk = st.lk;
  h.rlo = st.rlo;
  h.rhi = st.rhi;
  h.rllo = st.rllo;
  h.rlhi = st.rlhi;
  h.T = T;
  h.inv_pos = st.inv_pos;
  h.inv_val = st.inv_val;
  h.inv_cnt = st.inv_cnt;
  h.inv_cap = st.inv_cap;
  VDB_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_winv), &h, sizeof(WInv), 0, hipMemcpyHostToDevice, ctx().stream));
  return VDB_OK;
}

#define HEAD_TB 128
// inner_product(a, b) of fixed_point.rs:854-874 for one instance, cooperatively by the block:
// thread i emits qmul(a_i, b_i) and the following qadd; running sums come from an LDS prefix.
// mode 0: operands x_i = A[i], y_i = B[i];  mode 1: x_i = y_i = A[i] - B[i] (already emitted qsub)
__device__ void block_inner_product(const Streams& st, const FpTables* T, const u256* A, const u256* Bv, int mode, uint32_t D,
                                    uint64_t ipbase, uint64_t iplbase, u256* sh /* HEAD_TB + 1 */, u256* result) {
  const uint32_t tid = threadIdx.x;
  const uint32_t qm = T->sz.qmul[0], qml = T->sz.qmul[1];
  if (tid == 0) {
    WCtx c = make_ctx(st, T, ipbase, iplbase);
    Gadgets g(c);
    g.g_add(u256_zero(), u256_zero());  // res = qadd(0, 0)
    sh[HEAD_TB] = u256_zero();
  }
  __syncthreads();
  for (uint32_t c0 = 0; c0 < D; c0 += HEAD_TB) {
    uint32_t i = c0 + tid;
    u256 q = u256_zero();
    WCtx c = make_ctx(st, T, ipbase + 4 + (uint64_t)i * (qm + 4), iplbase + (uint64_t)i * qml);
    Gadgets g(c);
    if (i < D) {
      u256 x = A[i], y = Bv[i];
      if (mode == 1) {
        x = fr_sub(x, y);
        y = x;
      }
      q = g.fp_qmul(x, y);
      if (c.err) atomicOr(st.err, c.err);
    }
    sh[tid] = q;
    __syncthreads();
    if (i < D) {
      u256 prev = sh[HEAD_TB];
      for (uint32_t j = 0; j < tid; j++) prev = fr_add(prev, sh[j]);
      g.g_add(prev, q);  // res = qadd(res, a_i b_i)
    }
    __syncthreads();
    if (tid == 0) {
      u256 carry = sh[HEAD_TB];
      uint32_t lim = D - c0 < HEAD_TB ? D - c0 : HEAD_TB;
      for (uint32_t j = 0; j < lim; j++) carry = fr_add(carry, sh[j]);
      sh[HEAD_TB] = carry;
    }
    __syncthreads();
  }
  if (tid == 0) *result = sh[HEAD_TB];
  __syncthreads();
}

// head of a distance: everything before the sequential tail.  One block per instance.
__global__ __launch_bounds__(HEAD_TB) void k_dist_head(Streams st, const FpTables* __restrict__ T, DistLayout dl, InstMap im,
                                                       const u256* __restrict__ A, const u256* __restrict__ Bv, u256* __restrict__ mid /* 3 per inst */,
                                                       u256* __restrict__ result, int have_values) {
  __shared__ u256 sh[HEAD_TB + 1];
  const uint32_t t = blockIdx.x, tid = threadIdx.x, D = dl.D;
  const u256* a = A + (size_t)(t % im.a_mod) * D;
  const u256* b = Bv + (size_t)(t / im.b_div) * D;
  const uint64_t base = im.adv(t, dl), lbase = im.lk(t, dl);
  // sharded run: k_dist_values has left this instance's sums in `mid` already, so a block none of whose cells lie in the rank's
  // window has nothing to do (without it every rank walked every instance's head in value-only mode)
  if (have_values && !st.touches(base, base + dl.head_cells, lbase, lbase + dl.head_lk)) return;
  if (dl.metric == M_EUCLID) {  // distance.rs:97-119
    for (uint32_t i = tid; i < D; i += HEAD_TB) {
      WCtx c = make_ctx(st, T, base + 4ull * i, lbase);
      Gadgets g(c);
      g.g_sub(a[i], b[i]);
    }
    block_inner_product(st, T, a, b, 1, D, base + 4ull * D, lbase, sh, &mid[3 * (size_t)t]);
  } else if (dl.metric == M_COSINE) {  // distance.rs:121-144
    const uint64_t ipc = 4 + (uint64_t)D * (T->sz.qmul[0] + 4), ipl = (uint64_t)D * T->sz.qmul[1];
    block_inner_product(st, T, a, b, 0, D, base, lbase, sh, &mid[3 * (size_t)t]);
    block_inner_product(st, T, a, a, 0, D, base + ipc, lbase + ipl, sh, &mid[3 * (size_t)t + 1]);
    block_inner_product(st, T, b, b, 0, D, base + 2 * ipc, lbase + 2 * ipl, sh, &mid[3 * (size_t)t + 2]);
  } else {  // manhattan, distance.rs:177-195; hamming, distance.rs:146-175: one value per element, then gate().sum over them
    const bool ham = dl.metric == M_HAMMING;
    const uint32_t qa = T->sz.qabs[0], qal = T->sz.qabs[1];
    const uint64_t sumbase = ham ? base + 12ull * D : base + 4ull * D + (uint64_t)D * qa;
    if (tid == 0) sh[HEAD_TB] = u256_zero();
    __syncthreads();
    for (uint32_t c0 = 0; c0 < D; c0 += HEAD_TB) {
      uint32_t i = c0 + tid;
      u256 v = u256_zero();
      if (i < D) {
        if (ham) {  // gate().is_equal(a_i, b_i): [a - b, b, 1, a] then is_zero's eight cells
          WCtx c = make_ctx(st, T, base + 12ull * i, lbase);
          Gadgets g(c);
          v = g.g_is_equal(a[i], b[i]);
        } else {
          WCtx c = make_ctx(st, T, base + 4ull * i, lbase);
          Gadgets g(c);
          u256 d = g.g_sub(a[i], b[i]);
          c.pos = base + 4ull * D + (uint64_t)i * qa;
          c.lpos = lbase + (uint64_t)i * qal;
          v = g.fp_qabs(d);
        }
      }
      sh[tid] = v;
      __syncthreads();
      if (i < D) {  // gate().sum: [a0, a1, 1, s1, a2, 1, s2, ...]
        WCtx c = make_ctx(st, T, 0, 0);
        if (i == 0) {
          c.pos = sumbase;
          c.push(v, D > 1);
        } else {
          u256 s = sh[HEAD_TB];
          for (uint32_t j = 0; j <= tid; j++) s = fr_add(s, sh[j]);
          c.pos = sumbase + 1 + 3ull * (i - 1);
          c.push(v, false);
          c.push(mont_one<Fr>(), false, true);
          c.push(s, i + 1 < D);
        }
      }
      __syncthreads();
      if (tid == 0) {
        u256 carry = sh[HEAD_TB];
        uint32_t lim = D - c0 < HEAD_TB ? D - c0 : HEAD_TB;
        for (uint32_t j = 0; j < lim; j++) carry = fr_add(carry, sh[j]);
        sh[HEAD_TB] = carry;
      }
      __syncthreads();
    }
    if (tid == 0) {
      if (ham)
        mid[3 * (size_t)t] = sh[HEAD_TB];   // the number of equal elements: the tail quantizes it
      else
        result[t] = sh[HEAD_TB];
    }
  }
}

// sequential tail of a distance, cut into `gridDim.y` position windows; lanes = instances
__global__ __launch_bounds__(64) void k_dist_tail(Streams st, const FpTables* __restrict__ T, DistLayout dl, InstMap im, uint32_t n_inst,
                                                  const u256* __restrict__ mid, u256* __restrict__ result, int have_values) {
  uint32_t t = blockIdx.x * 64 + threadIdx.x;
  const bool live = t < n_inst;
  if (!live) t = n_inst - 1;
  const uint32_t S = gridDim.y, s = blockIdx.y;
  const uint64_t tb = im.adv(t, dl) + dl.head_cells, tlb = im.lk(t, dl) + dl.head_lk;
  // segment S-1 carries the result every rank needs; the other segments only emit cells and leave at once
  // when none of the wavefront's instances lies in this rank's window
  // (`have_values`: k_dist_tail_values has computed every result already — the last segment leaves like the others)
  if ((s != S - 1 || have_values) && !__any((int)(live && st.touches(tb, tb + dl.tail_cells, tlb, tlb + dl.tail_lk)))) return;
  WCtx c = make_ctx(st, T, tb, tlb);
  c.lo = tb + dl.tail_cells * s / S;
  c.hi = tb + dl.tail_cells * (s + 1) / S;
  if (!live) c.lo = c.hi = tb;  // padding lanes follow the same control flow but store nothing
  Gadgets g(c);
  u256 r;
  if (dl.metric == M_EUCLID) {
    r = g.fp_qsqrt(mid[3 * (size_t)t]);
  } else if (dl.metric == M_HAMMING) {
    // len = load_witness(quantization(D)), ab_sum_q = load_witness(quantization(the count as f64)): both exact (an integer times 2^P),
    // neither constrained by the reference (distance.rs:165-169); 1 - ab_sum_q / len
    const u256 len = fr_mul(to_mont<Fr>(u256_from_u64(dl.D)), T->scale);
    const u256 sq = fr_mul(mid[3 * (size_t)t], T->scale);
    c.push(len, false);
    c.push(sq, false);
    u256 sim = g.fp_qdiv(sq, len);
    u256 one = g.load_constant(T->c_one_q);
    r = g.g_sub(one, sim);
  } else {
    u256 ab = mid[3 * (size_t)t], aa = mid[3 * (size_t)t + 1], bb = mid[3 * (size_t)t + 2];
    u256 as = g.fp_qsqrt(aa);
    u256 bs = g.fp_qsqrt(bb);
    u256 den = g.fp_qmul(as, bs);
    u256 sim = g.fp_qdiv(ab, den);
    u256 one = g.load_constant(T->c_one_q);
    r = g.g_sub(one, sim);
  }
  if (live && s == S - 1) {
    result[t] = r;
    if (c.err) atomicOr(st.err, c.err);
  }
}

// ---- the distances' VALUES alone, for sharded runs (every rank needs every distance — assignments and centroids follow
// from them — but stores only the cells of its own columns).  One wavefront per instance: lane i takes dimensions i, i + 64, ...
// through the gadgets' value-only helpers, the sums are folded across the wavefront (field addition: the order is free), lane 0
// writes what the head would have left in `mid` (Manhattan: the result itself).  No emission context, no stores of cells.
__device__ __forceinline__ u256 wave_sum_fr(u256 v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    u256 o;
#pragma unroll
    for (int k = 0; k < 8; k++) o.w[k] = __shfl_xor(v.w[k], off, 64);
    v = fr_add(v, o);
  }
  return v;
}
__device__ __forceinline__ u256 wave_shfl_up(const u256& v, int off) {
  u256 o;
#pragma unroll
  for (int k = 0; k < 8; k++) o.w[k] = __shfl_up(v.w[k], off, 64);
  return o;
}
__device__ __forceinline__ u256 wave_bcast(const u256& v, int lane) {
  u256 o;
#pragma unroll
  for (int k = 0; k < 8; k++) o.w[k] = __shfl(v.w[k], lane, 64);
  return o;
}
__global__ __launch_bounds__(64) void k_dist_values(const FpTables* __restrict__ T, DistLayout dl, InstMap im, const u256* __restrict__ A,
                                                    const u256* __restrict__ Bv, u256* __restrict__ mid, u256* __restrict__ result) {
  const uint32_t t = blockIdx.x, lane = threadIdx.x, D = dl.D;
  const u256* a = A + (size_t)(t % im.a_mod) * D;
  const u256* b = Bv + (size_t)(t / im.b_div) * D;
  WCtx c{};
  Gadgets g(c);
  u256 s0 = u256_zero(), s1 = u256_zero(), s2 = u256_zero();
  for (uint32_t i = lane; i < D; i += 64) {
    const u256 x = a[i], y = b[i];
    if (dl.metric == M_EUCLID) {
      const u256 d = fr_sub(x, y);
      s0 = fr_add(s0, g.v_qmul(d, d));
    } else if (dl.metric == M_COSINE) {
      s0 = fr_add(s0, g.v_qmul(x, y));
      s1 = fr_add(s1, g.v_qmul(x, x));
      s2 = fr_add(s2, g.v_qmul(y, y));
    } else if (dl.metric == M_HAMMING) {
      if (u256_eq(x, y)) s0 = fr_add(s0, mont_one<Fr>());
    } else {
      s0 = fr_add(s0, g.v_qabs(fr_sub(x, y)));
    }
  }
  s0 = wave_sum_fr(s0);
  if (dl.metric == M_COSINE) {
    s1 = wave_sum_fr(s1);
    s2 = wave_sum_fr(s2);
  }
  if (lane == 0) {
    if (dl.metric == M_MANHATTAN) {
      result[t] = s0;
    } else {
      mid[3 * (size_t)t] = s0;
      if (dl.metric == M_COSINE) {
        mid[3 * (size_t)t + 1] = s1;
        mid[3 * (size_t)t + 2] = s2;
      }
    }
  }
}
// ... and the sequential tails' values: lanes = instances, the tail's own code with an emission window that holds no position
// (every sub-gadget takes its value-only path; domain errors — a division by zero — are reported as the emitting walk reports them)
__global__ __launch_bounds__(64) void k_dist_tail_values(Streams st, const FpTables* __restrict__ T, DistLayout dl, uint32_t n_inst,
                                                         const u256* __restrict__ mid, u256* __restrict__ result) {
  uint32_t t = blockIdx.x * 64 + threadIdx.x;
  const bool live = t < n_inst;
  if (!live) t = n_inst - 1;
  WCtx c = make_ctx(st, T, 1, 0);
  c.lo = c.hi = 0;
  Gadgets g(c);
  u256 r;
  if (dl.metric == M_EUCLID) {
    r = g.fp_qsqrt(mid[3 * (size_t)t]);
  } else if (dl.metric == M_HAMMING) {
    // len = load_witness(quantization(D)), ab_sum_q = load_witness(quantization(the count as f64)): both exact (an integer times 2^P),
    // neither constrained by the reference (distance.rs:165-169); 1 - ab_sum_q / len
    const u256 len = fr_mul(to_mont<Fr>(u256_from_u64(dl.D)), T->scale);
    const u256 sq = fr_mul(mid[3 * (size_t)t], T->scale);
    c.push(len, false);
    c.push(sq, false);
    u256 sim = g.fp_qdiv(sq, len);
    u256 one = g.load_constant(T->c_one_q);
    r = g.g_sub(one, sim);
  } else {
    u256 ab = mid[3 * (size_t)t], aa = mid[3 * (size_t)t + 1], bb = mid[3 * (size_t)t + 2];
    u256 as = g.fp_qsqrt(aa);
    u256 bs = g.fp_qsqrt(bb);
    u256 den = g.fp_qmul(as, bs);
    u256 sim = g.fp_qdiv(ab, den);
    u256 one = g.load_constant(T->c_one_q);
    r = g.g_sub(one, sim);
  }
  if (live) {
    result[t] = r;
    if (c.err) atomicOr(st.err, c.err);
  }
}

// Batched evaluation of the deferred inverse cells: Montgomery's trick over runs of 16 entries
#define INVFIX_CH 16
__global__ __launch_bounds__(64) void k_inv_fixup(u256* __restrict__ adv, const uint64_t* __restrict__ pos, const u256* __restrict__ val,
                                                  const uint32_t* __restrict__ cnt, uint32_t cap) {
  const uint32_t n = *cnt < cap ? *cnt : cap;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; (uint64_t)t * INVFIX_CH < n; t += stride) {
    const uint32_t lo = t * INVFIX_CH, hi = lo + INVFIX_CH < n ? lo + INVFIX_CH : n;
    u256 pre[INVFIX_CH];
    u256 acc = mont_one<Fr>();
    for (uint32_t i = lo; i < hi; i++) {
      pre[i - lo] = acc;
      acc = fr_mul(acc, val[i]);  // entries are non-zero by construction
    }
    acc = mont_inv<Fr>(acc);
    for (uint32_t i = hi; i-- > lo;) {
      adv[pos[i]] = fr_mul(acc, pre[i - lo]);
      acc = fr_mul(acc, val[i]);
    }
  }
}
// attaches the context-owned deferred-inversion list to `st` and resets its counter
static int inv_list_attach(Streams& st, uint64_t cells) {
  uint64_t cap = cells / 16 + 4096;
  if (cap > (16u << 20)) cap = 16u << 20;
  uint8_t* buf = (uint8_t*)scratch_get(4, cap * (sizeof(u256) + sizeof(uint64_t)) + 64);
  if (!buf) return VDB_ERR_OOM;
  st.inv_cnt = (uint32_t*)buf;
  st.inv_val = (u256*)(buf + 64);
  st.inv_pos = (uint64_t*)(buf + 64 + cap * sizeof(u256));
  st.inv_cap = (uint32_t)cap;
  VDB_HIP(hipMemsetAsync(st.inv_cnt, 0, sizeof(uint32_t), ctx().stream));
  return VDB_OK;
}
static int inv_list_fixup(const Streams& st) {
  if (!st.inv_cnt) return VDB_OK;
  VDB_LAUNCH(k_inv_fixup, dim3((unsigned)(ctx().cu_count * 8)), dim3(64), st.adv, st.inv_pos, st.inv_val, st.inv_cnt, st.inv_cap);
  return VDB_OK;
}

static uint32_t tail_segments(uint32_t n_inst) {
  uint32_t groups = (n_inst + 63) / 64;
  uint32_t s = 4096 / (groups ? groups : 1);
  if (s < 1) s = 1;
  if (s > 64) s = 64;
  return s;
}

// runs head + tail for n_inst instances; distances land in `result` (device)
static int run_distances(const Streams& st, FpEntry* fp, const DistLayout& dl, const InstMap& im, uint32_t n_inst, const u256* A,
                         const u256* Bv, u256* mid, u256* result) {
  if (n_inst == 0) return VDB_OK;
  // a rank that stores only a window of the streams first computes every distance's value with the value-only kernels; the emitting
  // kernels then leave at once wherever none of their cells lie in the window (with selectors requested, every rank runs every head and
  // the last tail segment in value-only mode instead)
  const bool windowed = !(st.rlo == 0 && st.rhi == ~0ull && st.rllo == 0 && st.rlhi == ~0ull);
  const int have_values = (windowed && st.sel == nullptr) ? 1 : 0;
  if (have_values) {
    VDB_LAUNCH(k_dist_values, dim3(n_inst), dim3(64), fp->dev, dl, im, A, Bv, mid, result);
    if (dl.tail_cells) VDB_LAUNCH(k_dist_tail_values, dim3((n_inst + 63) / 64), dim3(64), st, fp->dev, dl, n_inst, mid, result);
  }
  VDB_LAUNCH(k_dist_head, dim3(n_inst), dim3(HEAD_TB), st, fp->dev, dl, im, A, Bv, mid, result, have_values);
  if (dl.tail_cells)
    VDB_LAUNCH(k_dist_tail, dim3((n_inst + 63) / 64, tail_segments(n_inst)), dim3(64), st, fp->dev, dl, im, n_inst, mid, result, have_values);
  return VDB_OK;
}

// ------------------------------------------------------------------ nearest_vector (vectordb.rs:122-163): the t nearest vectors of
// every one of Q queries over one database, the queries' blocks end to end in the stream.  t = 1 is nearest_vector itself, once per query
// (no select(M, ..) is emitted); Q = t = 1 is the reference's single call.
// Per query: the n distances, then t rounds of [n - 1 qmin | n is_equal | D select_by_indicator | n select(Constant(M), cur_i, ind_i)],
// the last round without its select(M, ..) blocks.  M = 2^(2P) - 1 takes a round's winners out of the next round's minimum.  Round r of
// query q keeps its prefix minima at [(q * t + r) * n, + n) of `pm`; `rnd[q * n + i]` is the first round whose mask replaced entry i
// (NV_UNMASKED: none), so that the entry a round works on is cur_r,i = rnd < r ? M : d_i.
constexpr uint32_t NV_UNMASKED = 0xffffffffu;
struct NvMap {
  uint64_t adv0, lk0;          // first cell / lookup cell of query 0's block
  uint64_t per_q, per_q_l;     // cells / lookup cells of one query's block
  uint64_t rounds_off, rounds_loff, per_r, per_r_l;   // where round 0 starts inside a block; cells / lookup cells of a round that masks
  uint64_t iseq_off, sel_off, mask_off;               // where the stages after the qmin chain start inside a round
  uint32_t Q, n, D, t;
};
__device__ __forceinline__ u256 nv_mask_value(const FpTables* T) { return fr_sub(T->pow2[2 * T->P], mont_one<Fr>()); }
// qmin(m, x) as a value (vectordb.rs:141-145 folds it over the distances): is_neg(m - x) ? m : x
__device__ __forceinline__ u256 nv_vmin(const Gadgets& g, const u256& m, const u256& x) {
  return g.v_is_neg(from_mont<Fr>(fr_sub(m, x))) ? m : x;
}
__device__ __forceinline__ u256 nv_cur(const u256* __restrict__ dq, const uint32_t* __restrict__ rq, uint32_t i, uint32_t r, const u256& M) {
  return rq[i] < r ? M : dq[i];
}
// All t rounds of a query's values, one wavefront per query.  Per round: the prefix minima of the qmin chain over the entries the
// earlier rounds left — an inclusive scan over 64 entries at a time, the running minimum carried from tile to tile — the round's
// minimum to every lane, and the entries whose bits equal it marked as masked from the next round on.  Over values the range checks
// admit, v_is_neg(m - x) is a total order and the scan IS the serial fold (ties: equal values, equal bits).  Over anything else (field
// elements no fixed-point value quantizes to) the relation need not be transitive, so every lane checks the fold's own recurrence
// pm[i] == qmin(pm[i - 1], cur_i) on what the scan produced — which, with pm[0] == cur_0, characterises the serial walk — and a round
// that fails it is walked serially by lane 0.  Lanes past the end of a tile hold M: a live lane only ever reads lower lanes, and the
// carry is taken from a full tile.
__global__ __launch_bounds__(64) void k_nv_rounds(const FpTables* __restrict__ T, const u256* __restrict__ d, uint32_t n, uint32_t t,
                                                   u256* __restrict__ pm, uint32_t* __restrict__ rnd) {
  const uint32_t q = blockIdx.x, lane = threadIdx.x;
  const u256* dq = d + (size_t)q * n;
  uint32_t* rq = rnd + (size_t)q * n;
  WCtx c{};
  Gadgets g(c);
  const u256 M = nv_mask_value(T);
  for (uint32_t i = lane; i < n; i += 64) rq[i] = NV_UNMASKED;
  for (uint32_t r = 0; r < t; r++) {
    u256* pq = pm + ((size_t)q * t + r) * n;
    u256 carry = u256_zero();
    bool ok = true;
    for (uint32_t c0 = 0; c0 < n; c0 += 64) {
      const uint32_t i = c0 + lane;
      const bool live = i < n;
      const u256 x = live ? nv_cur(dq, rq, i, r, M) : M;
      u256 v = x;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const u256 o = wave_shfl_up(v, off);
        if ((int)lane >= off) v = nv_vmin(g, o, v);
      }
      if (c0) v = nv_vmin(g, carry, v);
      u256 prev = wave_shfl_up(v, 1);
      if (lane == 0) prev = carry;
      if (live) {
        ok = ok && u256_eq(v, i == 0 ? x : nv_vmin(g, prev, x));
        pq[i] = v;
      }
      carry = wave_bcast(v, n - c0 < 64 ? (int)(n - c0 - 1) : 63);
    }
    u256 m = carry;
    if (!__all((int)ok)) {
      if (lane == 0) {
        m = nv_cur(dq, rq, 0, r, M);
        pq[0] = m;
        for (uint32_t i = 1; i < n; i++) {
          m = nv_vmin(g, m, nv_cur(dq, rq, i, r, M));
          pq[i] = m;
        }
      }
      m = wave_bcast(m, 0);
    }
    if (r + 1 < t) {
      for (uint32_t i = lane; i < n; i += 64)
        if (rq[i] == NV_UNMASKED && u256_eq(dq[i], m)) rq[i] = r;
      __threadfence_block();   // lane 0's serial walk of a later round reads what the other lanes marked
      __syncthreads();
    }
  }
}
// The minimum of a query's n distances and the LAST entry that holds it, as values alone (vdb_nearest_values_dev), one wavefront per
// query.  `a before b` is qmin's own test, v_is_neg(a - b): the signed fixed-point order, not the order of the 256 raw bits (a negative
// value is a field element near the modulus).  A lane folds entries lane, lane + 64, ... in rising order and moves to a later entry
// unless its own comes strictly before it, so a tie leaves the later index; the 64 (value, index) pairs then meet in a butterfly that
// keeps the earlier value and, between two values neither of which comes before the other, the larger index — both partners of an
// exchange decide alike.  Lanes past the end start from entry 0, a real entry with the lowest index: it can never displace a winner.
// Over values the range checks admit this is the serial fold's minimum (see k_nv_rounds on what lies outside them), and the index is
// the last set indicator of nearest_vector's is_equal(min, d_i).
__global__ __launch_bounds__(64) void k_nv_argmin(const u256* __restrict__ d, uint32_t n, uint32_t* __restrict__ idx_out, u256* __restrict__ dist_out) {
  const uint32_t q = blockIdx.x, lane = threadIdx.x;
  const u256* dq = d + (size_t)q * n;
  WCtx c{};
  Gadgets g(c);
  uint32_t bi = lane < n ? lane : 0;
  u256 best = dq[bi];
  for (uint32_t i = lane + 64; i < n; i += 64) {
    const u256 x = dq[i];
    if (!g.v_is_neg(from_mont<Fr>(fr_sub(best, x)))) {
      best = x;
      bi = i;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    u256 o;
#pragma unroll
    for (int k = 0; k < 8; k++) o.w[k] = __shfl_xor(best.w[k], off, 64);
    const uint32_t oi = __shfl_xor(bi, off, 64);
    const bool o_first = g.v_is_neg(from_mont<Fr>(fr_sub(o, best))), b_first = g.v_is_neg(from_mont<Fr>(fr_sub(best, o)));
    if (o_first || (!b_first && oi > bi)) {
      best = o;
      bi = oi;
    }
  }
  if (lane == 0) {
    idx_out[q] = bi;
    if (dist_out) dist_out[q] = best;
  }
}
// The winner of every round of k_nv_rounds as a value (vdb_nearest_topk_values_dev), one wavefront per (query, round): the LAST entry the
// round works on whose bits equal the round's minimum pm[.. n - 1] — the last set indicator of the round's is_equal(min, cur_i), which
// is what its select_by_indicator states.  The round's entries are read through nv_cur, so the last round needs no mark of its own.
// A lane keeps the last hit of its stride (rising i), a butterfly of maxima joins the 64; every round has a hit (the minimum is one of
// its entries), a round with nothing left unmasked works on M everywhere and states n - 1.  No LDS, no scratch.
__global__ __launch_bounds__(64) void k_nv_round_winners(const FpTables* __restrict__ T, const u256* __restrict__ d, const u256* __restrict__ pm,
                                                          const uint32_t* __restrict__ rnd, uint32_t n, uint32_t t, uint32_t* __restrict__ idx_out,
                                                          u256* __restrict__ dist_out) {
  const uint32_t qr = blockIdx.x, q = qr / t, r = qr % t, lane = threadIdx.x;
  const u256* dq = d + (size_t)q * n;
  const uint32_t* rq = rnd + (size_t)q * n;
  const u256 M = nv_mask_value(T), m = pm[(size_t)qr * n + n - 1];
  int best = -1;
  for (uint32_t i = lane; i < n; i += 64)
    if (u256_eq(nv_cur(dq, rq, i, r, M), m)) best = (int)i;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int o = __shfl_xor(best, off, 64);
    best = o > best ? o : best;
  }
  if (lane == 0) {
    idx_out[qr] = (uint32_t)best;
    if (dist_out) dist_out[qr] = m;
  }
}
// lanes = (query, round, link of the round's chain): qmin(pm[i - 1], cur_i), i = 1 .. n - 1
__global__ __launch_bounds__(64) void k_nv_qmin(Streams st, const FpTables* __restrict__ T, NvMap nm, const u256* __restrict__ d,
                                                 const u256* __restrict__ pm, const uint32_t* __restrict__ rnd) {
  const uint64_t th = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  const uint32_t links = nm.n - 1;
  if (th >= (uint64_t)nm.Q * nm.t * links) return;
  const uint32_t i = (uint32_t)(th % links) + 1, r = (uint32_t)((th / links) % nm.t), q = (uint32_t)(th / ((uint64_t)links * nm.t));
  WCtx c = make_ctx(st, T, nm.adv0 + q * nm.per_q + nm.rounds_off + r * nm.per_r + (uint64_t)(i - 1) * T->sz.qmin[0],
                    nm.lk0 + q * nm.per_q_l + nm.rounds_loff + r * nm.per_r_l + (uint64_t)(i - 1) * T->sz.qmin[1]);
  Gadgets g(c);
  const u256 M = nv_mask_value(T);
  g.fp_qmin(pm[((size_t)q * nm.t + r) * nm.n + i - 1], nv_cur(d + (size_t)q * nm.n, rnd + (size_t)q * nm.n, i, r, M));
}
// lanes = (query, round, vector): is_equal(min_r, cur_i)
__global__ __launch_bounds__(64) void k_nv_is_equal(Streams st, const FpTables* __restrict__ T, NvMap nm, const u256* __restrict__ d,
                                                     const u256* __restrict__ pm, const uint32_t* __restrict__ rnd, u256* __restrict__ ind) {
  const uint64_t th = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (th >= (uint64_t)nm.Q * nm.t * nm.n) return;
  const uint32_t i = (uint32_t)(th % nm.n), r = (uint32_t)((th / nm.n) % nm.t), q = (uint32_t)(th / ((uint64_t)nm.n * nm.t));
  WCtx c = make_ctx(st, T, nm.adv0 + q * nm.per_q + nm.rounds_off + r * nm.per_r + nm.iseq_off + 12ull * i, 0);
  Gadgets g(c);
  const u256 M = nv_mask_value(T);
  ind[th] = g.g_is_equal(pm[((size_t)q * nm.t + r) * nm.n + nm.n - 1], nv_cur(d + (size_t)q * nm.n, rnd + (size_t)q * nm.n, i, r, M));
}
// lanes = (query, round before the last, vector): select(Constant(M), cur_i, ind_i), the entry the next round works on
__global__ __launch_bounds__(64) void k_nv_mask(Streams st, const FpTables* __restrict__ T, NvMap nm, const u256* __restrict__ d,
                                                 const uint32_t* __restrict__ rnd, const u256* __restrict__ ind) {
  const uint64_t th = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  const uint32_t masking = nm.t - 1;
  if (th >= (uint64_t)nm.Q * masking * nm.n) return;
  const uint32_t i = (uint32_t)(th % nm.n), r = (uint32_t)((th / nm.n) % masking), q = (uint32_t)(th / ((uint64_t)nm.n * masking));
  WCtx c = make_ctx(st, T, nm.adv0 + q * nm.per_q + nm.rounds_off + r * nm.per_r + nm.mask_off + 8ull * i, 0);
  Gadgets g(c);
  const u256 M = nv_mask_value(T);
  g.g_select(M, nv_cur(d + (size_t)q * nm.n, rnd + (size_t)q * nm.n, i, r, M), ind[((size_t)q * nm.t + r) * nm.n + i]);
}
// select_by_indicator per (query, round, dimension): [0, a0, ind0, s0, a1, ind1, s1, ...], the walk over the n vectors cut into `S`
// segments: lanes = (query, round, segment, dimension), the dimension fastest so that a wavefront reads consecutive elements of one
// vector.  The running value at a segment's start is the element of the last vector before it whose indicator is set (0 when there is
// none), found by walking the indicators backwards.
__global__ __launch_bounds__(64) void k_nv_select(Streams st, const FpTables* __restrict__ T, NvMap nm, uint32_t S, const u256* __restrict__ vectors,
                                                   const u256* __restrict__ ind, u256* __restrict__ result) {
  const uint64_t th = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  const uint32_t n = nm.n, D = nm.D;
  if (th >= (uint64_t)nm.Q * nm.t * S * D) return;
  const uint32_t j = (uint32_t)(th % D), sg = (uint32_t)((th / D) % S), qr = (uint32_t)(th / ((uint64_t)D * S));
  const uint32_t q = qr / nm.t, r = qr % nm.t;
  const uint32_t i0 = (uint32_t)((uint64_t)n * sg / S), i1 = (uint32_t)((uint64_t)n * (sg + 1) / S);
  const u256* indq = ind + (size_t)qr * n;
  const uint64_t base = nm.adv0 + q * nm.per_q + nm.rounds_off + r * nm.per_r + nm.sel_off + (uint64_t)j * (1 + 3ull * n);
  u256 s = u256_zero();
  for (uint32_t i = i0; i-- > 0;) {
    if (!u256_is_zero(indq[i])) {
      s = vectors[(size_t)i * D + j];
      break;
    }
  }
  WCtx c = make_ctx(st, T, base + (i0 ? 1 + 3ull * i0 : 0), 0);
  if (i0 == 0) c.push(s, n > 0);
  for (uint32_t i = i0; i < i1; i++) {
    u256 a = vectors[(size_t)i * D + j], in = indq[i];
    if (!u256_is_zero(in)) s = a;
    c.push(a, false);
    c.push(in, false);
    c.push(s, i + 1 < n);
  }
  if (sg == S - 1) result[(size_t)qr * D + j] = s;
}

// ------------------------------------------------------------------ kmeans (vectordb.rs:225-362)
struct KmLayout {
  uint32_t N, D, K;
  uint64_t per_vec, per_vec_l, assign, assign_l, sizes, per_cluster, per_cluster_l, iter, iter_l;
};
__global__ __launch_bounds__(64) void k_km_assign(Streams st, const FpTables* __restrict__ T, KmLayout kl, DistLayout dl, uint64_t ibase, uint64_t ilbase,
                                                  const u256* __restrict__ dist, u256* __restrict__ ind) {
  // lanes = vectors, blockIdx.y = position window of the per-vector assignment block
  uint32_t v = blockIdx.x * 64 + threadIdx.x;
  const bool live = v < kl.N;
  if (!live) v = kl.N - 1;
  const uint32_t K = kl.K, S = gridDim.y, s = blockIdx.y;
  const uint64_t base = ibase + (uint64_t)v * kl.per_vec + (uint64_t)K * dl.total_cells;
  const uint64_t cells = (uint64_t)(K - 1) * T->sz.qmin[0] + 20ull * K;
  const uint64_t lbase_v = ilbase + (uint64_t)v * kl.per_vec_l + (uint64_t)K * dl.total_lk;
  if (s != S - 1 && !__any((int)(live && st.touches(base, base + cells, lbase_v, lbase_v + (uint64_t)(K - 1) * T->sz.qmin[1])))) return;
  WCtx c = make_ctx(st, T, base, lbase_v);
  c.lo = base + cells * s / S;
  c.hi = base + cells * (s + 1) / S;
  if (!live) c.lo = c.hi = base;
  Gadgets g(c);
  const u256* d = dist + (size_t)v * K;
  u256 m = d[0];
  for (uint32_t k = 1; k < K; k++) m = g.fp_qmin(m, d[k]);
  for (uint32_t k = 0; k < K; k++) {
    u256 eq = g.g_is_equal(m, d[k]);
    u256 r = g.g_select(T->c_one_q, u256_zero(), eq);
    if (live && s == S - 1) ind[(size_t)v * K + k] = r;
  }
}
#define KM_PF 8
// One wavefront folds one chain s_v = s_{v-1} + x_v (s_0 = x_0) and emits the qadd cells of steps v = 1 .. N-1 at
// base + (v - 1) * stride: ORDER 0 = [s_{v-1}, x_v, 1, s_v], ORDER 1 = [x_v, s_{v-1}, 1, s_v].  The chain is
// sequential in the reference; here lane l owns the contiguous steps [l * per, (l + 1) * per): lane totals (loads
// only), a wavefront scan, then every lane emits its steps from its own prefix.  Loads always run ahead of the stores
// of a chunk (a load issued after stores waits for their acknowledgement), and lanes whose cells lie outside the
// rank window skip the emission altogether.  Returns the chain total (all lanes).
template <int ORDER, class LoadFn>
__device__ __forceinline__ u256 chain_fold_wave(WCtx& c, uint64_t base, uint64_t stride, uint32_t N, LoadFn&& x) {
  const uint32_t lane = threadIdx.x & 63, per = (N + 63) / 64;
  const uint32_t lo = lane * per < N ? lane * per : N, hi = lo + per < N ? lo + per : N;
  u256 tot = u256_zero();
  for (uint32_t v0 = lo; v0 < hi; v0 += KM_PF) {
    u256 xv[KM_PF];
#pragma unroll
    for (uint32_t q = 0; q < KM_PF; q++) xv[q] = x(v0 + q < hi ? v0 + q : hi - 1);
#pragma unroll
    for (uint32_t q = 0; q < KM_PF; q++)
      if (v0 + q < hi) tot = fr_add(tot, xv[q]);
  }
  u256 inc = tot;  // inclusive scan over lanes
  for (int o = 1; o < 64; o <<= 1) {
    u256 t = wave_shfl_up(inc, o);
    if ((int)lane >= o) inc = fr_add(inc, t);
  }
  const u256 total = wave_bcast(inc, 63);
  u256 run = fr_sub(inc, tot);  // exclusive prefix = s_{lo-1}
  // the lane's cells: steps max(lo, 1) .. hi-1
  const uint32_t first = lo ? lo : 1;
  if (first >= hi) return total;
  const uint64_t c_lo = base + (uint64_t)(first - 1) * stride, c_hi = base + (uint64_t)(hi - 2) * stride + 4;
  if (!c.count_only && (c_hi <= winv().rlo || c_lo >= winv().rhi)) return total;
  for (uint32_t v0 = lo; v0 < hi; v0 += KM_PF) {
    u256 xv[KM_PF];
#pragma unroll
    for (uint32_t q = 0; q < KM_PF; q++) xv[q] = x(v0 + q < hi ? v0 + q : hi - 1);
#pragma unroll
    for (uint32_t q = 0; q < KM_PF; q++) {
      const uint32_t v = v0 + q;
      if (v < hi) {
        const u256 nx = fr_add(run, xv[q]);
        if (v >= 1) {
          c.pos = base + (uint64_t)(v - 1) * stride;
          c.push(ORDER == 0 ? run : xv[q], true);
          c.push(ORDER == 0 ? xv[q] : run, false);
          c.push(mont_one<Fr>(), false, true);
          c.push(nx, false);
        }
        run = nx;
      }
    }
  }
  return total;
}
// cluster sizes: sizes_k = sum_v indicator[v][k] as a chain of qadd cells (vectordb.rs:316-322); one wavefront per cluster
__global__ __launch_bounds__(64) void k_km_sizes(Streams st, const FpTables* __restrict__ T, KmLayout kl, uint64_t base, const u256* __restrict__ ind,
                                                 u256* __restrict__ sizes) {
  const uint32_t k = blockIdx.x;
  WCtx c = make_ctx(st, T, 0, 0);
  const u256 tot = chain_fold_wave<0>(c, base + 4ull * k, 4ull * kl.K, kl.N, [&](uint32_t v) { return ind[(size_t)v * kl.K + k]; });
  if (threadIdx.x == 0) sizes[k] = tot;
}
// filtered vectors: select(0, vector_j, is_zero(indicator)) per (cluster, vector, dimension); a thread owns KM_PF dimensions
__global__ __launch_bounds__(64) void k_km_filter(Streams st, const FpTables* __restrict__ T, KmLayout kl, uint64_t cbase0, const u256* __restrict__ vectors,
                                                  const u256* __restrict__ ind, u256 scale_inv, u256* __restrict__ filt) {
  const uint32_t JC = (kl.D + KM_PF - 1) / KM_PF;
  const uint64_t id = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (id >= (uint64_t)kl.K * kl.N * JC) return;
  const uint32_t jc = (uint32_t)(id % JC), v = (uint32_t)((id / JC) % kl.N), k = (uint32_t)(id / ((uint64_t)JC * kl.N));
  const uint32_t j0 = jc * KM_PF;
  const u256 sel = ind[(size_t)v * kl.K + k];
  u256 x[KM_PF];
#pragma unroll
  for (uint32_t q = 0; q < KM_PF; q++) x[q] = vectors[(size_t)v * kl.D + (j0 + q < kl.D ? j0 + q : kl.D - 1)];
  const uint64_t cb = cbase0 + (uint64_t)k * kl.per_cluster + (uint64_t)v * (8 + 8ull * kl.D);
  WCtx c = make_ctx(st, T, cb, 0);
  Gadgets g(c);
  u256 iz;
  if (jc == 0) iz = g.g_is_zero_inv(sel, u256_is_zero(sel) ? mont_one<Fr>() : scale_inv);
  else iz = u256_is_zero(sel) ? mont_one<Fr>() : u256_zero();
  c.pos = cb + 8 + 8ull * j0;
#pragma unroll
  for (uint32_t q = 0; q < KM_PF; q++)
    if (j0 + q < kl.D) filt[((size_t)k * kl.N + v) * kl.D + j0 + q] = g.g_select(u256_zero(), x[q], iz);
}
// per-cluster, per-dimension sums of the filtered vectors (vectordb.rs:338-347): one wavefront per (cluster, dimension)
__global__ __launch_bounds__(64) void k_km_sum(Streams st, const FpTables* __restrict__ T, KmLayout kl, uint64_t cbase0, const u256* __restrict__ filt,
                                               u256* __restrict__ sums) {
  const uint32_t id = blockIdx.x, k = id / kl.D, j = id % kl.D;
  WCtx c = make_ctx(st, T, 0, 0);
  const uint64_t base = cbase0 + (uint64_t)k * kl.per_cluster + (uint64_t)kl.N * (8 + 8ull * kl.D) + 4ull * j;
  const u256 tot = chain_fold_wave<1>(c, base, 4ull * kl.D, kl.N, [&](uint32_t v) { return filt[((size_t)k * kl.N + v) * kl.D + j]; });
  if (threadIdx.x == 0) sums[id] = tot;
}
// One lane's qdiv(a(), b()) at (base, lbase), its cell range cut into gridDim.y slices (blockIdx.y's is emitted); every slice but the last
// leaves at once where no lane of the wavefront touches the rank window.  The last slice hands the quotient to done(r) and reports err.
// A lane past the end (`live` false) runs a real lane's operands with an empty window.  The body of k_km_div and k_annm_div.
template <class A, class B, class Done>
__device__ __forceinline__ void qdiv_sliced(const Streams& st, const FpTables* __restrict__ T, uint64_t base, uint64_t lbase, bool live, A&& a, B&& b,
                                            Done&& done) {
  const uint32_t S = gridDim.y, s = blockIdx.y;
  if (s != S - 1 && !__any((int)(live && st.touches(base, base + T->sz.qdiv[0], lbase, lbase + T->sz.qdiv[1])))) return;
  WCtx c = make_ctx(st, T, base, lbase);
  c.lo = base + (uint64_t)T->sz.qdiv[0] * s / S;
  c.hi = base + (uint64_t)T->sz.qdiv[0] * (s + 1) / S;
  if (!live) c.lo = c.hi = base;
  Gadgets g(c);
  u256 r = g.fp_qdiv(a(), b());
  if (live && s == S - 1) {
    done(r);
    if (c.err) atomicOr(st.err, c.err);
  }
}
__global__ __launch_bounds__(64) void k_km_div(Streams st, const FpTables* __restrict__ T, KmLayout kl, uint64_t cbase0, uint64_t clbase0,
                                               const u256* __restrict__ sums, const u256* __restrict__ sizes, u256* __restrict__ cent) {
  uint32_t id = blockIdx.x * 64 + threadIdx.x;
  const bool live = id < kl.K * kl.D;
  if (!live) id = kl.K * kl.D - 1;
  uint32_t k = id / kl.D, j = id % kl.D;
  const uint64_t base = cbase0 + (uint64_t)k * kl.per_cluster + (uint64_t)kl.N * (8 + 8ull * kl.D) + (uint64_t)(kl.N - 1) * kl.D * 4 + (uint64_t)j * T->sz.qdiv[0];
  const uint64_t lbase = clbase0 + (uint64_t)k * kl.per_cluster_l + (uint64_t)j * T->sz.qdiv[1];
  qdiv_sliced(st, T, base, lbase, live, [&] { return sums[id]; }, [&] { return sizes[k]; }, [&](const u256& r) { cent[id] = r; });
}
// The mean audit's block M (include/vdb.h vdb_wit_ann_mean), addressed without an indicator or a filter: one wavefront per word j folds
// s_ij = member_i[j] + s_{i-1,j} over the n_c members, the qadd cells [x_ij, s_{i-1,j}, 1, s_ij] at chain + 4 ((i - 1) dim + j)
// (k_km_sum's order and stride); then per word qdiv(s_j, len) at div + j qdiv[0], and mean_ok[j]: the quotient's bits are own_j's.
__global__ __launch_bounds__(64) void k_annm_sum(Streams st, const FpTables* __restrict__ T, uint64_t chain, uint32_t n_c, uint32_t dim,
                                                 const u256* __restrict__ members, u256* __restrict__ sums) {
  const uint32_t j = blockIdx.x;
  WCtx c = make_ctx(st, T, 0, 0);
  const u256 tot = chain_fold_wave<1>(c, chain + 4ull * j, 4ull * dim, n_c, [&](uint32_t v) { return members[(size_t)v * dim + j]; });
  if (threadIdx.x == 0) sums[j] = tot;
}
__global__ __launch_bounds__(64) void k_annm_div(Streams st, const FpTables* __restrict__ T, uint64_t div, uint32_t dim, const u256* __restrict__ sums,
                                                 u256 len, const u256* __restrict__ own, uint8_t* __restrict__ mean_ok) {
  uint32_t j = blockIdx.x * 64 + threadIdx.x;
  const bool live = j < dim;
  if (!live) j = dim - 1;
  qdiv_sliced(st, T, div + (uint64_t)j * T->sz.qdiv[0], (uint64_t)j * T->sz.qdiv[1], live, [&] { return sums[j]; }, [&] { return len; },
              [&](const u256& r) { mean_ok[j] = u256_eq(r, own[j]) ? 1 : 0; });
}
// k_annm_div's sibling of the recentre (include/vdb.h vdb_wit_ann_recentre): the same cells, and the quotient itself kept as a value in
// mean[j] — the new centroid's word j, which the update block of the centroids' tree absorbs — where the audit compares it with own_j
__global__ __launch_bounds__(64) void k_annr_div(Streams st, const FpTables* __restrict__ T, uint64_t div, uint32_t dim, const u256* __restrict__ sums,
                                                 u256 len, u256* __restrict__ mean) {
  uint32_t j = blockIdx.x * 64 + threadIdx.x;
  const bool live = j < dim;
  if (!live) j = dim - 1;
  qdiv_sliced(st, T, div + (uint64_t)j * T->sz.qdiv[0], (uint64_t)j * T->sz.qdiv[1], live, [&] { return sums[j]; }, [&] { return len; },
              [&](const u256& r) { mean[j] = r; });
}
// The means of all K clusters of a resident index as values alone (include/vdb.h vdb_ann_cluster_means_dev): per cluster k and word j
// qdiv(sum_i member_i[j], quantization(n_k)), the k-means tail's arithmetic with no filter in front.  fr_add is exact and associative, so
// the serial walk gives the bits of the circuit's qadd chain; the quotient is the value form fp_qdiv takes under an empty window.  Grid
// (ceil(dim / 64), K), one wavefront per block: lane l owns word 64 blockIdx.x + l, a member row is read as one contiguous run, KM_PF
// loads are issued ahead of their adds as in chain_fold_wave.  The host has checked the offsets (rising, the last one the row count).
__global__ __launch_bounds__(64) void k_ann_means(const u256* __restrict__ grouped, const uint64_t* __restrict__ offsets, uint32_t dim, int* __restrict__ err,
                                                  u256* __restrict__ means) {
  const uint32_t k = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
  if (j >= dim) return;
  const uint64_t lo = offsets[k], hi = offsets[k + 1];
  u256 tot = u256_zero();
  for (uint64_t v0 = lo; v0 < hi; v0 += KM_PF) {
    u256 xv[KM_PF];
#pragma unroll
    for (uint32_t q = 0; q < KM_PF; q++) xv[q] = grouped[(size_t)(v0 + q < hi ? v0 + q : hi - 1) * dim + j];
#pragma unroll
    for (uint32_t q = 0; q < KM_PF; q++)
      if (v0 + q < hi) tot = fr_add(tot, xv[q]);
  }
  WCtx c{};
  Gadgets g(c);
  const u256 len = fr_mul(to_mont<Fr>(u256_from_u64(hi - lo)), g.T.scale);   // quantization(n_k) = n_k 2^P
  int e = 0;
  means[(size_t)k * dim + j] = g.v_qdiv(tot, len, e);
  if (e) atomicOr(err, e);
}
__global__ void k_push_cells(Streams st, uint64_t pos, u256 a, u256 b, uint32_t n) {
  if (blockIdx.x || threadIdx.x || n == 0) return;
  // load_constant / load_zero cells: data-independent; stored by the rank whose window holds them, like every other cell
  if (pos >= st.rlo && pos < st.rhi) {
    st.adv[pos] = a;
    if (st.sel) st.sel[pos] = 2;
  }
  if (n > 1 && pos + 1 >= st.rlo && pos + 1 < st.rhi) {
    st.adv[pos + 1] = b;
    if (st.sel) st.sel[pos + 1] = 2;
  }
}

// ------------------------------------------------------------------ Poseidon trace (merkle_commitment)
// cells of PoseidonChip::permutation (halo2-lib community-edition poseidon chip, [UPSTREAM-RECALL])
// GateChip::sum; cmask bit i set = v[i] is a Constant cell
__device__ u256 trace_sum(WCtx& c, const FpTables* T, const u256* v, int n, unsigned cmask) {
  u256 s = v[0];
  c.push(v[0], n > 1, cmask & 1u);
  for (int i = 1; i < n; i++) {
    s = fr_add(s, v[i]);
    c.push(v[i], false, (cmask >> i) & 1u);
    c.push(mont_one<Fr>(), false, true);
    c.push(s, i + 1 < n);
  }
  return s;
}
template <class A>   // inner_product(a, constants), operand i = a(i)
__device__ __forceinline__ u256 trace_ip_const_of(WCtx& c, A&& a, const u256* row, int n) {
  u256 s;
  int i0, ng;
  if (u256_eq(row[0], mont_one<Fr>())) {
    s = a(0);
    i0 = 1;
    ng = n - 1;
    c.push(s, ng > 0);
  } else {
    s = u256_zero();
    i0 = 0;
    ng = n;
    c.push(u256_zero(), ng > 0, true);
  }
  int gi = 1;
  for (int i = i0; i < n; i++, gi++) {
    const u256 ai = a(i);
    s = fr_add(s, fr_mul(ai, row[i]));
    c.push(ai, false);
    c.push(row[i], false, true);  // Constant(matrix entry)
    c.push(s, gi < ng);
  }
  return s;
}
__device__ u256 trace_ip_const(WCtx& c, const FpTables* T, const u256* a, const u256* row, int n) {
  return trace_ip_const_of(c, [a](int i) { return a[i]; }, row, n);
}
__device__ void trace_sbox(Gadgets& g, u256& x, const u256& cst) {
  u256 x2 = g.g_mul(x, x);
  u256 x4 = g.g_mul(x2, x2);
  u256 o = fr_add(fr_mul(x, x4), cst);  // mul_add(x, x4, Constant(c)): [c, x, x4, out]
  g.c.push(cst, true, true); g.c.push(x, false); g.c.push(x4, false); g.c.push(o, false);
  x = o;
}
__device__ void trace_dense(WCtx& c, const FpTables* T, u256 st[PSD_T], const u256 m[PSD_T][PSD_T]) {
  u256 r[PSD_T];
  for (int i = 0; i < PSD_T; i++) r[i] = trace_ip_const(c, T, st, m[i], PSD_T);
  for (int i = 0; i < PSD_T; i++) st[i] = r[i];
}
// (the context by value and back: ten dwords in registers — by reference it lived in the caller's scratch and was re-read around
//  every cell store, which on gfx9 waits for the stores before it)
__device__ __noinline__ WCtx trace_permutation(WCtx c, const FpTables* T, const PoseidonSpec* __restrict__ sp, u256 st[PSD_T], const u256* in, int n_in) {
  Gadgets g(c);
  {
    u256 v[2] = {st[0], sp->start[0][0]};
    st[0] = trace_sum(c, T, v, 2, 2u);
  }
  for (int i = 0; i < n_in; i++) {
    u256 v[3] = {st[1 + i], in[i], sp->start[0][1 + i]};
    st[1 + i] = trace_sum(c, T, v, 3, 4u);
  }
  for (int i = n_in + 1, k = 0; i < PSD_T; i++, k++) {
    u256 cst = sp->start[0][i];
    if (k == 0) cst = fr_add(cst, mont_one<Fr>());
    u256 v[2] = {st[i], cst};
    st[i] = trace_sum(c, T, v, 2, 2u);
  }
  for (int r = 1; r < PSD_HALF; r++) {
    for (int i = 0; i < PSD_T; i++) trace_sbox(g, st[i], sp->start[r][i]);
    trace_dense(c, T, st, sp->mds);
  }
  for (int i = 0; i < PSD_T; i++) trace_sbox(g, st[i], sp->start[PSD_HALF][i]);
  trace_dense(c, T, st, sp->pre_sparse);
  for (int p = 0; p < PSD_RP; p++) {
    trace_sbox(g, st[0], sp->partial[p]);
    u256 r[PSD_T];
    r[0] = trace_ip_const(c, T, st, sp->sparse_row[p], PSD_T);
    for (int i = 1; i < PSD_T; i++) {  // mul_add(s0, Constant(e), s_i): [s_i, s0, e, out]
      r[i] = fr_add(fr_mul(st[0], sp->sparse_col[p][i - 1]), st[i]);
      c.push(st[i], true); c.push(st[0], false); c.push(sp->sparse_col[p][i - 1], false, true); c.push(r[i], false);
    }
    for (int i = 0; i < PSD_T; i++) st[i] = r[i];
  }
  for (int r = 0; r < PSD_HALF - 1; r++) {
    for (int i = 0; i < PSD_T; i++) trace_sbox(g, st[i], sp->end[r][i]);
    trace_dense(c, T, st, sp->mds);
  }
  u256 z = u256_zero();
  for (int i = 0; i < PSD_T; i++) trace_sbox(g, st[i], z);
  trace_dense(c, T, st, sp->mds);
  return c;
}
HD constexpr uint32_t perm_cells(int n_in) { return (n_in == 2 ? 18u : (n_in == 1 ? 15u : 12u)) + 2238u; }
// a tree node's hash: the permutation absorbing [left, right], then the padding-only one.  A level of a Merkle path: [assert_bit 4 |
// select 8 | select 8 | node] for the first running digest, [select 8 | select 8 | node] for a second one (the updates' new path)
constexpr uint32_t NODE_CELLS = perm_cells(2) + perm_cells(0), PATH_HEAD_CELLS = 4 + 2 * 8, PATH_TAIL_CELLS = 2 * 8;
HD constexpr uint64_t path_level_cells(int sides) { return PATH_HEAD_CELLS + NODE_CELLS + (uint64_t)(sides - 1) * (PATH_TAIL_CELLS + NODE_CELLS); }
// One permutation of the node hash H(left, right) whose cells start at p0: the absorbing one, or (`second`) the padding-only one behind
// it, which starts from the state its lane recomputes.  A rank that holds a block of columns emits only the permutations whose cells
// fall into its stretch of the stream.
__device__ __forceinline__ void trace_node_half(const Streams& stq, const FpTables* T, const PoseidonSpec* __restrict__ sp, uint64_t p0,
                                                const u256* left, const u256* right, uint32_t second) {
  if (second) p0 += perm_cells(2);
  if (!stq.touches(p0, p0 + (second ? perm_cells(0) : perm_cells(2)), 0, 0)) return;
  u256 st[PSD_T] = {sp->cap, u256_zero(), u256_zero()};
  u256 in[PSD_RATE] = {*left, *right};
  if (second) psd_permute_absorb(sp, st, in, 2);   // the padding-only permutation starts where the absorbing one ended
  WCtx c = make_ctx(stq, T, p0, 0);
  c = trace_permutation(c, T, sp, st, in, second ? 0 : 2);
}
// One part of the level of a Merkle path whose cells start at lb, for SIDES running digests (*cur0, and *cur1 of the updates' new path)
// against one sibling: part 0 = the bit and every side's two selects, part 1 + 2 * side + second = one permutation of that side's hash
template <int SIDES>
__device__ __forceinline__ void trace_path_level(const Streams& stq, const FpTables* T, const PoseidonSpec* __restrict__ sp, uint64_t lb, uint32_t bit,
                                                 const u256* psib, const u256* cur0, const u256* cur1, uint32_t part) {
  constexpr uint64_t tail_at = PATH_HEAD_CELLS + NODE_CELLS;
  if (part == 0) {
    if (!stq.touches(lb, lb + PATH_HEAD_CELLS, 0, 0) && !(SIDES == 2 && stq.touches(lb + tail_at, lb + tail_at + PATH_TAIL_CELLS, 0, 0))) return;
    const u256 b = bit ? mont_one<Fr>() : u256_zero();
    const u256 sib = *psib;
    WCtx c = make_ctx(stq, T, lb, 0);
    Gadgets g(c);
    g.g_assert_bit(b);
    for (int side = 0; side < SIDES; side++) {
      const u256 cur = *(side ? cur1 : cur0);
      g.g_select(sib, cur, b);
      g.g_select(cur, sib, b);
      c.pos = lb + tail_at;
    }
    return;
  }
  const uint32_t side = SIDES == 2 ? (part - 1) >> 1 : 0, second = (part - 1) & 1u;
  const u256* pcur = side ? cur1 : cur0;
  trace_node_half(stq, T, sp, lb + (side ? tail_at + PATH_TAIL_CELLS : PATH_HEAD_CELLS), bit ? psib : pcur, bit ? pcur : psib, second);
}
// idx = gate.inner_product(bits of `slot`, Constant(2^l)), l < depth, traced from c on
__device__ u256 trace_path_index(WCtx& c, const FpTables* T, uint32_t slot, uint32_t depth) {
  return trace_ip_const_of(c, [slot](int l) { return ((slot >> l) & 1u) ? mont_one<Fr>() : u256_zero(); }, T->pow2, (int)depth);
}

// one thread per leaf permutation: the trace cells; leaf v's sponge starts at base + v * leaf_cells, or at base + starts[v] where given
__global__ __launch_bounds__(64) void k_mk_leaf_trace(Streams stq, const FpTables* __restrict__ T, const PoseidonSpec* __restrict__ sp,
                                                      const u256* __restrict__ vectors, uint32_t n, uint32_t D, uint32_t nperm, uint64_t base,
                                                      uint64_t leaf_cells, const u256* __restrict__ states, const uint64_t* __restrict__ starts) {
  uint32_t id = blockIdx.x * 64 + threadIdx.x;
  if (id >= n * nperm) return;
  uint32_t v = id / nperm, p = id % nperm;
  const uint32_t off = 2 * p;
  const int cnt = leaf_absorbs(D, p);
  // permutations 0..p-1 of a leaf are full (2 inputs) except possibly the one before the padding-only one
  uint64_t pos = base + (starts ? starts[v] : (uint64_t)v * leaf_cells);
  for (uint32_t q = 0; q < p; q++) pos += perm_cells(leaf_absorbs(D, q));
  // a rank that holds a block of columns emits only the permutations whose cells fall into its stretch of the stream
  // (the sponge states they start from were computed by k_mk_leaf_states)
  if (!stq.touches(pos, pos + perm_cells(cnt), 0, 0)) return;
  WCtx c = make_ctx(stq, T, pos, 0);
  u256 st[PSD_T];
  for (int i = 0; i < PSD_T; i++) st[i] = states[((size_t)v * nperm + p) * PSD_T + i];
  const u256* msg = vectors + (size_t)v * D;
  u256 in[PSD_RATE] = {cnt > 0 ? msg[off] : u256_zero(), cnt > 1 ? msg[off + 1] : u256_zero()};
  c = trace_permutation(c, T, sp, st, in, cnt);
}
// The tree without a launch per level's TRACE: the digests of every level first (value only: two permutations of latency per level,
// k_mk_level_values of resident.hip), then every node's two permutations traced in ONE launch — a thread per (node, permutation), the padding-only
// permutation starting from the state its thread recomputes.  (One thread per node tracing 4.5 k cells level after level cost ten
// launches of 2.1 ms each whatever the level's size: 21 of C3's 49 ms of witness.)
// levels: level 0 = the lp (padded) leaf digests, level l at offset lp (2 - 2^(1-l)) ... i.e. one after the other; node g of the
// tree (level-major numbering, g < lp - 1) has its cells at base + g * NODE_CELLS
__global__ __launch_bounds__(64) void k_mk_tree_trace(Streams stq, const FpTables* __restrict__ T, const PoseidonSpec* __restrict__ sp,
                                                      const u256* __restrict__ levels, uint32_t lp, uint64_t base) {
  const uint32_t id = blockIdx.x * 64 + threadIdx.x;
  const uint32_t g = id >> 1, j = id & 1u;
  if (g + 1 >= lp) return;
  // level of node g: level sizes lp/2, lp/4, ...; in_off = offset of the level it reads in `levels`
  uint32_t sz = lp >> 1, first = 0, in_off = 0, in_sz = lp;
  while (g >= first + sz) {
    first += sz;
    in_off += in_sz;
    in_sz = sz;
    sz >>= 1;
  }
  const u256* in = levels + in_off + 2 * (g - first);
  trace_node_half(stq, T, sp, base + (uint64_t)g * NODE_CELLS, in, in + 1, j);
}

// ------------------------------------------------------------------ Merkle path updates (include/vdb.h vdb_wit_merkle_update)
// A batch of m updates (idx_j, new vector_j) against the resident tree `levels` (k_mk_tree_trace's layout), applied in order.  Stream:
// [new vectors | old leaves | bits | siblings] (the assigned witnesses), then per update its leaf sponge, per level
// [assert_bit | select lo | select ro | H(lo, ro) | select ln | select rn | H(ln, rn)], and the index inner product.
// Values: the m leaf hashes (k_mk_leaf_states), then level after level (k_mku_level, a thread per (update, old / new path)).  Which
// earlier update of the batch last touched a node depends on the indices alone, so one kernel (k_mku_touchers) answers it for every
// (update, level) before any hash is known: a backward scan over the batch's indices held in LDS.
// An update is a write or a delete (kinds): a delete's new leaf is one load_constant(0) cell in place of the sponge, so the blocks of
// a batch differ in size and the kernels take where update j's levels start from an array (level_at, host prefix sums).  The tree may
// have been doubled `grow` times before the batch (vdb_merkle_tree_grow_dev): then the assigned witnesses end with R_0, the root before
// the growth, and a growth block follows them: [Z_0 = load_constant(0) | Z_{l+1} = H(Z_l, Z_l), l < depth - 1 | R_{i+1} = H(R_i, Z_{d+i}),
// i < grow] (k_mku_grow_trace), d the depth before the growth.  A plain batch is all writes and grow = 0.
// what the stream of a path circuit is made of, for updates and reads alike (path_layout): the leaf sponge, a level, the index
struct PathLayout {
  uint32_t D, depth, nperm;
  uint64_t leaf_cells, level_cells, ip_cells;
};
struct MkuLayout : PathLayout {
  uint32_t m, w, d0, grow;  // w: the writes among the m updates; depth = d0 + grow
  uint64_t n_vec, n_wit, n_in, grow_cells, total;  // n_in = n_vec + n_wit (+ 1: R_0 when grow)
};
// per (level, update), arrays indexed [l * m + j]: sib_from = the latest earlier update whose path holds this one's sibling node at
// level l (-1: the resident digest is still current), last = no later update touches this update's node at level l (its new-path
// digest is the batch's final state of that node); prev_same[j] = the latest earlier update of the same slot (-1: none).
// write_no[j]: which of the new vectors update j writes, -1 for a delete, whose new leaf 0 goes into row 0 of path_new here, and
// -2 - s for a carried leaf (the index delete's move, mku_plan): the digest slot s of `levels` holds before the batch
__global__ __launch_bounds__(256) void k_mku_touchers(const uint32_t* __restrict__ idx, uint32_t m, uint32_t depth, int32_t* __restrict__ sib_from,
                                                      int32_t* __restrict__ prev_same, uint8_t* __restrict__ last, const int32_t* __restrict__ write_no,
                                                      const u256* __restrict__ levels, u256* __restrict__ path_new) {
  __shared__ uint32_t sidx[MKU_MAX_UPDATES];
  for (uint32_t i = threadIdx.x; i < m; i += 256) sidx[i] = idx[i];
  __syncthreads();
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= m * depth) return;
  const uint32_t j = t % m, l = t / m;
  const uint32_t node = sidx[j] >> l;
  int32_t from = -1;
  for (int32_t i = (int32_t)j - 1; i >= 0; i--)
    if ((sidx[i] >> l) == (node ^ 1u)) {
      from = i;
      break;
    }
  sib_from[t] = from;
  if (l == 0) {
    int32_t same = -1;
    for (int32_t i = (int32_t)j - 1; i >= 0; i--)
      if (sidx[i] == node) {
        same = i;
        break;
      }
    prev_same[j] = same;
    const int32_t wn = write_no[j];
    if (wn < 0) path_new[j] = wn == -1 ? u256_zero() : levels[-2 - wn];
  }
  uint8_t is_last = 1;
  for (uint32_t i = j + 1; i < m; i++)
    if ((sidx[i] >> l) == node) {
      is_last = 0;
      break;
    }
  last[t] = is_last;
}
// level l of both paths of every update: lane (j, side) hashes its path's digest with the sibling as it is at update j's turn.
// path_old / path_new: [(depth + 1) * m], level-major; row 0 of path_new holds the new leaves already (k_mk_leaf_states).
// wit: [old leaves m | bits m * depth | siblings m * depth], the assigned witnesses behind the new vectors.
__global__ __launch_bounds__(64) void k_mku_level(const PoseidonSpec* __restrict__ sp, const u256* __restrict__ levels, uint64_t lp,
                                                  const uint32_t* __restrict__ idx, uint32_t m, uint32_t depth, uint32_t l,
                                                  const int32_t* __restrict__ sib_from, const int32_t* __restrict__ prev_same, u256* __restrict__ wit,
                                                  u256* __restrict__ path_old, u256* __restrict__ path_new) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= 2 * m) return;
  const uint32_t j = t % m, side = t / m;
  const uint32_t node = idx[j] >> l, bit = node & 1u;
  const int32_t from = sib_from[(size_t)l * m + j];
  const u256 sib = from >= 0 ? path_new[(size_t)l * m + from] : levels[mku_level_off(lp, l) + (node ^ 1u)];
  u256 cur;
  if (side) {
    cur = path_new[(size_t)l * m + j];
  } else if (l == 0) {
    const int32_t ps = prev_same[j];
    cur = ps >= 0 ? path_new[ps] : levels[node];
    path_old[j] = cur;
    wit[j] = cur;
  } else {
    cur = path_old[(size_t)l * m + j];
  }
  if (!side) {
    wit[(size_t)m + (size_t)j * depth + l] = bit ? mont_one<Fr>() : u256_zero();
    wit[(size_t)m + (size_t)m * depth + (size_t)j * depth + l] = sib;
  }
  u256 st[PSD_T] = {sp->cap, u256_zero(), u256_zero()};
  u256 in[PSD_RATE] = {bit ? sib : cur, bit ? cur : sib};
  psd_permute_absorb(sp, st, in, 2);
  psd_permute_absorb(sp, st, in, 0);
  (side ? path_new : path_old)[(size_t)(l + 1) * m + j] = st[1];
}
// the batch's final state into the resident tree: every node's digest from the last update that touched it
__global__ __launch_bounds__(64) void k_mku_writeback(u256* __restrict__ levels, uint64_t lp, const uint32_t* __restrict__ idx, uint32_t m, uint32_t depth,
                                                      const uint8_t* __restrict__ last, const u256* __restrict__ path_new) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= m * (depth + 1)) return;
  const uint32_t j = t % m, l = t / m;
  const bool is_last = l < depth ? last[t] != 0 : j + 1 == m;
  if (is_last) levels[mku_level_off(lp, l) + (idx[j] >> l)] = path_new[t];
}
// ctx.assign_witnesses of the four input groups: plain cells, no gate (R_0 behind them is k_mku_grow_trace's)
__global__ __launch_bounds__(256) void k_mku_inputs(Streams st, uint64_t base, const u256* __restrict__ new_vectors, const u256* __restrict__ wit,
                                                    uint64_t n_vec, uint64_t n_in) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_in) return;
  const uint64_t p = base + i;
  if (p < st.rlo || p >= st.rhi) return;
  st.adv[p] = i < n_vec ? new_vectors[i] : wit[i - n_vec];
  if (st.sel) st.sel[p] = 0;
}
// the cells of one level of one update in five parts (blockIdx.y): the bit and the four selects, then the two permutations of the
// old path's hash and the two of the new path's — a lane per (update, level), a wavefront holding one part only
__global__ __launch_bounds__(64) void k_mku_level_trace(Streams stq, const FpTables* __restrict__ T, const PoseidonSpec* __restrict__ sp, MkuLayout ml,
                                                        uint64_t base, const uint64_t* __restrict__ level_at, const uint32_t* __restrict__ idx,
                                                        const u256* __restrict__ wit, const u256* __restrict__ path_old,
                                                        const u256* __restrict__ path_new) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x, part = blockIdx.y;
  const uint32_t m = ml.m, depth = ml.depth;
  if (t >= m * depth) return;
  const uint32_t j = t / depth, l = t % depth;
  const uint64_t lb = base + level_at[j] + (uint64_t)l * ml.level_cells;
  trace_path_level<2>(stq, T, sp, lb, (idx[j] >> l) & 1u, wit + ((size_t)m + (size_t)m * depth + (size_t)j * depth + l), path_old + ((size_t)l * m + j),
                      path_new + ((size_t)l * m + j), part);
}
// idx_j = gate.inner_product(bits, Constant(2^l)) per update, a delete's load_constant(0) cell (a carried leaf's load_witness cell) in
// front of its levels, and the public
// values [old root | idx, old leaf, new leaf per update | new root] (the old root of a grown tree is R_0: k_mku_grow_trace's)
__global__ __launch_bounds__(64) void k_mku_index(Streams stq, const FpTables* __restrict__ T, MkuLayout ml, uint64_t base,
                                                  const uint64_t* __restrict__ level_at, const uint32_t* __restrict__ idx,
                                                  const int32_t* __restrict__ write_no, const u256* __restrict__ wit, const u256* __restrict__ path_old,
                                                  const u256* __restrict__ path_new, u256* __restrict__ pub) {
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  const uint32_t m = ml.m, depth = ml.depth;
  if (j >= m) return;
  WCtx c = make_ctx(stq, T, base + level_at[j] - 1, 0);
  if (write_no[j] < 0) c.push(path_new[j], false, write_no[j] == -1);
  c.pos = base + level_at[j] + (uint64_t)depth * ml.level_cells;
  pub[1 + 3 * (size_t)j] = trace_path_index(c, T, idx[j], depth);   // (the assigned bits are those of idx_j: k_mku_level)
  pub[2 + 3 * (size_t)j] = wit[j];
  pub[3 + 3 * (size_t)j] = path_new[j];
  if (j == 0 && !ml.grow) pub[0] = path_old[(size_t)depth * m];
  if (j + 1 == m) pub[1 + 3 * (size_t)m] = path_new[(size_t)depth * m + j];
}
// The growth block of a batch against a tree doubled ml.grow times, and what belongs to it: the assigned R_0 in front of it and the
// public old root.  A lane per permutation of its depth - 1 + grow node hashes; every input is resident: Z_l in `empty`
// (poseidon_empty_subtrees_dev), R_i at entry 0 of level d0 + i of `levels` as long as k_mku_writeback has not run.
__global__ __launch_bounds__(64) void k_mku_grow_trace(Streams stq, const FpTables* __restrict__ T, const PoseidonSpec* __restrict__ sp, MkuLayout ml,
                                                       uint64_t base, uint64_t lp, const u256* __restrict__ levels, const u256* __restrict__ empty,
                                                       u256* __restrict__ pub) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  const uint32_t n_z = ml.depth - 1, n_hash = n_z + ml.grow;
  if (t >= 2 * n_hash) return;
  const uint64_t gb = base + ml.n_in;
  if (t == 0) {
    const u256 r0 = levels[mku_level_off(lp, ml.d0)];
    pub[0] = r0;
    WCtx c = make_ctx(stq, T, gb - 1, 0);
    c.push(r0, false);
    c.push(u256_zero(), false, true);
  }
  const uint32_t h = t >> 1, second = t & 1u;
  const uint32_t lz = h < n_z ? h : ml.d0 + (h - n_z);
  trace_node_half(stq, T, sp, gb + 1 + (uint64_t)h * NODE_CELLS, h < n_z ? empty + lz : levels + mku_level_off(lp, lz), empty + lz, second);
}

// ------------------------------------------------------------------ Merkle openings (include/vdb.h vdb_wit_merkle_open)
// m reads of slots idx_j of the resident tree `levels`, independent of each other; `levels` is only read.  Stream:
// [vectors m * D (vector mode) or leaves m (leaf mode) | bits | siblings] (the assigned witnesses), then per read its leaf sponge
// (vector mode only), per level [assert_bit | select lo | select ro | H(lo, ro)], and the index inner product.  No value pass hashes a
// path node: the digest of read j at level l and its sibling are levels[mku_level_off(lp, l) + (idx_j >> l)] and its neighbour.
struct MkoLayout : PathLayout {
  uint32_t m, with_vectors;
  uint64_t per_read, n_lead, n_in, total;
};
// ctx.assign_witnesses of the three input groups: plain cells, no gate, a lane per cell
__global__ __launch_bounds__(256) void k_mko_inputs(Streams st, uint64_t base, MkoLayout ml, uint64_t lp, const u256* __restrict__ vectors,
                                                    const u256* __restrict__ levels, const uint32_t* __restrict__ idx) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ml.n_in) return;
  const uint64_t p = base + i;
  if (p < st.rlo || p >= st.rhi) return;
  u256 v;
  if (i < ml.n_lead) {
    v = ml.with_vectors ? vectors[i] : levels[idx[i]];
  } else {
    const uint64_t n_bits = (uint64_t)ml.m * ml.depth;
    uint64_t t = i - ml.n_lead;
    const bool sibling = t >= n_bits;
    if (sibling) t -= n_bits;
    const uint32_t l = (uint32_t)(t % ml.depth), node = idx[t / ml.depth] >> l;
    v = sibling ? levels[mku_level_off(lp, l) + (node ^ 1u)] : ((node & 1u) ? mont_one<Fr>() : u256_zero());
  }
  st.adv[p] = v;
  if (st.sel) st.sel[p] = 0;
}
// the cells of one level of one read in three parts (blockIdx.y): the bit and the two selects, then the absorbing and the padding-only
// permutation of H(lo, ro) — a lane per (read, level), a wavefront holding one part only
__global__ __launch_bounds__(64) void k_mko_level_trace(Streams stq, const FpTables* __restrict__ T, const PoseidonSpec* __restrict__ sp, MkoLayout ml,
                                                        uint64_t base, uint64_t lp, const uint32_t* __restrict__ idx, const u256* __restrict__ levels) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x, part = blockIdx.y;
  const uint32_t depth = ml.depth;
  if (t >= ml.m * depth) return;
  const uint32_t j = t / depth, l = t % depth;
  const uint64_t lb = base + ml.n_in + (uint64_t)j * ml.per_read + ml.leaf_cells + (uint64_t)l * ml.level_cells;
  const uint32_t node = idx[j] >> l;
  trace_path_level<1>(stq, T, sp, lb, node & 1u, levels + mku_level_off(lp, l) + (node ^ 1u), levels + mku_level_off(lp, l) + node, nullptr, part);
}
// idx_j = gate.inner_product(bits, Constant(2^l)) per read, and the public values [root | idx, leaf per read | the vectors word by word]
// (vleaf: the sponges' digests, k_mk_leaf_states; null in leaf mode, where the leaf is the assigned one)
__global__ __launch_bounds__(64) void k_mko_index(Streams stq, const FpTables* __restrict__ T, MkoLayout ml, uint64_t base, uint64_t lp,
                                                  const uint32_t* __restrict__ idx, const u256* __restrict__ levels, const u256* __restrict__ vectors,
                                                  const u256* __restrict__ vleaf, u256* __restrict__ pub) {
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  const uint32_t m = ml.m, depth = ml.depth;
  if (j >= m) return;
  const uint32_t slot = idx[j];
  WCtx c = make_ctx(stq, T, base + ml.n_in + (uint64_t)j * ml.per_read + ml.leaf_cells + (uint64_t)depth * ml.level_cells, 0);
  pub[1 + 2 * (size_t)j] = trace_path_index(c, T, slot, depth);
  pub[2 + 2 * (size_t)j] = vleaf ? vleaf[j] : levels[slot];
  if (j == 0) pub[0] = levels[mku_level_off(lp, depth)];
  if (ml.with_vectors)
    for (uint32_t w = 0; w < ml.D; w++) pub[1 + 2 * (size_t)m + (size_t)j * ml.D + w] = vectors[(size_t)j * ml.D + w];
}

// ---- device-level drivers -------------------------------------------------------------------
int wit_distance_dev(FpEntry* fp, int metric, const u256* a, const u256* b, size_t n_pairs, size_t dim, Streams st, u256* result) {
  DistLayout dl;
  TRY(dist_layout(fp->host, metric, dim, &dl));
  TRY(inv_list_attach(st, n_pairs * dl.total_cells));
  TRY(set_winv(st, fp->dev));
  InstMap im{0, 0, 1, dl.total_cells, dl.total_lk, 0xffffffffu, 1};
  u256* mid = (u256*)scratch_get(0, n_pairs * 3 * sizeof(u256) + 64);
  if (!mid) return VDB_ERR_OOM;
  TRY(run_distances(st, fp, dl, im, (uint32_t)n_pairs, a, b, mid, result));
  return inv_list_fixup(st);
}

// ------------------------------------------------------------------ one FixedPointInstructions call per lane (vdb_wit_fp_op*)
__global__ __launch_bounds__(64) void k_fp_op(Streams st, const FpTables* __restrict__ T, int op, const u256* __restrict__ a, const u256* __restrict__ b,
                                              uint32_t n, uint32_t cells, uint32_t lks, uint64_t adv_off, uint64_t lk_off, u256* __restrict__ result) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  WCtx c = make_ctx(st, T, adv_off + (uint64_t)i * cells, lk_off + (uint64_t)i * lks);
  Gadgets g(c);
  const u256 r = fp_op_apply(g, op, a[i], b ? b[i] : u256_zero());
  result[i] = r;
  if (c.err) atomicOr(st.err, c.err);
}
int wit_fp_op_dev(FpEntry* fp, int op, const u256* a, const u256* b, size_t n, Streams st, u256* result) {
  uint32_t sz[2];
  fp_op_size(fp->host, op, sz);
  TRY(inv_list_attach(st, n * (uint64_t)sz[0]));
  TRY(set_winv(st, fp->dev));
  VDB_LAUNCH(k_fp_op, dim3((unsigned)((n + 63) / 64)), dim3(64), st, fp->dev, op, a, b, (uint32_t)n, sz[0], sz[1], 0, 0, result);
  return inv_list_fixup(st);
}

// the block of one query with `topk` rounds (include/vdb.h vdb_wit_nearest_topk): the distances, then per round the qmin chain, the
// is_equal blocks, the select_by_indicator walks and the select(M, ..) blocks, which the last round does not emit
struct NvLayout {
  uint64_t dist, dist_l, qmin, qmin_l, iseq, sel, mask, per_r, total, total_l;
};
static int nv_layout(FpEntry* fp, int metric, size_t n, size_t dim, size_t topk, DistLayout* dl, NvLayout* o) {
  TRY(dist_layout(fp->host, metric, dim, dl));
  o->dist = n * dl->total_cells;
  o->dist_l = n * dl->total_lk;
  o->qmin = (n - 1) * (uint64_t)fp->host.sz.qmin[0];
  o->qmin_l = (n - 1) * (uint64_t)fp->host.sz.qmin[1];
  o->iseq = 12ull * n;
  o->sel = dim * (1 + 3ull * n);
  o->mask = 8ull * n;
  o->per_r = o->qmin + o->iseq + o->sel + o->mask;
  o->total = o->dist + topk * o->per_r - o->mask;
  o->total_l = o->dist_l + topk * o->qmin_l;
  return VDB_OK;
}
// what one call may hold (include/vdb.h VDB_NEAREST_TOPK_MAX_*): the instance numbers of the distance kernels are 32-bit, and so are
// the lane numbers over (query, round, vector) and (query, round, dimension) before the segments multiply them; the work space is 32 B
// per (query, round, vector) and 132 B per (query, vector); the deferred-inversion counter is 32-bit (an is_zero block of eight cells
// defers at most one inverse, so 2^34 cells stay far below its wrap).
// At topk = 1 this refuses exactly the calls whose n_queries * n or n_queries * dim exceed 2^24 or whose cells exceed 2^34, the limit
// of the batch entry points: the last term is that cell limit, and the two before it follow from it — nl.dist is part of the cells,
// and the round's 8 n select(M, ..) cells, which the last round does not emit, are at most nl.dist, because one distance block has
// at least 8 cells (dist_layout: for dim >= 1 the smallest, Manhattan's, is 4 dim + dim qabs + 1, and the entry points that run ask
// for dim >= 1).
// The single-query entry points share the limit.  No call that could run is refused by it: 2^34 cells are 512 GiB of advice stream,
// more than the card's 288 GB of memory, and n or dim above 2^24 with one distance block per vector passes 2^34 cells far earlier.
static int nv_fits(size_t Q, size_t n, size_t dim, size_t topk, const NvLayout& nl) {
  if (topk == 0 || topk > n) {
    set_error("top-k: topk must be at least 1 and at most n");
    return VDB_ERR_ARG;
  }
  const size_t cap = VDB_NEAREST_TOPK_MAX_INSTANCES;
  if (Q > cap || topk > cap / Q || n > cap / (Q * topk) || dim > cap / (Q * topk) || nl.dist > VDB_NEAREST_TOPK_MAX_CELLS / Q ||
      nl.per_r > VDB_NEAREST_TOPK_MAX_CELLS / (Q * topk) || Q * nl.total > VDB_NEAREST_TOPK_MAX_CELLS) {
    set_error("nearest_vector call too large: n_queries * topk * n and n_queries * topk * dim at most 2^24, cells at most 2^34 (include/vdb.h)");
    return VDB_ERR_ARG;
  }
  return VDB_OK;
}
// segments of the select's walk over the n vectors: enough lanes to give every CU a few wavefronts, no segment below eight vectors
static uint32_t nv_select_segments(size_t QT, size_t n, size_t dim) {
  const uint64_t lanes = (uint64_t)QT * dim, want = (uint64_t)ctx().cu_count * 4 * 64;
  uint64_t s = (want + lanes - 1) / lanes, cap = n / 8;
  if (s > cap) s = cap;
  return s < 1 ? 1u : (uint32_t)s;
}
// Q x [n distances, then topk rounds of qmin chain / is_equal / select_by_indicator / mask], block q at q * (cells of one):
// one run_distances over Q x n instances (instance t = q * n + i is distance(vector_i, query_q)), one value kernel that runs every
// round of every query, and one launch per emitting stage — the launch count depends on neither Q nor topk
// (the blocks alone, Q of them from stream cell `base` / lookup cell `lbase` on: the caller has attached the inversion list and published
//  the call's context.  `fixed_launches`: the qmin chain is launched at n = 1 too, where it has no lane, so that a caller's launch count
//  does not depend on n)
static int nv_emit(FpEntry* fp, const DistLayout& dl, const NvLayout& nl, const u256* queries, const u256* vectors, size_t Q, size_t n, size_t dim,
                   size_t topk, const Streams& st, uint64_t base, uint64_t lbase, bool fixed_launches, u256* ind, u256* result) {
  const size_t inst = Q * n, rinst = inst * topk;
  InstMap im{base, lbase, (uint32_t)n, nl.total, nl.total_l, (uint32_t)n, (uint32_t)n};  // (vector_{t % n}, query_{t / n})
  u256* mid = (u256*)scratch_get(0, (inst * 4 + rinst + 8) * sizeof(u256) + inst * sizeof(uint32_t));
  if (!mid) return VDB_ERR_OOM;
  u256* dist = mid + 3 * inst;
  u256* pm = dist + inst;
  uint32_t* rnd = (uint32_t*)(pm + rinst + 8);
  TRY(run_distances(st, fp, dl, im, (uint32_t)inst, vectors, queries, mid, dist));
  const NvMap nm{base, lbase, nl.total, nl.total_l, nl.dist, nl.dist_l, nl.per_r, nl.qmin_l, nl.qmin, nl.qmin + nl.iseq,
                 nl.qmin + nl.iseq + nl.sel, (uint32_t)Q, (uint32_t)n, (uint32_t)dim, (uint32_t)topk};
  VDB_LAUNCH(k_nv_rounds, dim3((unsigned)Q), dim3(64), fp->dev, dist, (uint32_t)n, (uint32_t)topk, pm, rnd);
  if (n > 1 || fixed_launches)
    VDB_LAUNCH(k_nv_qmin, dim3((unsigned)((Q * topk * (n - 1) + 63) / 64 + (n == 1))), dim3(64), st, fp->dev, nm, dist, pm, rnd);
  VDB_LAUNCH(k_nv_is_equal, dim3((unsigned)((rinst + 63) / 64)), dim3(64), st, fp->dev, nm, dist, pm, rnd, ind);
  // launched for topk == 1 too (one wavefront that finds no lane of its own): the launch count of a call does not depend on topk
  VDB_LAUNCH(k_nv_mask, dim3((unsigned)((inst * (topk - 1) + 63) / 64 + (topk == 1))), dim3(64), st, fp->dev, nm, dist, rnd, ind);
  const uint32_t S = nv_select_segments(Q * topk, n, dim);
  VDB_LAUNCH(k_nv_select, dim3((unsigned)((Q * topk * dim * S + 63) / 64)), dim3(64), st, fp->dev, nm, S, vectors, ind, result);
  return VDB_OK;
}
int wit_nearest_dev(FpEntry* fp, int metric, const u256* queries, const u256* vectors, size_t Q, size_t n, size_t dim, size_t topk, Streams st,
                    u256* ind, u256* result) {
  DistLayout dl;
  NvLayout nl;
  TRY(nv_layout(fp, metric, n, dim, topk, &dl, &nl));
  TRY(nv_fits(Q, n, dim, topk, nl));
  TRY(inv_list_attach(st, Q * nl.total));
  TRY(set_winv(st, fp->dev));
  TRY(nv_emit(fp, dl, nl, queries, vectors, Q, n, dim, topk, st, 0, 0, false, ind, result));
  return inv_list_fixup(st);
}
// nearest_vector's distances and their minimum as values alone (include/vdb.h vdb_nearest_values_dev): the distance generators run as
// a rank runs them whose window holds no cell — k_dist_values and k_dist_tail_values compute, the emitting kernels leave at once — so the
// arithmetic is stated where the circuit's is and no stream is attached; then one wavefront per query takes the minimum.  Instance
// t = q * n + i is distance(vector_i, query_q), as in nv_emit.  The launch count depends on neither Q nor n.
int nearest_values_dev(FpEntry* fp, int metric, const u256* queries, const u256* vectors, size_t Q, size_t n, size_t dim, int* err, uint32_t* idx,
                       u256* dist_out) {
  DistLayout dl;
  NvLayout nl;
  TRY(nv_layout(fp, metric, n, dim, 1, &dl, &nl));
  TRY(nv_fits(Q, n, dim, 1, nl));
  Streams st{nullptr, nullptr, nullptr, err, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};   // the empty rank window
  TRY(inv_list_attach(st, 0));   // (an is_zero block outside every window defers nothing and inverts nothing)
  TRY(set_winv(st, fp->dev));
  const size_t inst = Q * n;
  u256* mid = (u256*)scratch_get(0, inst * 4 * sizeof(u256));
  if (!mid) return VDB_ERR_OOM;
  u256* dist = mid + 3 * inst;
  InstMap im{0, 0, (uint32_t)n, nl.total, nl.total_l, (uint32_t)n, (uint32_t)n};  // (vector_{t % n}, query_{t / n})
  TRY(run_distances(st, fp, dl, im, (uint32_t)inst, vectors, queries, mid, dist));
  VDB_LAUNCH(k_nv_argmin, dim3((unsigned)Q), dim3(64), dist, (uint32_t)n, idx, dist_out);
  return VDB_OK;
}
// the same at p rounds (include/vdb.h vdb_nearest_topk_values_dev): the distances as above, every round's prefix minima and masks by the
// witness call's own k_nv_rounds, then one wavefront per (query, round) for the round's winner.  idx / dist_out: (Q, p)
int nearest_topk_values_dev(FpEntry* fp, int metric, const u256* queries, const u256* vectors, size_t Q, size_t n, size_t dim, size_t p, int* err,
                            uint32_t* idx, u256* dist_out) {
  DistLayout dl;
  NvLayout nl;
  TRY(nv_layout(fp, metric, n, dim, p, &dl, &nl));
  TRY(nv_fits(Q, n, dim, p, nl));
  Streams st{nullptr, nullptr, nullptr, err, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};   // the empty rank window
  TRY(inv_list_attach(st, 0));
  TRY(set_winv(st, fp->dev));
  const size_t inst = Q * n, rinst = inst * p;
  u256* mid = (u256*)scratch_get(0, (inst * 4 + rinst + 8) * sizeof(u256) + inst * sizeof(uint32_t));
  if (!mid) return VDB_ERR_OOM;
  u256* dist = mid + 3 * inst;
  u256* pm = dist + inst;
  uint32_t* rnd = (uint32_t*)(pm + rinst + 8);
  InstMap im{0, 0, (uint32_t)n, nl.total, nl.total_l, (uint32_t)n, (uint32_t)n};  // (vector_{t % n}, query_{t / n})
  TRY(run_distances(st, fp, dl, im, (uint32_t)inst, vectors, queries, mid, dist));
  VDB_LAUNCH(k_nv_rounds, dim3((unsigned)Q), dim3(64), fp->dev, dist, (uint32_t)n, (uint32_t)p, pm, rnd);
  VDB_LAUNCH(k_nv_round_winners, dim3((unsigned)(Q * p)), dim3(64), fp->dev, dist, pm, rnd, (uint32_t)n, (uint32_t)p, idx, dist_out);
  return VDB_OK;
}

static int km_layout(FpEntry* fp, int metric, size_t n, size_t dim, size_t K, DistLayout* dl, KmLayout* kl) {
  TRY(dist_layout(fp->host, metric, dim, dl));
  const Sizes& z = fp->host.sz;
  kl->N = (uint32_t)n;
  kl->D = (uint32_t)dim;
  kl->K = (uint32_t)K;
  kl->per_vec = K * dl->total_cells + (K - 1) * (uint64_t)z.qmin[0] + K * 20ull;
  kl->per_vec_l = K * dl->total_lk + (K - 1) * (uint64_t)z.qmin[1];
  kl->assign = n * kl->per_vec;
  kl->assign_l = n * kl->per_vec_l;
  kl->sizes = (n - 1) * K * 4ull;
  kl->per_cluster = n * (8 + 8ull * dim) + (n - 1) * dim * 4ull + dim * (uint64_t)z.qdiv[0];
  kl->per_cluster_l = dim * (uint64_t)z.qdiv[1];
  kl->iter = kl->assign + kl->sizes + K * kl->per_cluster;
  kl->iter_l = kl->assign_l + K * kl->per_cluster_l;
  return VDB_OK;
}
int wit_kmeans_dev(FpEntry* fp, int metric, const u256* vectors, size_t n, size_t dim, size_t K, size_t I, int zero_cached, Streams st,
                   u256* cent_out, u256* ind_out) {
  DistLayout dl;
  KmLayout kl;
  TRY(km_layout(fp, metric, n, dim, K, &dl, &kl));
  TRY(inv_list_attach(st, I * kl.iter));
  TRY(set_winv(st, fp->dev));
  hipStream_t s = ctx().stream;
  size_t need = (n * K * 4 + K * dim * 2 + K + K * n * dim + 16) * sizeof(u256);
  u256* buf = (u256*)scratch_get(0, need);
  if (!buf) return VDB_ERR_OOM;
  u256* mid = buf;
  u256* dist = mid + 3 * n * K;
  u256* cent = dist + n * K;
  u256* sums = cent + K * dim;
  u256* sizes = sums + K * dim;
  u256* filt = sizes + K;
  // preamble: load_constant(quantization(1.0)); load_zero()
  VDB_LAUNCH(k_push_cells, dim3(1), dim3(1), st, 0, fp->host.c_one_q, u256_zero(), zero_cached ? 1u : 2u);
  uint64_t pos = zero_cached ? 1 : 2, lpos = 0;
  VDB_HIP(hipMemcpyAsync(cent, vectors, K * dim * sizeof(u256), hipMemcpyDeviceToDevice, s));
  u256 scale_inv = mont_inv<Fr>(fp->host.scale);
  for (size_t it = 0; it < I; it++) {
    InstMap im{pos, lpos, (uint32_t)K, kl.per_vec, kl.per_vec_l, (uint32_t)K, (uint32_t)K};  // distance(centroid_k, vector_v)
    TRY(run_distances(st, fp, dl, im, (uint32_t)(n * K), cent, vectors, mid, dist));
    VDB_LAUNCH(k_km_assign, dim3((unsigned)((n + 63) / 64), (unsigned)(2 * K)), dim3(64), st, fp->dev, kl, dl, pos, lpos, dist, ind_out);
    VDB_LAUNCH(k_km_sizes, dim3((unsigned)K), dim3(64), st, fp->dev, kl, pos + kl.assign, ind_out, sizes);
    uint64_t cb = pos + kl.assign + kl.sizes, clb = lpos + kl.assign_l;
    VDB_LAUNCH(k_km_filter, dim3((unsigned)((K * n * ((dim + KM_PF - 1) / KM_PF) + 63) / 64)), dim3(64), st, fp->dev, kl, cb, vectors, ind_out, scale_inv,
               filt);
    VDB_LAUNCH(k_km_sum, dim3((unsigned)(K * dim)), dim3(64), st, fp->dev, kl, cb, filt, sums);
    VDB_LAUNCH(k_km_div, dim3((unsigned)((K * dim + 63) / 64), 8), dim3(64), st, fp->dev, kl, cb, clb, sums, sizes, cent);
    pos += kl.iter;
    lpos += kl.iter_l;
  }
  VDB_HIP(hipMemcpyAsync(cent_out, cent, K * dim * sizeof(u256), hipMemcpyDeviceToDevice, s));
  return inv_list_fixup(st);
}

// merkle_commitment over n vectors of `dim` words: the tree's shape (MkShape, resident.hpp) and the cells of its trace
struct MkLayout : MkShape {
  uint64_t leaf_cells, leaves, zero_cell, total;
};
static void mk_layout(size_t n, size_t dim, int zero_cached, MkLayout* o) {
  mk_shape(n, dim, o);
  o->leaf_cells = 0;
  for (uint32_t p = 0; p < o->nperm; p++) o->leaf_cells += perm_cells(leaf_absorbs(dim, p));
  o->leaves = n * o->leaf_cells;
  const uint64_t lp = o->n_leaves_pow2;
  o->zero_cell = (lp > n && !zero_cached) ? 1 : 0;
  o->total = o->leaves + o->zero_cell + (lp - 1) * (uint64_t)NODE_CELLS;
}
// the centroids' tree, then the members' tree behind it in the same context: Context::load_zero caches its cell, so where the centroids'
// padding has loaded it the members' padding does not load it again
static void mk_layout_pair(size_t K, size_t n_c, size_t dim, MkLayout* mc, MkLayout* mm) {
  mk_layout(K, dim, 0, mc);
  mk_layout(n_c, dim, (int)mc->zero_cell, mm);
}
// merkle_commitment's cells from stream cell `base` on (the caller has published the call's context).  `resident`: the tree's digests
// where they already lie on the device (vdb_merkle_tree_build_dev's layout, only read) — then only the leaves' sponge states are computed,
// and the launch count does not depend on n (the zero cell and the tree trace are launched where they have nothing to store, too);
// null: the digests are computed here, a launch per level
static int mk_emit(FpEntry* fp, const PoseidonSpec* sp, const u256* vectors, size_t n, size_t dim, const MkLayout& ml, const Streams& st, uint64_t base,
                   const u256* resident, u256* root_out) {
  const uint64_t lp = ml.n_leaves_pow2;
  u256* states = (u256*)scratch_get(0, (n * ml.nperm * PSD_T + 2 * lp + 8) * sizeof(u256));
  if (!states) return VDB_ERR_OOM;
  u256* levels = states + n * ml.nperm * PSD_T;
  uint64_t root_off = 2 * lp - 2;
  if (resident)  // (the leaf digests the kernel writes beside the states are the resident ones again)
    TRY(mk_leaf_states(sp, vectors, (uint32_t)n, (uint32_t)dim, ml.nperm, states, levels, nullptr));
  else
    TRY(mk_tree_values(sp, vectors, n, dim, ml, states, levels, &root_off));
  const u256* lv = resident ? resident : levels;
  VDB_LAUNCH(k_mk_leaf_trace, dim3((unsigned)((n * ml.nperm + 63) / 64)), dim3(64), st, fp->dev, sp, vectors, (uint32_t)n, (uint32_t)dim, ml.nperm, base,
             ml.leaf_cells, states, nullptr);
  if (ml.zero_cell || resident)
    VDB_LAUNCH(k_push_cells, dim3(1), dim3(1), st, base + ml.leaves, u256_zero(), u256_zero(), ml.zero_cell ? 1u : 0u);
  // every node's two permutations in one launch (a tree of one leaf has no node: its root is the leaf digest)
  if (lp > 1 || resident)
    VDB_LAUNCH(k_mk_tree_trace, dim3((unsigned)((2 * (lp - 1) + 63) / 64 + (lp == 1))), dim3(64), st, fp->dev, sp, lv, (uint32_t)lp,
               base + ml.leaves + ml.zero_cell);
  if (root_out) VDB_HIP(hipMemcpyAsync(root_out, lv + root_off, sizeof(u256), hipMemcpyDeviceToDevice, ctx().stream));
  return VDB_OK;
}
// what a Poseidon-only witness call starts with: the gate tables, the call's context published, the permutation's constants
static int mk_begin(const Streams& st, FpEntry** fp, const PoseidonSpec** sp) {
  TRY(get_fp(48, 13, fp));  // only GateChip primitives are used: P and L are irrelevant
  TRY(set_winv(st, (*fp)->dev));
  return poseidon_spec_dev(sp, nullptr);
}
int wit_merkle_dev(const u256* vectors, size_t n, size_t dim, int zero_cached, Streams st, u256* root_out) {
  VDB_ARG(n <= ((size_t)1 << 30), "tree deeper than 30 levels");
  FpEntry* fp;
  const PoseidonSpec* sp;
  TRY(mk_begin(st, &fp, &sp));
  MkLayout ml;
  mk_layout(n, dim, zero_cached, &ml);
  return mk_emit(fp, sp, vectors, n, dim, ml, st, 0, nullptr, root_out);
}

// The part of a path circuit's layout that updates (sides = 2: an old and a new running digest per level) and reads (sides = 1) share,
// with the limits both have (include/vdb.h): a tree over n vectors of `dim` words, doubled `grow` times; *lp: its padded leaf count
static int path_layout(size_t n, size_t dim, unsigned grow, int sides, PathLayout* o, uint64_t* lp) {
  VDB_ARG(n > 0 && dim > 0, "empty database");
  VDB_ARG(n <= ((size_t)1 << 30) && dim <= ((size_t)1 << 20), "tree deeper than 30 levels or vector longer than 2^20 words");
  MkLayout ml;
  mk_layout(n, dim, 0, &ml);
  VDB_ARG(ml.depth + (uint64_t)grow <= 30, "grown tree deeper than 30 levels");
  o->D = (uint32_t)dim;
  o->depth = ml.depth + (uint32_t)grow;
  VDB_ARG(o->depth >= 1, "a tree of one leaf has no path (depth 0)");
  o->nperm = ml.nperm;
  o->leaf_cells = ml.leaf_cells;
  o->level_cells = path_level_cells(sides);
  o->ip_cells = 1 + 3 * (uint64_t)(o->depth - 1);
  *lp = ml.n_leaves_pow2 << grow;
  return VDB_OK;
}
// sizes of a batch of m path updates (kinds: 0 write, 1 delete; null: all writes) in a tree over n vectors grown `grow` times; the
// limits of one call (include/vdb.h).  level_at (m; null: not wanted): where the levels of update j start in the stream, behind its
// leaf sponge or its zero cell; write_no (m): the row of new_vectors update j writes, -1 for a delete.
// `carried` admits kind 2, a carried leaf: one load_witness cell where a delete has its zero (write_no -2; the index delete's alone)
static int mku_layout(size_t n, size_t dim, size_t m, const uint8_t* kinds, unsigned grow, MkuLayout* o, uint64_t* lp_out, uint64_t* level_at,
                      int32_t* write_no, bool carried = false) {
  uint64_t lp;
  TRY(path_layout(n, dim, grow, 2, o, &lp));
  VDB_ARG(m > 0, "a batch holds at least one update");
  VDB_ARG(m <= MKU_MAX_UPDATES, "more than VDB_MERKLE_UPDATE_MAX_UPDATES updates in one call");
  const uint32_t depth = o->depth;
  size_t w = 0;
  for (size_t j = 0; j < m; j++) {
    VDB_ARG(!kinds || kinds[j] <= (carried ? 2 : 1), "an update is a write (0) or a delete (1)");
    w += !kinds || kinds[j] == 0;
  }
  o->m = (uint32_t)m;
  o->w = (uint32_t)w;
  o->d0 = depth - (uint32_t)grow;
  o->grow = (uint32_t)grow;
  o->n_vec = (uint64_t)w * dim;
  o->n_wit = (uint64_t)m * (1 + 2 * (uint64_t)depth);
  o->n_in = o->n_vec + o->n_wit + (grow ? 1 : 0);
  o->grow_cells = grow ? 1 + (uint64_t)(depth - 1 + grow) * NODE_CELLS : 0;
  uint64_t at = o->n_in + o->grow_cells;
  int32_t wn = 0;
  for (size_t j = 0; j < m; j++) {
    const bool del = kinds && kinds[j];
    at += del ? 1 : o->leaf_cells;
    if (level_at) level_at[j] = at;
    if (write_no) write_no[j] = del ? -(int32_t)kinds[j] : wn++;
    at += depth * o->level_cells + o->ip_cells;
  }
  o->total = at;
  VDB_ARG(o->total <= ((uint64_t)1 << 34) && (uint64_t)m * o->nperm <= ((uint64_t)1 << 30), "more than VDB_MERKLE_UPDATE_MAX_CELLS cells in one call");
  if (lp_out) *lp_out = lp;
  return VDB_OK;
}
// What a batch of updates is on the host before anything is launched (mku_plan): its layout and, in one array that a single upload
// takes to the device, [level_at m | leaf_at w: where the sponge of write v starts | idx m | write_no m | write_of w: the update of write v]
struct MkuPlan {
  MkuLayout ml;
  uint64_t lp;
  size_t n_tab;
  std::vector<uint64_t> level_at, tab;   // (tab: the pageable source of the upload; hipMemcpyAsync stages it before returning)
  std::vector<int32_t> write_no;
};
// carry_src (null: no kind 2 is admitted): for an update of kind 2 the slot whose resident digest is its new leaf; carry_n > 0: the
// digest is entry carry_src[j] of a second array of carry_n digests, which mku_emit is given (the index move's append: a leaf of the
// OTHER cluster's tree)
static int mku_plan(size_t n, size_t dim, unsigned grow, const u256* new_vectors, const uint64_t* indices, const uint8_t* kinds, size_t m, MkuPlan* p,
                    const uint32_t* carry_src = nullptr, uint64_t carry_n = 0) {
  VDB_ARG(m > 0 && m <= MKU_MAX_UPDATES, "a batch holds 1 .. VDB_MERKLE_UPDATE_MAX_UPDATES updates");
  p->level_at.resize(m);
  p->write_no.resize(m);
  MkuLayout& ml = p->ml;
  TRY(mku_layout(n, dim, m, kinds, grow, &ml, &p->lp, p->level_at.data(), p->write_no.data(), carry_src != nullptr));
  VDB_ARG(new_vectors || ml.w == 0, "null pointer: a write needs its new vector");
  const size_t w = ml.w;
  p->n_tab = (m + w) * sizeof(uint64_t) + (2 * m + w) * sizeof(uint32_t);
  p->tab.resize(p->n_tab / sizeof(uint64_t) + 1);
  uint64_t* p_level_at = p->tab.data();
  uint64_t* p_leaf_at = p_level_at + m;
  uint32_t* p_idx = (uint32_t*)(p_leaf_at + w);
  int32_t* p_write_no = (int32_t*)(p_idx + m);
  uint32_t* p_write_of = (uint32_t*)(p_write_no + m);
  for (size_t j = 0; j < m; j++) {
    VDB_ARG(indices[j] < p->lp, "update index outside the padded tree (grow it first: vdb_merkle_tree_grow_dev)");
    p_level_at[j] = p->level_at[j];
    p_idx[j] = (uint32_t)indices[j];
    if (p->write_no[j] == -2) {
      VDB_ARG(carry_src[j] < (carry_n ? carry_n : p->lp), "carried leaf outside the padded tree");
      p->write_no[j] = -2 - (int32_t)carry_src[j];
    }
    p_write_no[j] = p->write_no[j];
    if (p->write_no[j] >= 0) {
      p_leaf_at[p->write_no[j]] = p->level_at[j] - ml.leaf_cells;
      p_write_of[p->write_no[j]] = (uint32_t)j;
    }
  }
  return VDB_OK;
}
// The cells of a planned batch from stream cell `base` on, and its 3 m + 2 public values into `pub` (the caller has published the call's
// context: mk_begin).  `levels`: the tree at depth d + grow (merkle_tree_grow_dev's when grow > 0), left in the state after the batch;
// new_vectors: the rows of the writes in update order; carry (null: `levels`): the array a carried leaf names its digest in
static int mku_emit(FpEntry* fp, const PoseidonSpec* sp, const MkuPlan& pl, u256* levels, size_t dim, const u256* new_vectors, const Streams& st,
                    uint64_t base, u256* pub, const u256* carry = nullptr) {
  const MkuLayout& ml = pl.ml;
  const uint64_t lp = pl.lp;
  const size_t m = ml.m, w = ml.w, n_tab = pl.n_tab;
  const unsigned grow = ml.grow;
  const u256* empty = nullptr;
  if (grow) TRY(poseidon_empty_subtrees_dev(&empty));
  hipStream_t s = ctx().stream;
  const uint32_t depth = ml.depth;
  const size_t n_states = w * ml.nperm * PSD_T, n_wit = ml.n_wit, n_path = m * ((size_t)depth + 1);
  const size_t n_u256 = n_states + n_wit + 2 * n_path;
  const size_t need = n_u256 * sizeof(u256) + n_tab + (m * depth + m) * sizeof(uint32_t) + m * depth + 64;
  u256* buf = (u256*)scratch_get(0, need);
  if (!buf) return VDB_ERR_OOM;
  u256* states = buf;
  u256* wit = states + n_states;
  u256* path_old = wit + n_wit;
  u256* path_new = path_old + n_path;
  uint64_t* level_at = (uint64_t*)(path_new + n_path);
  uint64_t* leaf_at = level_at + m;
  uint32_t* didx = (uint32_t*)(leaf_at + w);
  int32_t* write_no = (int32_t*)(didx + m);
  uint32_t* write_of = (uint32_t*)(write_no + m);
  int32_t* sib_from = (int32_t*)(write_of + w);
  int32_t* prev_same = sib_from + m * depth;
  uint8_t* last = (uint8_t*)(prev_same + m);
  VDB_HIP(hipMemcpyAsync(level_at, pl.tab.data(), n_tab, hipMemcpyHostToDevice, s));
  const uint32_t mu = (uint32_t)m, wu = (uint32_t)w;
  // grids of at least one block: the launches of a call do not depend on how many of its updates are writes
  VDB_LAUNCH(k_mku_touchers, dim3((unsigned)((m * depth + 255) / 256)), dim3(256), didx, mu, depth, sib_from, prev_same, last, write_no,
             carry ? carry : levels, path_new);
  TRY(mk_leaf_states(sp, new_vectors, wu, (uint32_t)dim, ml.nperm, states, path_new, write_of));
  for (uint32_t l = 0; l < depth; l++)
    VDB_LAUNCH(k_mku_level, dim3((unsigned)((2 * m + 63) / 64)), dim3(64), sp, levels, lp, didx, mu, depth, l, sib_from, prev_same, wit, path_old, path_new);
  if (grow)  // R_i and the public old root, read before the write-back replaces them
    VDB_LAUNCH(k_mku_grow_trace, dim3((unsigned)((2 * (depth - 1 + grow) + 63) / 64)), dim3(64), st, fp->dev, sp, ml, base, lp, levels, empty, pub);
  VDB_LAUNCH(k_mku_writeback, dim3((unsigned)((n_path + 63) / 64)), dim3(64), levels, lp, didx, mu, depth, last, path_new);
  VDB_LAUNCH(k_mku_inputs, dim3((unsigned)((ml.n_vec + n_wit + 255) / 256)), dim3(256), st, base, new_vectors, wit, ml.n_vec, ml.n_vec + n_wit);
  VDB_LAUNCH(k_mk_leaf_trace, dim3((unsigned)((w * ml.nperm + 63) / 64 + (w == 0))), dim3(64), st, fp->dev, sp, new_vectors, wu, (uint32_t)dim, ml.nperm, base,
             ml.leaf_cells, states, leaf_at);
  VDB_LAUNCH(k_mku_level_trace, dim3((unsigned)((m * depth + 63) / 64), 5), dim3(64), st, fp->dev, sp, ml, base, level_at, didx, wit, path_old, path_new);
  VDB_LAUNCH(k_mku_index, dim3((unsigned)((m + 63) / 64)), dim3(64), st, fp->dev, ml, base, level_at, didx, write_no, wit, path_old, path_new, pub);
  return VDB_OK;
}
// vdb_wit_merkle_update_ops: the batch alone, at stream cell 0
int wit_merkle_update_dev(u256* levels, size_t n, size_t dim, unsigned grow, const u256* new_vectors, const uint64_t* indices, const uint8_t* kinds,
                          size_t m, Streams st, u256* pub) {
  static thread_local MkuPlan pl;
  TRY(mku_plan(n, dim, grow, new_vectors, indices, kinds, m, &pl));
  FpEntry* fp;
  const PoseidonSpec* sp;
  TRY(mk_begin(st, &fp, &sp));
  return mku_emit(fp, sp, pl, levels, dim, new_vectors, st, 0, pub);
}

// sizes of m openings in a tree over n vectors; the limits of one call (include/vdb.h).  No cap on m beyond the cell count: nothing
// is scanned in LDS.
static int mko_layout(size_t n, size_t dim, size_t m, int with_vectors, MkoLayout* o, uint64_t* lp_out) {
  uint64_t lp;
  TRY(path_layout(n, dim, 0, 1, o, &lp));
  VDB_ARG(m > 0, "a call opens at least one slot");
  const uint32_t depth = o->depth;
  VDB_ARG(m < ((size_t)1 << 31) && (uint64_t)m * depth < ((uint64_t)1 << 31), "2^31 or more (read, level) pairs in one call");
  o->m = (uint32_t)m;
  o->with_vectors = with_vectors ? 1u : 0u;
  if (!with_vectors) o->nperm = 0, o->leaf_cells = 0;   // leaf mode: the leaf is assigned, no sponge
  o->per_read = o->leaf_cells + depth * o->level_cells + o->ip_cells;
  o->n_lead = with_vectors ? (uint64_t)m * dim : (uint64_t)m;
  o->n_in = o->n_lead + 2 * (uint64_t)m * depth;
  o->total = o->n_in + (uint64_t)m * o->per_read;
  VDB_ARG(o->total <= ((uint64_t)1 << 34), "more than VDB_MERKLE_OPEN_MAX_CELLS cells in one call");
  if (lp_out) *lp_out = lp;
  return VDB_OK;
}
// every opened slot lies in the padded tree, and in vector mode holds a vector
static int mko_check_indices(const uint64_t* indices, size_t m, uint64_t lp, size_t n, int with_vectors) {
  for (size_t j = 0; j < m; j++) {
    VDB_ARG(indices[j] < lp, "opened slot outside the padded tree");
    VDB_ARG(!with_vectors || indices[j] < n, "opened slot holds no vector (open it in leaf mode: its leaf is 0)");
  }
  return VDB_OK;
}
int wit_merkle_open_dev(const u256* levels, size_t n, size_t dim, const u256* vectors, const uint64_t* indices, size_t m, Streams st, u256* pub) {
  MkoLayout ml;
  uint64_t lp;
  TRY(mko_layout(n, dim, m, vectors != nullptr, &ml, &lp));
  TRY(mko_check_indices(indices, m, lp, n, vectors != nullptr));
  static thread_local std::vector<uint32_t> hidx;  // pageable source: hipMemcpyAsync stages it before returning
  hidx.resize(m);
  for (size_t j = 0; j < m; j++) hidx[j] = (uint32_t)indices[j];
  FpEntry* fp;
  const PoseidonSpec* sp;
  TRY(mk_begin(st, &fp, &sp));
  const size_t n_states = m * ml.nperm * PSD_T, n_leaf = vectors ? m : 0;
  u256* states = (u256*)scratch_get(0, (n_states + n_leaf) * sizeof(u256) + m * sizeof(uint32_t) + 64);
  if (!states) return VDB_ERR_OOM;
  u256* vleaf = vectors ? states + n_states : nullptr;
  uint32_t* didx = (uint32_t*)(states + n_states + n_leaf);
  VDB_HIP(hipMemcpyAsync(didx, hidx.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, ctx().stream));
  const uint32_t mu = (uint32_t)m, depth = ml.depth;
  VDB_LAUNCH(k_mko_inputs, dim3((unsigned)((ml.n_in + 255) / 256)), dim3(256), st, 0, ml, lp, vectors, levels, didx);
  if (vectors) {
    TRY(mk_leaf_states(sp, vectors, mu, (uint32_t)dim, ml.nperm, states, vleaf, nullptr));
    VDB_LAUNCH(k_mk_leaf_trace, dim3((unsigned)((m * ml.nperm + 63) / 64)), dim3(64), st, fp->dev, sp, vectors, mu, (uint32_t)dim, ml.nperm, ml.n_in,
               ml.per_read, states, nullptr);
  }
  VDB_LAUNCH(k_mko_level_trace, dim3((unsigned)(((uint64_t)m * depth + 63) / 64), 3), dim3(64), st, fp->dev, sp, ml, 0, lp, didx, levels);
  VDB_LAUNCH(k_mko_index, dim3((unsigned)((m + 63) / 64)), dim3(64), st, fp->dev, ml, 0, lp, didx, levels, vectors, vleaf, pub);
  return VDB_OK;
}

// ------------------------------------------------------------------ an approximate-nearest-neighbour query against the committed index:
// over the p nearest clusters, the t nearest candidates (include/vdb.h vdb_wit_ann_probe; the single-cluster vdb_wit_ann_query is this at
// p = t = 1; the index itself, its forest of K + 1 trees and their roots: resident.hip).
// [query | centroids | candidates | cluster roots] assigned, then nearest_vector(query, centroids) with p rounds, merkle_commitment(centroids),
// nearest_vector(query, candidates) with t rounds, one merkle_commitment per probed cluster, one select_by_indicator(cluster roots, centroid
// indicator of the round) per probed cluster — which the map ties to that cluster's root — and the sponge over [centroids' root | cluster
// roots].  Where its blocks start:
struct AnnpLayout {
  DistLayout dl;
  NvLayout nc, nm;
  MkLayout mc, mw, mm[VDB_ANN_PROBE_MAX];
  uint64_t off[VDB_ANN_PROBE_MAX + 1];   // candidate rows [off[r], off[r + 1]) are the cluster of round r
  uint64_t b_mm[VDB_ANN_PROBE_MAX];
  uint64_t N, n_in, b_nc, b_mc, b_nm, b_sel, b_root, total, l_nm, total_l;
};
static int annp_layout(FpEntry* fp, int metric, size_t K, size_t dim, size_t p, const size_t* n_c, size_t t, AnnpLayout* o) {
  VDB_ARG(K > 0 && dim > 0, "K = 0 or dim = 0");
  VDB_ARG(K <= VDB_ANN_MAX_CLUSTERS && dim <= ((size_t)1 << 20), "query too large (include/vdb.h)");
  VDB_ARG(p >= 1 && p <= K, "probes: at least 1 and at most K");
  VDB_ARG(p <= VDB_ANN_PROBE_MAX, "probes above VDB_ANN_PROBE_MAX");
  VDB_ARG(n_c != nullptr, "null pointer");
  o->off[0] = 0;
  for (size_t r = 0; r < p; r++) {
    VDB_ARG(n_c[r] > 0, "empty cluster");
    VDB_ARG(n_c[r] <= VDB_ANN_MAX_VECTORS, "candidates above VDB_ANN_MAX_VECTORS");
    o->off[r + 1] = o->off[r] + n_c[r];
  }
  const size_t N = o->N = o->off[p];
  VDB_ARG(N <= VDB_ANN_MAX_VECTORS, "candidates above VDB_ANN_MAX_VECTORS");
  VDB_ARG(t >= 1 && t <= N, "topk: at least 1 and at most the number of candidates");
  TRY(nv_layout(fp, metric, K, dim, p, &o->dl, &o->nc));
  TRY(nv_fits(1, K, dim, p, o->nc));
  TRY(nv_layout(fp, metric, N, dim, t, &o->dl, &o->nm));
  TRY(nv_fits(1, N, dim, t, o->nm));
  // the chain of p + 1 trees in one context: the first padded one loads the zero cell, every later padded one copies it
  mk_layout(K, dim, 0, &o->mc);
  int zero = (int)o->mc.zero_cell;
  mk_layout(1, K + 1, 1, &o->mw);
  o->n_in = dim + K * dim + N * dim + K;
  o->b_nc = o->n_in;
  o->b_mc = o->b_nc + o->nc.total;
  o->b_nm = o->b_mc + o->mc.total;
  uint64_t at = o->b_nm + o->nm.total;
  for (size_t r = 0; r < p; r++) {
    mk_layout(n_c[r], dim, zero, &o->mm[r]);
    zero |= (int)o->mm[r].zero_cell;
    o->b_mm[r] = at;
    at += o->mm[r].total;
  }
  o->b_sel = at;
  o->b_root = o->b_sel + p * (1 + 3 * (uint64_t)K);
  o->total = o->b_root + o->mw.total;
  o->l_nm = o->nc.total_l;
  o->total_l = o->nc.total_l + o->nm.total_l;
  VDB_ARG(o->total <= VDB_NEAREST_TOPK_MAX_CELLS, "query circuit above 2^34 cells");
  return VDB_OK;
}
// where the candidates lie: the p clusters' rows and the prefix sums of their sizes
struct AnnpSegments {
  const u256* rows[VDB_ANN_PROBE_MAX];
  uint32_t pre[VDB_ANN_PROBE_MAX + 1];
};
// The candidates in one pass: lane i is word i of the N x dim candidates — consecutive lanes, consecutive words of one row — read from
// the cluster whose prefix sums hold its row (bisection, as k_ann_forest_level finds its segment), written to the contiguous buffer the
// second search reads and, inside the rank window, to its assigned cell (ctx.assign_witnesses: no gate, no constant flag).
__global__ __launch_bounds__(256) void k_annp_gather(Streams st, uint64_t base, const AnnpSegments* __restrict__ sg, uint32_t p, uint32_t D,
                                                     u256* __restrict__ cand) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (uint64_t)sg->pre[p] * D) return;
  const uint32_t row = (uint32_t)(i / D), j = (uint32_t)(i % D);
  uint32_t lo = 0, hi = p;   // the last segment s with pre[s] <= row (no segment is empty)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (sg->pre[mid] <= row) lo = mid; else hi = mid;
  }
  const u256 v = sg->rows[lo][(uint64_t)(row - sg->pre[lo]) * D + j];
  cand[i] = v;
  const uint64_t pos = base + i;
  if (pos < st.rlo || pos >= st.rhi) return;
  st.adv[pos] = v;
  if (st.sel) st.sel[pos] = 0;
}
// members: HOST array of the p clusters' rows on the device; levels_c / levels_m (HOST array of p): the p + 1 trees where they are
// resident, or null.  pub: the t x dim result words, nearest first, then the index root.
int wit_ann_probe_dev(FpEntry* fp, int metric, const u256* query, const u256* centroids, const u256* const* members, const u256* cluster_roots,
                      const u256* levels_c, const u256* const* levels_m, size_t K, size_t dim, size_t p, const size_t* n_c, size_t t, Streams st,
                      u256* ind_c, u256* ind_m, u256* pub) {
  AnnpLayout a;
  static thread_local AnnpSegments hseg;   // pageable source of an asynchronous upload: it outlives the call
  TRY(annp_layout(fp, metric, K, dim, p, n_c, t, &a));
  const PoseidonSpec* sp;
  TRY(poseidon_spec_dev(&sp, nullptr));
  const size_t N = a.N;
  // work space of the call: [centroids' root | cluster roots], the p selected roots, the first search's results, the sponge's states,
  // the candidates, the segment table
  const size_t n_words = K + 1 + p + p * dim + 8 + (size_t)a.mw.nperm * PSD_T + N * dim;
  u256* words = (u256*)scratch_get(7, n_words * sizeof(u256) + sizeof(AnnpSegments));
  if (!words) return VDB_ERR_OOM;
  u256 *picked = words + K + 1, *res_c = picked + p, *wstates = res_c + p * dim + 8, *cand = wstates + (size_t)a.mw.nperm * PSD_T;
  AnnpSegments* dseg = (AnnpSegments*)(cand + N * dim);
  TRY(inv_list_attach(st, a.total));
  TRY(set_winv(st, fp->dev));
  hipStream_t s = ctx().stream;
  for (size_t r = 0; r < VDB_ANN_PROBE_MAX; r++) hseg.rows[r] = r < p ? members[r] : nullptr;
  for (size_t r = 0; r <= VDB_ANN_PROBE_MAX; r++) hseg.pre[r] = (uint32_t)a.off[r < p ? r : p];
  VDB_HIP(hipMemcpyAsync(dseg, &hseg, sizeof(AnnpSegments), hipMemcpyHostToDevice, s));
  const uint64_t b_cand = dim + K * dim, b_roots = b_cand + N * dim;
  VDB_LAUNCH(k_mku_inputs, dim3((unsigned)((dim + K * dim + 255) / 256)), dim3(256), st, 0, query, centroids, (uint64_t)dim, (uint64_t)(dim + K * dim));
  VDB_LAUNCH(k_annp_gather, dim3((unsigned)((N * dim + 255) / 256)), dim3(256), st, b_cand, dseg, (uint32_t)p, (uint32_t)dim, cand);
  VDB_LAUNCH(k_mku_inputs, dim3((unsigned)((K + 255) / 256)), dim3(256), st, b_roots, cluster_roots, cluster_roots, (uint64_t)K, (uint64_t)K);
  TRY(nv_emit(fp, a.dl, a.nc, query, centroids, 1, K, dim, p, st, a.b_nc, 0, true, ind_c, res_c));
  TRY(mk_emit(fp, sp, centroids, K, dim, a.mc, st, a.b_mc, levels_c, words));
  TRY(nv_emit(fp, a.dl, a.nm, query, cand, 1, N, dim, t, st, a.b_nm, a.l_nm, true, ind_m, pub));
  for (size_t r = 0; r < p; r++)
    TRY(mk_emit(fp, sp, cand + a.off[r] * dim, n_c[r], dim, a.mm[r], st, a.b_mm[r], levels_m ? levels_m[r] : nullptr, nullptr));
  VDB_HIP(hipMemcpyAsync(words + 1, cluster_roots, K * sizeof(u256), hipMemcpyDeviceToDevice, s));
  // the p selections end to end: rounds of 1 + 3 K cells, one dimension, over the cluster roots
  const NvMap sm{a.b_sel, 0, 0, 0, 0, 0, 1 + 3 * (uint64_t)K, 0, 0, 0, 0, 1u, (uint32_t)K, 1u, (uint32_t)p};
  VDB_LAUNCH(k_nv_select, dim3(1), dim3(64), st, fp->dev, sm, 1u, cluster_roots, ind_c, picked);
  TRY(mk_leaf_states(sp, words, 1u, (uint32_t)(K + 1), a.mw.nperm, wstates, pub + t * dim, nullptr));
  VDB_LAUNCH(k_mk_leaf_trace, dim3((unsigned)((a.mw.nperm + 63) / 64)), dim3(64), st, fp->dev, sp, words, 1u, (uint32_t)(K + 1), a.mw.nperm, a.b_root,
             a.mw.leaf_cells, wstates, nullptr);
  return inv_list_fixup(st);
}

// ------------------------------------------------------------------ inserts and replacements against the index root (include/vdb.h
// vdb_wit_ann_update, vdb_ann_index_apply_dev).  m writes into cluster c move index_root_old to index_root_new in one circuit:
// A [c | centroids_root | cluster roots] assigned, B idx_to_indicator(c, K), C select_by_indicator(cluster roots, indicators) -> picked,
// D the sponge over the header's roots, E the update block of the cluster's tree (mku_emit at its base), F out_j = select(new cluster
// root, cluster_root_j, indicator_j), G the sponge over [centroids_root | out_j].  The map ties picked to E's old root.  A - D, F and G
// are the frame of every batch against the index root (AnnFrame: the delete below puts its own blocks into the same frame).
struct AnnuLayout {
  MkLayout mw;
  AnnuBlocks b;
};
// the header: lane i < K + 2 assigns cell i and keeps the value for the blocks that read it
__global__ __launch_bounds__(256) void k_annu_header(Streams st, uint64_t base, uint32_t c, const u256* __restrict__ roots, uint32_t K,
                                                     u256* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K + 2) return;
  const u256 v = i ? roots[i - 1] : Gadgets::mont_small(c);
  hdr[i] = v;
  const uint64_t p = base + i;
  if (p < st.rlo || p >= st.rhi) return;
  st.adv[p] = v;
  if (st.sel) st.sel[p] = 0;
}
// idx_to_indicator(c, K) as g_select_from_idx unrolls it, a lane per j: indicator 0 is is_zero(c) (8 cells), indicator j >= 1 is
// is_equal(c, Constant(j)) (12 cells); the inverse of c - j comes from the small-inverse table or goes through the inverse list
__global__ __launch_bounds__(64) void k_annu_indicator(Streams st, const FpTables* __restrict__ T, uint64_t base, uint32_t c, uint32_t K,
                                                       u256* __restrict__ ind) {
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  if (j >= K) return;
  ind[j] = j == c ? mont_one<Fr>() : u256_zero();
  WCtx cx = make_ctx(st, T, base + annu_indicator_off(j), 0);
  Gadgets g(cx);
  if (cx.skip(j ? 12 : 8)) return;
  const int64_t diff = (int64_t)c - (int64_t)j;
  const u256 idx = Gadgets::mont_small(c);
  if (j == 0) {
    g.g_is_zero_inv(idx, g.signed_small_inv(idx, diff));
  } else {
    const u256 cj = Gadgets::mont_small(j), d = fr_sub(idx, cj);
    cx.push(d, true); cx.push(cj, false, true); cx.push(mont_one<Fr>(), false, true); cx.push(idx, false);
    g.g_is_zero_inv(d, g.signed_small_inv(d, diff));
  }
}
// out_j = select(new cluster root, cluster_root_j, indicator_j), a lane per j; out_j is word 1 + j of the new sponge (word 0: the
// centroids' root, lane 0's)
__global__ __launch_bounds__(64) void k_annu_new_roots(Streams st, const FpTables* __restrict__ T, uint64_t base, uint32_t K,
                                                       const u256* __restrict__ new_root, const u256* __restrict__ words_old,
                                                       const u256* __restrict__ ind, u256* __restrict__ words_new) {
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  if (j >= K) return;
  if (j == 0) words_new[0] = words_old[0];
  WCtx cx = make_ctx(st, T, base + 8ull * j, 0);
  Gadgets g(cx);
  words_new[1 + j] = g.g_select(*new_root, words_old[1 + j], ind[j]);
}
// [index_root_old | c | idx_j, old_leaf_j, new_leaf_j per write | index_root_new] from the update block's own public values
__global__ __launch_bounds__(256) void k_annu_public(const u256* __restrict__ upub, const u256* __restrict__ hdr, const u256* __restrict__ iroot,
                                                     uint32_t m, u256* __restrict__ pub) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * m + 3) return;
  pub[i] = i == 0 ? iroot[0] : i == 1 ? hdr[0] : i == 3 * m + 2 ? iroot[1] : upub[i - 1];
}
// The refusals and the blocks every circuit against the index root shares.  inner(&update_cells, &shrink_cells) lays out the circuit's
// own blocks, with its own refusals, which come between the frame's: after the arguments', before the cell limit.  An audit has no block
// between the head and F: both counts stay 0, and the limit of its own cells is its own.
template <class Inner>
static int ann_frame_layout(size_t K, size_t cluster, size_t n_c, MkLayout* mw, AnnuBlocks* b, Inner inner) {
  VDB_ARG(K > 0 && K <= VDB_ANN_MAX_CLUSTERS, "K = 0 or K above VDB_ANN_MAX_CLUSTERS");
  VDB_ARG(cluster < K, "cluster >= K");
  VDB_ARG(n_c <= VDB_ANN_MAX_VECTORS, "cluster larger than VDB_ANN_MAX_VECTORS");
  uint64_t update_cells = 0, shrink_cells = 0;
  TRY(inner(&update_cells, &shrink_cells));
  mk_layout(1, K + 1, 1, mw);
  *b = annu_blocks(K, mw->total, update_cells, shrink_cells);
  VDB_ARG(b->total <= ((uint64_t)1 << 34), "more than VDB_MERKLE_UPDATE_MAX_CELLS cells in one call");
  return VDB_OK;
}
static int annu_layout(size_t K, size_t cluster, size_t n_c, size_t dim, size_t m, unsigned grow, AnnuLayout* o, MkuLayout* ml) {
  return ann_frame_layout(K, cluster, n_c, &o->mw, &o->b, [&](uint64_t* update_cells, uint64_t*) -> int {
    TRY(mku_layout(n_c, dim, m, nullptr, grow, ml, nullptr, nullptr, nullptr));
    *update_cells = ml->total;
    return VDB_OK;
  });
}
// The frame of one call: its work space in scratch slot 7, in u256: [c | words_old K + 1] (the header as it is assigned) | ind K |
// picked | words_new K + 1 | index_root_old, index_root_new | the inner block's public values n_upub | n_extra for the caller | the
// sponge states of D and of G.  open() attaches the inverse list to the streams and emits A - D; the caller emits its own blocks
// through `st`, then close() emits F and G over the new cluster root.
struct AnnFrame {
  Streams st;
  FpEntry* fp;
  const PoseidonSpec* sp;
  const MkLayout* mw;   // the sponge over K + 1 words, blocks D and G
  uint32_t K;
  u256 *hdr, *ind, *picked, *words_new, *iroot, *upub, *extra, *st_old, *st_new;
  // h: where the head's blocks start; total: the cells of the whole circuit
  int open(Streams streams, const u256* roots, size_t K_, size_t cluster, const AnnHead& h, const MkLayout& mw_, uint64_t total, size_t n_upub, size_t n_extra) {
    st = streams, mw = &mw_, K = (uint32_t)K_;
    const size_t n_st = (size_t)mw->nperm * PSD_T;
    hdr = (u256*)scratch_get(7, (2 * (K_ + 2) + K_ + 1 + 2 + n_upub + n_extra + 2 * n_st + 8) * sizeof(u256));
    if (!hdr) return VDB_ERR_OOM;
    ind = hdr + K_ + 2;
    picked = ind + K_;
    words_new = picked + 1;
    iroot = words_new + K_ + 1;
    upub = iroot + 2;
    extra = upub + n_upub;
    st_old = extra + n_extra;
    st_new = st_old + n_st;
    TRY(inv_list_attach(st, total));
    TRY(mk_begin(st, &fp, &sp));
    const uint32_t cu = (uint32_t)cluster;
    VDB_LAUNCH(k_annu_header, dim3((unsigned)((K_ + 2 + 255) / 256)), dim3(256), st, 0, cu, roots, K, hdr);
    VDB_LAUNCH(k_annu_indicator, dim3((unsigned)((K_ + 63) / 64)), dim3(64), st, fp->dev, h.b_ind, cu, K, ind);
    const NvMap sm{h.b_sel, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1u, K, 1u, 1u};
    VDB_LAUNCH(k_nv_select, dim3(1), dim3(64), st, fp->dev, sm, 1u, hdr + 2, ind, picked);
    return sponge(hdr + 1, h.b_old, st_old, iroot);
  }
  int close(const AnnuBlocks& b, const u256* new_root) {
    VDB_LAUNCH(k_annu_new_roots, dim3((unsigned)((K + 63) / 64)), dim3(64), st, fp->dev, b.b_new, K, new_root, hdr + 1, ind, words_new);
    return sponge(words_new, b.b_root, st_new, iroot + 1);
  }
  // the closing of a circuit that replaces word 0 and carries the K cluster roots over (the recentre): no block F, words_new =
  // [new centroids' root | the header's cluster roots], then G at b_root
  int close_word0(uint64_t b_root, const u256* new_croot) {
    VDB_HIP(hipMemcpyAsync(words_new, new_croot, sizeof(u256), hipMemcpyDeviceToDevice, ctx().stream));
    VDB_HIP(hipMemcpyAsync(words_new + 1, hdr + 2, K * sizeof(u256), hipMemcpyDeviceToDevice, ctx().stream));
    return sponge(words_new, b_root, st_new, iroot + 1);
  }
  // blocks D and G: the sponge over K + 1 words at `base`, its digest to *root
  int sponge(const u256* words, uint64_t base, u256* states, u256* root) {
    const uint32_t nperm = mw->nperm;
    TRY(mk_leaf_states(sp, words, 1u, K + 1, nperm, states, root, nullptr));
    VDB_LAUNCH(k_mk_leaf_trace, dim3((unsigned)((nperm + 63) / 64)), dim3(64), st, fp->dev, sp, words, 1u, K + 1, nperm, base, mw->leaf_cells, states,
               nullptr);
    return VDB_OK;
  }
};
// roots: [centroids_root | the K cluster roots] of the index before the batch; levels: cluster c's tree at depth d + grow, left in the
// state after the batch; pub: 3 m + 3
int wit_ann_update_dev(u256* levels, const u256* roots, size_t K, size_t cluster, size_t n_c, size_t dim, unsigned grow, const u256* new_vectors,
                       const uint64_t* indices, size_t m, Streams st, u256* pub) {
  static thread_local MkuPlan pl;
  AnnuLayout a;
  MkuLayout ml0;
  TRY(annu_layout(K, cluster, n_c, dim, m, grow, &a, &ml0));
  TRY(mku_plan(n_c, dim, grow, new_vectors, indices, nullptr, m, &pl));
  VDB_ARG(annu_track_fill(indices, m, n_c, pl.lp, nullptr, nullptr) == 0, "a write above the cluster's fill at its turn: the members of a cluster stay dense (append at the fill, or replace below it)");
  AnnFrame f;
  TRY(f.open(st, roots, K, cluster, a.b.h, a.mw, a.b.total, 3 * m + 2, 0));
  TRY(mku_emit(f.fp, f.sp, pl, levels, dim, new_vectors, f.st, a.b.b_upd, f.upub));
  TRY(f.close(a.b, f.upub + 3 * m + 1));
  VDB_LAUNCH(k_annu_public, dim3((unsigned)((3 * m + 3 + 255) / 256)), dim3(256), f.upub, f.hdr, f.iroot, (uint32_t)m, pub);
  return inv_list_fixup(f.st);
}

// ------------------------------------------------------------------ deletes against the index root (include/vdb.h vdb_wit_ann_delete,
// vdb_ann_index_remove_dev).  m deletes from cluster c: blocks A - D, F, G as above; E' is the update block over 2 m path updates (delete
// j: the last member's leaf carried into slot_j, then the last slot emptied: annd_expand), and when the cluster's tree halves s >= 1
// times block S between E' and F proves that the dropped half is empty: [S_0 assigned | Z_0 = load_constant(0) | Z_{l+1} = H(Z_l, Z_l),
// l < d - 1 | S_{i+1} = H(S_i, Z_{d-s+i}), i < s].  The map ties S_s to E's final root; F's `a` copies S_0, the root of the halved tree.

// Block S, a lane per permutation of its d - 1 + s node hashes, in the form of k_mku_grow_trace; every input is resident: Z_l in `empty`,
// S_i at entry 0 of level d - s + i of `levels` once k_mku_writeback has run.  Lane 0 also assigns S_0 and keeps it for block F.
__global__ __launch_bounds__(64) void k_annd_shrink_trace(Streams stq, const FpTables* __restrict__ T, const PoseidonSpec* __restrict__ sp, uint64_t base,
                                                          uint32_t depth, uint32_t shrink, uint64_t lp, const u256* __restrict__ levels,
                                                          const u256* __restrict__ empty, u256* __restrict__ s0) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  const uint32_t n_z = depth - 1, n_hash = n_z + shrink, d1 = depth - shrink;
  if (t >= 2 * n_hash) return;
  if (t == 0) {
    const u256 v = levels[mku_level_off(lp, d1)];
    *s0 = v;
    WCtx c = make_ctx(stq, T, base, 0);
    c.push(v, false);
    c.push(u256_zero(), false, true);
  }
  const uint32_t h = t >> 1, second = t & 1u;
  const uint32_t lz = h < n_z ? h : d1 + (h - n_z);
  trace_node_half(stq, T, sp, base + 2 + (uint64_t)h * NODE_CELLS, h < n_z ? empty + lz : levels + mku_level_off(lp, lz), empty + lz, second);
}
// [index_root_old | c | slot_j, removed_leaf_j, last_j, moved_leaf_j per delete | index_root_new] from the update block's public values
// [old root | idx, old leaf, new leaf per path update | new root]: delete j is updates 2 j (the move) and 2 j + 1 (the emptied slot)
__global__ __launch_bounds__(256) void k_annd_public(const u256* __restrict__ upub, const u256* __restrict__ hdr, const u256* __restrict__ iroot,
                                                     uint32_t m, u256* __restrict__ pub) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 4 * m + 3) return;
  if (i < 2 || i == 4 * m + 2) {
    pub[i] = i == 0 ? iroot[0] : i == 1 ? hdr[0] : iroot[1];
    return;
  }
  const uint32_t j = (i - 2) >> 2, k = (i - 2) & 3u;
  pub[i] = upub[1 + 6 * (size_t)j + (k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 3 : 2)];
}
// the host side of a delete batch, before anything is launched: the expansion to 2 m path updates and every refusal
static int annd_layout(size_t K, size_t cluster, size_t n_c, size_t dim, const uint64_t* slots, size_t m, AnnuLayout* o, MkuLayout* ml, AnndPlan* dp) {
  return ann_frame_layout(K, cluster, n_c, &o->mw, &o->b, [&](uint64_t* update_cells, uint64_t* shrink_cells) -> int {
    VDB_ARG(m > 0 && m <= MKU_MAX_UPDATES / 2, "a batch holds 1 .. VDB_MERKLE_UPDATE_MAX_UPDATES / 2 deletes (two path updates each)");
    VDB_ARG(m < n_c, "the batch would empty the cluster");
    static thread_local std::vector<uint64_t> none;
    if (!slots) {   // the size call: the shape does not depend on the slots
      none.assign(m, 0);
      slots = none.data();
    }
    const int rc = annd_expand(slots, m, n_c, MKU_MAX_UPDATES, dp, nullptr);
    VDB_ARG(rc != 3, "a slot at or above the cluster's fill at its turn (every delete lowers the fill by one)");
    VDB_ARG(rc == 0, "a batch holds at least one delete and leaves at least one member");
    *shrink_cells = annd_shrink_cells(dp->depth, dp->shrink, NODE_CELLS);
    TRY(mku_layout(n_c, dim, 2 * m, dp->kinds.data(), 0, ml, nullptr, nullptr, nullptr, true));
    *update_cells = ml->total;
    return VDB_OK;
  });
}
// roots: [centroids_root | the K cluster roots] of the index before the batch; levels: cluster c's tree over its n_c members, left in
// the state after the batch (at its old size: vdb_ann_index_remove_dev cuts it); pub: 4 m + 3
int wit_ann_delete_dev(u256* levels, const u256* roots, size_t K, size_t cluster, size_t n_c, size_t dim, const uint64_t* slots, size_t m, Streams st,
                       u256* pub) {
  static thread_local MkuPlan pl;
  static thread_local AnndPlan dp;
  AnnuLayout a;
  MkuLayout ml0;
  VDB_ARG(slots, "null pointer");
  TRY(annd_layout(K, cluster, n_c, dim, slots, m, &a, &ml0, &dp));
  TRY(mku_plan(n_c, dim, 0, nullptr, dp.indices.data(), dp.kinds.data(), 2 * m, &pl, dp.carry_src.data()));
  const u256* empty = nullptr;
  if (dp.shrink) TRY(poseidon_empty_subtrees_dev(&empty));
  const size_t n_up = 6 * m + 2;
  AnnFrame f;
  TRY(f.open(st, roots, K, cluster, a.b.h, a.mw, a.b.total, n_up, 1));
  u256* s0 = f.extra;
  TRY(mku_emit(f.fp, f.sp, pl, levels, dim, nullptr, f.st, a.b.b_upd, f.upub));
  if (dp.shrink)  // S_i are the halved tree's top digests as the write-back left them
    VDB_LAUNCH(k_annd_shrink_trace, dim3((unsigned)((2 * (dp.depth - 1 + dp.shrink) + 63) / 64)), dim3(64), f.st, f.fp->dev, f.sp, a.b.b_shr, dp.depth, dp.shrink,
               pl.lp, levels, empty, s0);
  TRY(f.close(a.b, dp.shrink ? s0 : f.upub + n_up - 1));
  VDB_LAUNCH(k_annd_public, dim3((unsigned)((4 * m + 3 + 255) / 256)), dim3(256), f.upub, f.hdr, f.iroot, (uint32_t)m, pub);
  return inv_list_fixup(f.st);
}

// ------------------------------------------------------------------ moves from one cluster to another (include/vdb.h vdb_wit_ann_move,
// vdb_ann_index_move_dev).  m members pass from cluster a to cluster b in one circuit, index_root_old to index_root_new:
// A [a | b | centroids_root | cluster roots], B_a, C_a -> picked_a, D the old sponge, E' and S the delete's blocks on a's tree, F_a
// mid_j = select(a's new root, cluster_root_j, ind_a_j), B_b, C_b over mid -> picked_b, E_b the update block on b's grown tree: m appends
// whose new leaf is carried from a (the removed leaf of delete j), F_b out_j = select(b's new root, mid_j, ind_b_j), G the new sponge.
// The composition is sequential: b's root is picked from mid, the roots after the removal.
struct AnnMoveLayout {
  MkLayout mw;
  AnnMoveBlocks b;
  MkuLayout ma, mb;
};
// the header: lane i < K + 3 assigns cell i and keeps the value for the blocks that read it
__global__ __launch_bounds__(256) void k_annmv_header(Streams st, uint32_t a, uint32_t b, const u256* __restrict__ roots, uint32_t K,
                                                      u256* __restrict__ hdr) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K + 3) return;
  const u256 v = i >= 2 ? roots[i - 2] : Gadgets::mont_small(i ? b : a);
  hdr[i] = v;
  if (i < st.rlo || i >= st.rhi) return;
  st.adv[i] = v;
  if (st.sel) st.sel[i] = 0;
}
// [index_root_old | a | b | slot_j, leaf_j, last_j, moved_leaf_j, dest_j, dest_old_leaf_j per move | index_root_new] from the two update
// blocks' public rows [old root | idx, old leaf, new leaf per path update | new root]: move j is updates 2 j and 2 j + 1 of a's, update j of b's
__global__ __launch_bounds__(256) void k_annmv_public(const u256* __restrict__ upa, const u256* __restrict__ upb, const u256* __restrict__ hdr,
                                                      const u256* __restrict__ iroot, uint32_t m, u256* __restrict__ pub) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 6 * m + 4) return;
  if (i < 3 || i == 6 * m + 3) {
    pub[i] = i == 0 ? iroot[0] : i < 3 ? hdr[i - 1] : iroot[1];
    return;
  }
  const uint32_t j = (i - 3) / 6, k = (i - 3) % 6;
  pub[i] = k < 4 ? upa[1 + 6 * (size_t)j + (k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 3 : 2)] : upb[1 + 3 * (size_t)j + (k - 4)];
}
// the host side of a move batch, before anything is launched: the expansion to 2 m + m path updates and every refusal.  grow < 0: the
// call computes it; slots null (the size call): the shape does not depend on them
static int annmv_layout(size_t K, size_t a, size_t b, size_t n_a, size_t n_b, int grow, const uint64_t* slots, size_t m, AnnMoveLayout* o, AnnMovePlan* mp) {
  VDB_ARG(K >= 2 && K <= VDB_ANN_MAX_CLUSTERS, "K below 2 (a move needs two clusters) or K above VDB_ANN_MAX_CLUSTERS");
  VDB_ARG(a < K && b < K, "cluster >= K");
  VDB_ARG(a != b, "a move goes to another cluster: src == dst");
  VDB_ARG(n_a <= VDB_ANN_MAX_VECTORS && n_b <= VDB_ANN_MAX_VECTORS, "cluster larger than VDB_ANN_MAX_VECTORS");
  VDB_ARG(m > 0 && m <= MKU_MAX_UPDATES / 2, "a batch holds 1 .. VDB_MERKLE_UPDATE_MAX_UPDATES / 2 moves (two path updates of the source each)");
  VDB_ARG(m < n_a, "the batch would empty the source cluster");
  static thread_local std::vector<uint64_t> none;
  if (!slots) {
    none.assign(m, 0);
    slots = none.data();
  }
  const int rc = annmv_expand(slots, m, n_a, n_b, grow, MKU_MAX_UPDATES, mp, nullptr);
  VDB_ARG(rc != 3, "a slot at or above the source cluster's fill at its turn (every move lowers the fill by one)");
  VDB_ARG(rc != 4, "empty destination cluster");
  VDB_ARG(rc != 5, "grow is the smallest number of doublings after which the destination's tree holds its new members");
  VDB_ARG(rc == 0, "a batch holds at least one move and leaves at least one member");
  TRY(mku_layout(n_a, 1, 2 * m, mp->d.kinds.data(), 0, &o->ma, nullptr, nullptr, nullptr, true));
  TRY(mku_layout(n_b, 1, m, mp->kinds.data(), mp->grow, &o->mb, nullptr, nullptr, nullptr, true));
  mk_layout(1, K + 1, 1, &o->mw);
  o->b = annmv_blocks(K, o->mw.total, o->ma.total, annd_shrink_cells(mp->d.depth, mp->d.shrink, NODE_CELLS), o->mb.total);
  VDB_ARG(o->b.total <= ((uint64_t)1 << 34), "more than VDB_MERKLE_UPDATE_MAX_CELLS cells in one call");
  return VDB_OK;
}
// roots: [centroids_root | the K cluster roots] of the index before the batch; levels_a: a's tree over its n_a members, left in the
// state after the batch at its old size; levels_b: b's tree at depth d_b + g, left in the state after the batch; pub: 6 m + 4.
// The two update blocks take the plan's work space (scratch slot 0) and its one table upload one after the other in stream order: the
// second block's upload and kernels are queued behind the first block's last kernel, which has read the first table by then.  What the
// second block needs of the first, the removed leaves, lies in the first block's public row in the frame's own slot.
int wit_ann_move_dev(u256* levels_a, u256* levels_b, const u256* roots, size_t K, size_t a, size_t b, size_t n_a, size_t n_b, int grow,
                     const uint64_t* slots, size_t m, Streams st, u256* pub) {
  static thread_local MkuPlan pa, pb;
  static thread_local AnnMovePlan mp;
  static thread_local std::vector<uint32_t> carry;
  AnnMoveLayout L;
  VDB_ARG(slots, "null pointer");
  TRY(annmv_layout(K, a, b, n_a, n_b, grow, slots, m, &L, &mp));
  const size_t n_upa = 6 * m + 2, n_upb = 3 * m + 2;
  TRY(mku_plan(n_a, 1, 0, nullptr, mp.d.indices.data(), mp.d.kinds.data(), 2 * m, &pa, mp.d.carry_src.data()));
  carry.resize(m);
  for (size_t j = 0; j < m; j++) carry[j] = (uint32_t)(2 + 6 * j);   // the old leaf of a's update 2 j in a's public row: the removed leaf
  TRY(mku_plan(n_b, 1, mp.grow, nullptr, mp.dest.data(), mp.kinds.data(), m, &pb, carry.data(), n_upa));
  const u256* empty = nullptr;
  if (mp.d.shrink) TRY(poseidon_empty_subtrees_dev(&empty));
  const AnnMoveBlocks& B = L.b;
  AnnFrame f;   // its sponge and its fields; the head is laid out here: two indicator blocks, K + 3 header cells
  f.st = st, f.mw = &L.mw, f.K = (uint32_t)K;
  const size_t n_st = (size_t)L.mw.nperm * PSD_T;
  f.hdr = (u256*)scratch_get(7, (K + 3 + 2 * K + 2 + 2 * (K + 1) + 2 + n_upa + n_upb + 1 + 2 * n_st + 8) * sizeof(u256));
  if (!f.hdr) return VDB_ERR_OOM;
  u256 *ind_a = f.hdr + K + 3, *ind_b = ind_a + K, *picked = ind_b + K, *words_mid = picked + 2, *words_new = words_mid + K + 1;
  f.iroot = words_new + K + 1;
  u256 *upa = f.iroot + 2, *upb = upa + n_upa, *s0 = upb + n_upb;
  f.st_old = s0 + 1;
  f.st_new = f.st_old + n_st;
  TRY(inv_list_attach(f.st, B.total));
  TRY(mk_begin(f.st, &f.fp, &f.sp));
  const uint32_t Ku = (uint32_t)K;
  const u256* words_old = f.hdr + 2;
  VDB_LAUNCH(k_annmv_header, dim3((unsigned)((K + 3 + 255) / 256)), dim3(256), f.st, (uint32_t)a, (uint32_t)b, roots, Ku, f.hdr);
  VDB_LAUNCH(k_annu_indicator, dim3((unsigned)((K + 63) / 64)), dim3(64), f.st, f.fp->dev, B.b_ind_a, (uint32_t)a, Ku, ind_a);
  const NvMap sa{B.b_sel_a, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1u, Ku, 1u, 1u};
  VDB_LAUNCH(k_nv_select, dim3(1), dim3(64), f.st, f.fp->dev, sa, 1u, words_old + 1, ind_a, picked);
  TRY(f.sponge(words_old, B.b_old, f.st_old, f.iroot));
  TRY(mku_emit(f.fp, f.sp, pa, levels_a, 1, nullptr, f.st, B.b_upd_a, upa));
  if (mp.d.shrink)
    VDB_LAUNCH(k_annd_shrink_trace, dim3((unsigned)((2 * (mp.d.depth - 1 + mp.d.shrink) + 63) / 64)), dim3(64), f.st, f.fp->dev, f.sp, B.b_shr, mp.d.depth,
               mp.d.shrink, pa.lp, levels_a, empty, s0);
  VDB_LAUNCH(k_annu_new_roots, dim3((unsigned)((K + 63) / 64)), dim3(64), f.st, f.fp->dev, B.b_mid, Ku, mp.d.shrink ? s0 : upa + n_upa - 1, words_old, ind_a,
             words_mid);
  VDB_LAUNCH(k_annu_indicator, dim3((unsigned)((K + 63) / 64)), dim3(64), f.st, f.fp->dev, B.b_ind_b, (uint32_t)b, Ku, ind_b);
  const NvMap sb{B.b_sel_b, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1u, Ku, 1u, 1u};
  VDB_LAUNCH(k_nv_select, dim3(1), dim3(64), f.st, f.fp->dev, sb, 1u, words_mid + 1, ind_b, picked + 1);
  TRY(mku_emit(f.fp, f.sp, pb, levels_b, 1, nullptr, f.st, B.b_upd_b, upb, upa));
  VDB_LAUNCH(k_annu_new_roots, dim3((unsigned)((K + 63) / 64)), dim3(64), f.st, f.fp->dev, B.b_new, Ku, upb + n_upb - 1, words_mid, ind_b, words_new);
  TRY(f.sponge(words_new, B.b_root, f.st_new, f.iroot + 1));
  VDB_LAUNCH(k_annmv_public, dim3((unsigned)((6 * m + 4 + 255) / 256)), dim3(256), upa, upb, f.hdr, f.iroot, (uint32_t)m, pub);
  return inv_list_fixup(f.st);
}

// ------------------------------------------------------------------ linked writes: one batch through the cluster's tree and the database
// tree (include/vdb.h vdb_wit_ann_write, vdb_ann_index_write_dev).  m inserts or replacements into cluster c in one circuit,
// (database_root_old, index_root_old) to (database_root_new, index_root_new): blocks A - D, E, F, G are the update's above, cell for cell;
// E_db between E and F is the update block on the database tree at dim 1 with grow g_db: update j at db_idx_j, its new leaf CARRIED from
// E (the digest E's leaf sponge j squeezed, entry 3 + 3 j of E's public row), so every vector is hashed once.
struct AnnwLayout {
  MkLayout mw;
  AnnwBlocks b;
  MkuLayout me, mdb;
};
// [database_root_old | index_root_old | c | idx_j, db_idx_j, old_leaf_j, new_leaf_j per write | database_root_new | index_root_new] from
// the two blocks' public rows [old root | idx, old leaf, new leaf per update | new root], the header and the two index roots
__global__ __launch_bounds__(256) void k_annw_public(const u256* __restrict__ upub, const u256* __restrict__ updb, const u256* __restrict__ hdr,
                                                     const u256* __restrict__ iroot, uint32_t m, u256* __restrict__ pub) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 4 * m + 5) return;
  if (i < 3 || i >= 4 * m + 3) {
    pub[i] = i == 0 ? updb[0] : i == 1 ? iroot[0] : i == 2 ? hdr[0] : i == 4 * m + 3 ? updb[3 * (size_t)m + 1] : iroot[1];
    return;
  }
  const uint32_t j = (i - 3) / 4, k = (i - 3) % 4;
  pub[i] = k == 1 ? updb[1 + 3 * (size_t)j] : upub[1 + 3 * (size_t)j + (k ? k - 1 : 0)];
}
// the host side of a linked write, before anything is launched: the layout of both blocks and every refusal.  indices null (the size
// call): the batch is `appends` appends followed by replacements of slot 0, which has the shape of every batch with as many appends.
// db_slots (null: unknown): the cluster's n_c database slots; db_indices (null: the expansion's own, which needs db_slots).  grow_db < 0:
// the call computes it
static int annw_layout(size_t K, size_t cluster, size_t n_c, size_t n_db, size_t dim, unsigned grow_c, int grow_db, const uint64_t* indices, uint64_t appends,
                       const uint64_t* db_slots, const uint64_t* db_indices, size_t m, AnnwLayout* o, AnnwPlan* wp) {
  static thread_local std::vector<uint64_t> shape_idx, shape_db;
  static thread_local std::vector<uint8_t> kinds;
  TRY(ann_frame_layout(K, cluster, n_c, &o->mw, &o->b.u, [&](uint64_t* update_cells, uint64_t* second_cells) -> int {
    TRY(mku_layout(n_c, dim, m, nullptr, grow_c, &o->me, nullptr, nullptr, nullptr));
    VDB_ARG(n_db > 0, "empty database");
    VDB_ARG(n_c <= n_db && n_db <= VDB_ANN_MAX_VECTORS, "a cluster larger than its database, or n_db above VDB_ANN_MAX_VECTORS");
    if (!indices) {
      VDB_ARG(appends <= m, "more appends than writes");
      shape_idx.resize(m);
      shape_db.resize(m);
      for (size_t j = 0; j < m; j++) shape_idx[j] = j < appends ? n_c + j : 0, shape_db[j] = j < appends ? n_db + j : 0;
      indices = shape_idx.data(), db_indices = shape_db.data(), db_slots = nullptr;
    }
    uint64_t lp, track = 0;
    uint32_t d;
    tree_shape(n_c, &lp, &d);
    VDB_ARG(annu_track_fill(indices, m, n_c, lp << grow_c, &track, nullptr) == 0,
            "a write above the cluster's fill at its turn or outside the grown tree: the members of a cluster stay dense");
    const int rc = annw_expand(db_slots, indices, m, n_c, n_db, db_indices, grow_db, wp, nullptr);
    VDB_ARG(rc != 1, "a write above the cluster's fill at its turn");
    VDB_ARG(rc != 2, "empty database, or a cluster larger than its database");
    VDB_ARG(rc != 3, "a member's database slot at or above n_db");
    VDB_ARG(rc != 4, "a database slot the batch does not yield: an append goes to the database's fill at its turn, a replacement below it");
    VDB_ARG(rc == 0, "grow_db is the smallest number of doublings after which the database tree holds the appends");
    kinds.assign(m, 2);
    TRY(mku_layout(n_db, 1, m, kinds.data(), wp->grow_db, &o->mdb, nullptr, nullptr, nullptr, true));
    *update_cells = o->me.total;
    *second_cells = o->mdb.total;   // (E_db lies where the delete has its block S: annw_blocks)
    return VDB_OK;
  }));
  o->b = annw_blocks(K, m, o->mw.total, o->me.total, o->mdb.total);
  return VDB_OK;
}
// roots: [centroids_root | the K cluster roots] of the index before the batch; levels_c: cluster c's tree at depth d_c + g_c, levels_db:
// the database tree at depth d_db + g_db (merkle_tree_grow_dev's when grown), both left in the state after the batch; pub: 4 m + 5.
// The two update blocks take the plan's work space (scratch slot 0) and its one table upload one after the other in stream order, as
// wit_ann_move_dev: E_db's upload and kernels are queued behind E's last kernel, which has read E's table by then and has written E's
// public row, where E_db's carried leaves name their digests.
int wit_ann_write_dev(u256* levels_c, u256* levels_db, const u256* roots, size_t K, size_t cluster, size_t n_c, size_t n_db, size_t dim, unsigned grow_c,
                      int grow_db, const u256* new_vectors, const uint64_t* indices, const uint64_t* db_indices, size_t m, Streams st, u256* pub) {
  static thread_local MkuPlan pe, pdb;
  static thread_local AnnwPlan wp;
  static thread_local std::vector<uint32_t> carry;
  static thread_local std::vector<uint8_t> kinds;
  AnnwLayout L;
  VDB_ARG(indices && db_indices, "null pointer");
  TRY(annw_layout(K, cluster, n_c, n_db, dim, grow_c, grow_db, indices, 0, nullptr, db_indices, m, &L, &wp));
  const size_t n_up = 3 * m + 2;
  TRY(mku_plan(n_c, dim, grow_c, new_vectors, indices, nullptr, m, &pe));
  carry.resize(m);
  kinds.assign(m, 2);
  for (size_t j = 0; j < m; j++) carry[j] = (uint32_t)(3 + 3 * j);   // the new leaf of E's update j in E's public row
  TRY(mku_plan(n_db, 1, wp.grow_db, nullptr, wp.db_idx.data(), kinds.data(), m, &pdb, carry.data(), n_up));
  const AnnuBlocks& B = L.b.u;
  AnnFrame f;
  TRY(f.open(st, roots, K, cluster, B.h, L.mw, B.total, n_up, n_up));
  TRY(mku_emit(f.fp, f.sp, pe, levels_c, dim, new_vectors, f.st, B.b_upd, f.upub));
  TRY(mku_emit(f.fp, f.sp, pdb, levels_db, 1, nullptr, f.st, L.b.b_upd_db, f.extra, f.upub));
  TRY(f.close(B, f.upub + n_up - 1));
  VDB_LAUNCH(k_annw_public, dim3((unsigned)((4 * m + 5 + 255) / 256)), dim3(256), f.upub, f.extra, f.hdr, f.iroot, (uint32_t)m, pub);
  return inv_list_fixup(f.st);
}

// ------------------------------------------------------------------ the cluster frame of the routing audit and the mean audit below: blocks
// A - D are the frame's head; I [centroids | members] assigned; the audit's own blocks; MC, MM the two merkle_commitments, whose roots the
// map ties to the header's centroids_root and to picked.  pub: [index_root | c].  Nothing after the head is AnnFrame's: close() is not called.
struct AnnClusterLayout { MkLayout mw, mc, mm; };
// the refusals, in the frame's order: the arguments', own() with the audit's, the frame's cell limit; the audit's own limit comes behind them
template <class Own>
static int ann_cluster_layout(size_t K, size_t cluster, size_t n_c, size_t dim, AnnClusterLayout* t, Own own) {
  AnnuBlocks frame;   // F and G over no block at all: asked for the cell limit alone
  TRY(ann_frame_layout(K, cluster, n_c, &t->mw, &frame, [&](uint64_t*, uint64_t*) -> int {
    VDB_ARG(n_c > 0 && dim > 0 && dim <= ((size_t)1 << 20), "empty cluster, dim = 0 or dim above 2^20");
    return own();
  }));
  mk_layout_pair(K, n_c, dim, &t->mc, &t->mm);
  return VDB_OK;
}
// One call's frame: open() emits the head and block I, the audit emits its own blocks through f.st, finish() emits MC and MM and the
// public values.  levels_c / levels_m: the two trees where they are resident (forest segments K and c), or both null.
struct AnnClusterFrame {
  AnnFrame f;
  FpEntry* fp;   // the tables of (P, L); f.fp is the head's
  const AnnClusterLayout* t;
  const AnnCluster* b;
  const u256 *centroids, *members;
  size_t K, n_c, dim;
  int open(Streams st, FpEntry* fp_, const u256* centroids_, const u256* members_, const u256* roots, size_t K_, size_t cluster, size_t n_c_, size_t dim_,
           const AnnClusterLayout& lay, const AnnCluster& blocks, size_t n_extra) {
    fp = fp_, t = &lay, b = &blocks, centroids = centroids_, members = members_, K = K_, n_c = n_c_, dim = dim_;
    TRY(f.open(st, roots, K, cluster, b->h, t->mw, b->total, 0, n_extra));
    TRY(set_winv(f.st, fp->dev));   // the head's gadgets are GateChip's alone; the audit's own read the tables of (P, L)
    VDB_LAUNCH(k_mku_inputs, dim3((unsigned)(((K + n_c) * dim + 255) / 256)), dim3(256), f.st, b->b_in, centroids, members, (uint64_t)(K * dim),
               (uint64_t)((K + n_c) * dim));
    return VDB_OK;
  }
  int finish(const u256* levels_c, const u256* levels_m, u256* pub) {
    const bool resident = levels_c && levels_m;
    TRY(mk_emit(fp, f.sp, centroids, K, dim, t->mc, f.st, b->b_mc, resident ? levels_c : nullptr, nullptr));
    TRY(mk_emit(fp, f.sp, members, n_c, dim, t->mm, f.st, b->b_mm, resident ? levels_m : nullptr, nullptr));
    VDB_HIP(hipMemcpyAsync(pub, f.iroot, sizeof(u256), hipMemcpyDeviceToDevice, ctx().stream));
    VDB_HIP(hipMemcpyAsync(pub + 1, f.hdr, sizeof(u256), hipMemcpyDeviceToDevice, ctx().stream));
    return inv_list_fixup(f.st);
  }
};

// ------------------------------------------------------------------ the audit of one cluster's routing (include/vdb.h vdb_wit_ann_audit):
// every member committed under cluster_root_c is at least as close to centroid c as to any other committed centroid.  Its own block in
// the cluster frame: R per member i the K distance(centroid_j, member_i), the qmin chain -> m_i and select_by_indicator(d_i0 .., ind) ->
// own_i, which the map ties to m_i.
struct AnnaLayout {
  AnnClusterLayout t;
  DistLayout dl;
  AnnaBlocks b;
};
// select_by_indicator([d_i0 .. d_i,K-1], ind) per member, lanes = (member i, j), j fastest.  ind is one-hot at c, so the running value
// is known without a walk: s_j = j >= c ? d_ic : 0, and lane (i, j) pushes [d_ij, ind_j, s_j] at 1 + 3 j of member i's block, lane
// (i, 0) the leading 0 as well (k_nv_select's cells and flags for the same gadget).  Lane (i, 0) also states whether member i is routed:
// d_ic is the chain's minimum.
__global__ __launch_bounds__(64) void k_anna_pick(Streams st, const FpTables* __restrict__ T, uint64_t base, uint64_t per_member, uint32_t c, uint32_t K,
                                                  uint32_t n_c, const u256* __restrict__ dist, const u256* __restrict__ pm,
                                                  uint8_t* __restrict__ routed) {
  const uint64_t th = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (th >= (uint64_t)n_c * K) return;
  const uint32_t j = (uint32_t)(th % K), i = (uint32_t)(th / K);
  const u256* di = dist + (size_t)i * K;
  const u256 own = di[c];
  if (j == 0) routed[i] = u256_eq(own, pm[(size_t)i * K + K - 1]) ? 1 : 0;
  WCtx cx = make_ctx(st, T, base + (uint64_t)i * per_member + (j ? 1 + 3ull * j : 0), 0);
  if (j == 0) cx.push(u256_zero(), true);
  cx.push(di[j], false);
  cx.push(j == c ? mont_one<Fr>() : u256_zero(), false);
  cx.push(j >= c ? own : u256_zero(), j + 1 < K);
}
// the refusals, in the frame's order, and where the blocks start
static int anna_layout(FpEntry* fp, int metric, size_t K, size_t cluster, size_t n_c, size_t dim, AnnaLayout* o) {
  TRY(ann_cluster_layout(K, cluster, n_c, dim, &o->t, [&]() -> int {
    const size_t cap = VDB_NEAREST_TOPK_MAX_INSTANCES;
    VDB_ARG(K <= cap / n_c && dim <= cap / n_c, "audit too large: n_c * K and n_c * dim at most VDB_NEAREST_TOPK_MAX_INSTANCES");
    return dist_layout(fp->host, metric, dim, &o->dl);
  }));
  o->b = anna_blocks(K, n_c, dim, o->t.mw.total, o->dl.total_cells, o->dl.total_lk, fp->host.sz.qmin[0], fp->host.sz.qmin[1], o->t.mc.total, o->t.mm.total);
  VDB_ARG(o->b.f.total <= VDB_NEAREST_TOPK_MAX_CELLS, "audit circuit above 2^34 cells");
  return VDB_OK;
}
// roots: [centroids_root | the K cluster roots]; routed: n_c bytes; the rest as AnnClusterFrame has it.  Scratch slot 0 holds the distances
// and the prefix minima until k_anna_pick has read them, and mk_emit asks for the slot again: every launch of R is enqueued before
// finish(), whose first mk_emit is the next to take the slot (the stream orders them).
int wit_ann_audit_dev(FpEntry* fp, int metric, const u256* centroids, const u256* members, const u256* roots, const u256* levels_c, const u256* levels_m,
                      size_t K, size_t cluster, size_t n_c, size_t dim, Streams st, uint8_t* routed, u256* pub) {
  AnnaLayout a;
  TRY(anna_layout(fp, metric, K, cluster, n_c, dim, &a));
  const AnnaBlocks& b = a.b;
  const size_t inst = n_c * K;
  u256* mid = (u256*)scratch_get(0, (inst * 5 + 8) * sizeof(u256) + inst * sizeof(uint32_t));
  if (!mid) return VDB_ERR_OOM;
  u256 *dist = mid + 3 * inst, *pm = dist + inst;
  uint32_t* rnd = (uint32_t*)(pm + inst + 8);
  AnnClusterFrame cf;
  TRY(cf.open(st, fp, centroids, members, roots, K, cluster, n_c, dim, a.t, b.f, 0));
  const InstMap im{b.f.b_own, 0, (uint32_t)K, b.per_member, b.per_member_l, (uint32_t)K, (uint32_t)K};   // t = i K + j: (centroid_j, member_i)
  TRY(run_distances(cf.f.st, fp, a.dl, im, (uint32_t)inst, centroids, members, mid, dist));
  VDB_LAUNCH(k_nv_rounds, dim3((unsigned)n_c), dim3(64), fp->dev, dist, (uint32_t)K, 1u, pm, rnd);
  const NvMap nm{b.f.b_own, 0, b.per_member, b.per_member_l, b.chain_off, b.chain_loff, 0, 0, 0, 0, 0, (uint32_t)n_c, (uint32_t)K, (uint32_t)dim, 1u};
  VDB_LAUNCH(k_nv_qmin, dim3((unsigned)((n_c * (K - 1) + 63) / 64 + (K == 1))), dim3(64), cf.f.st, fp->dev, nm, dist, pm, rnd);
  VDB_LAUNCH(k_anna_pick, dim3((unsigned)((inst + 63) / 64)), dim3(64), cf.f.st, fp->dev, b.f.b_own + b.pick_off, b.per_member, (uint32_t)cluster, (uint32_t)K,
             (uint32_t)n_c, dist, pm, routed);
  return cf.finish(levels_c, levels_m, pub);
}

// ------------------------------------------------------------------ the mean audit of one cluster (include/vdb.h vdb_wit_ann_mean):
// word for word, centroid c is qdiv(sum of the members committed under cluster_root_c, quantization(n_c)).  Its own blocks in the cluster
// frame: S select_by_indicator(centroids, ind) -> own (k_nv_select over the K centroids, a lane per word); M the constant len, the qadd
// chains and the dim qdiv, whose outputs the map ties to own.
struct AnnmLayout {
  AnnClusterLayout t;
  AnnmBlocks b;
};
// the refusals, in the frame's order, and where the blocks start
static int annm_layout(FpEntry* fp, size_t K, size_t cluster, size_t n_c, size_t dim, AnnmLayout* o) {
  TRY(ann_cluster_layout(K, cluster, n_c, dim, &o->t, [&]() -> int {
    const size_t cap = VDB_NEAREST_TOPK_MAX_INSTANCES;
    VDB_ARG(K <= cap / dim && n_c <= cap / dim, "mean audit too large: K * dim and n_c * dim at most VDB_NEAREST_TOPK_MAX_INSTANCES");
    // qdiv's divisor is asserted below 2^(2P) (r_div_mod_var(ar, ba, 4P, 2P, ..) in fp_qdiv_emit__body): quantization(n_c) = n_c 2^P
    VDB_ARG(fp->host.P >= 63 || n_c < ((uint64_t)1 << fp->host.P), "n_c not below 2^P: quantization(n_c) would not pass qdiv's divisor bound 2^(2P)");
    return VDB_OK;
  }));
  o->b = annm_blocks(K, n_c, dim, o->t.mw.total, fp->host.sz.qdiv[0], fp->host.sz.qdiv[1], o->t.mc.total, o->t.mm.total);
  VDB_ARG(o->b.f.total <= VDB_NEAREST_TOPK_MAX_CELLS, "mean audit circuit above 2^34 cells");
  return VDB_OK;
}
// roots: [centroids_root | the K cluster roots]; mean_ok: dim bytes; the rest as AnnClusterFrame has it.  own and the chain totals live in
// the frame's work space (`extra`, scratch slot 7), not in slot 0, which mk_emit asks for: S and M are still enqueued before finish() and
// its first mk_emit, the order the audit documents.
int wit_ann_mean_dev(FpEntry* fp, const u256* centroids, const u256* members, const u256* roots, const u256* levels_c, const u256* levels_m, size_t K,
                     size_t cluster, size_t n_c, size_t dim, Streams st, uint8_t* mean_ok, u256* pub) {
  AnnmLayout a;
  TRY(annm_layout(fp, K, cluster, n_c, dim, &a));
  const AnnmBlocks& b = a.b;
  AnnClusterFrame cf;
  TRY(cf.open(st, fp, centroids, members, roots, K, cluster, n_c, dim, a.t, b.f, 2 * dim));
  const AnnFrame& f = cf.f;
  u256 *own = f.extra, *sums = own + dim;
  const NvMap sm{b.b_s, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1u, (uint32_t)K, (uint32_t)dim, 1u};
  VDB_LAUNCH(k_nv_select, dim3((unsigned)((dim + 63) / 64)), dim3(64), f.st, fp->dev, sm, 1u, centroids, f.ind, own);
  const u256 len = fr_mul(to_mont<Fr>(u256_from_u64(n_c)), fp->host.scale);   // load_constant(quantization(n_c))
  VDB_LAUNCH(k_push_cells, dim3(1), dim3(1), f.st, b.b_m, len, len, 1u);
  VDB_LAUNCH(k_annm_sum, dim3((unsigned)dim), dim3(64), f.st, fp->dev, b.b_chain, (uint32_t)n_c, (uint32_t)dim, members, sums);
  VDB_LAUNCH(k_annm_div, dim3((unsigned)((dim + 63) / 64), 8), dim3(64), f.st, fp->dev, b.b_div, (uint32_t)dim, sums, len, own, mean_ok);
  return cf.finish(levels_c, levels_m, pub);
}

// ------------------------------------------------------------------ the recentre of one cluster (include/vdb.h vdb_wit_ann_recentre):
// the index under index_root_new has the K cluster roots of the index under index_root_old, and its centroids' tree is the old one with
// leaf c replaced by the leaf of qdiv(sum of the members committed under cluster_root_c, quantization(n_c)).  Blocks: A - D the frame's
// head; I the members assigned; M the mean audit's (len, the qadd chains, one qdiv per word -> mean_j); MM merkle_commitment(members),
// tied to picked; U the update block of the centroids' tree with the one write (idx tied to c, its new vector to mean_j, its old root
// to the header's centroids_root); G the sponge over [U's new root | the header's cluster roots].  The old centroid is never assigned.
struct AnnrLayout {
  MkLayout mw, mm;
  MkuLayout mu;
  AnnrBlocks b;
};
// the refusals, in the frame's order (the mean audit's and mku_layout's between the frame's), and where the blocks start
static int annr_layout(FpEntry* fp, size_t K, size_t cluster, size_t n_c, size_t dim, AnnrLayout* o) {
  AnnuBlocks frame;   // F and G over no block at all: asked for the cell limit alone
  TRY(ann_frame_layout(K, cluster, n_c, &o->mw, &frame, [&](uint64_t*, uint64_t*) -> int {
    VDB_ARG(n_c > 0 && dim > 0 && dim <= ((size_t)1 << 20), "empty cluster, dim = 0 or dim above 2^20");
    VDB_ARG(n_c <= (size_t)VDB_NEAREST_TOPK_MAX_INSTANCES / dim, "recentre too large: n_c * dim at most VDB_NEAREST_TOPK_MAX_INSTANCES");
    VDB_ARG(fp->host.P >= 63 || n_c < ((uint64_t)1 << fp->host.P), "n_c not below 2^P: quantization(n_c) would not pass qdiv's divisor bound 2^(2P)");
    return mku_layout(K, dim, 1, nullptr, 0, &o->mu, nullptr, nullptr, nullptr);   // K = 1: a centroids' tree of one leaf has no path
  }));
  mk_layout(n_c, dim, 0, &o->mm);
  o->b = annr_blocks(K, n_c, dim, o->mw.total, fp->host.sz.qdiv[0], fp->host.sz.qdiv[1], o->mm.total, o->mu.total);
  VDB_ARG(o->b.total <= VDB_NEAREST_TOPK_MAX_CELLS, "recentre circuit above 2^34 cells");
  return VDB_OK;
}
// levels: the centroids' tree (2 lp_K digests, a copy the caller owns), left in the state after the write; roots: [centroids_root | the K
// cluster roots]; levels_m: cluster c's tree where it is resident, or null; new_centroid: dim words out; pub: [index_root_old | c |
// index_root_new].  The quotients and the chain totals live in the frame's work space (`extra`, scratch slot 7).  Scratch slot 0 has
// one user at a time: M asks for nothing there; mk_emit (MM) takes it first and every launch that reads what it put there is enqueued
// before mku_emit (U) takes it again (the stream orders them); G's states are the frame's own.
int wit_ann_recentre_dev(FpEntry* fp, u256* levels, const u256* members, const u256* roots, const u256* levels_m, size_t K, size_t cluster, size_t n_c,
                         size_t dim, Streams st, u256* new_centroid, u256* pub) {
  static thread_local MkuPlan pl;
  AnnrLayout a;
  TRY(annr_layout(fp, K, cluster, n_c, dim, &a));
  const AnnrBlocks& b = a.b;
  const uint64_t slot = cluster;
  TRY(mku_plan(K, dim, 0, new_centroid, &slot, nullptr, 1, &pl));   // (the plan only asks that a write has a vector: the quotients, below)
  AnnFrame f;
  TRY(f.open(st, roots, K, cluster, b.h, a.mw, b.total, 5, 2 * dim));
  TRY(set_winv(f.st, fp->dev));   // the head's gadgets are GateChip's alone; M reads the tables of (P, L)
  u256 *mean = f.extra, *sums = mean + dim;
  VDB_LAUNCH(k_mku_inputs, dim3((unsigned)((n_c * dim + 255) / 256)), dim3(256), f.st, b.b_in, members, members, (uint64_t)(n_c * dim), (uint64_t)(n_c * dim));
  const u256 len = fr_mul(to_mont<Fr>(u256_from_u64(n_c)), fp->host.scale);   // load_constant(quantization(n_c))
  VDB_LAUNCH(k_push_cells, dim3(1), dim3(1), f.st, b.b_m, len, len, 1u);
  VDB_LAUNCH(k_annm_sum, dim3((unsigned)dim), dim3(64), f.st, fp->dev, b.b_chain, (uint32_t)n_c, (uint32_t)dim, members, sums);
  VDB_LAUNCH(k_annr_div, dim3((unsigned)((dim + 63) / 64), 8), dim3(64), f.st, fp->dev, b.b_div, (uint32_t)dim, sums, len, mean);
  TRY(mk_emit(fp, f.sp, members, n_c, dim, a.mm, f.st, b.b_mm, levels_m, nullptr));
  TRY(mku_emit(fp, f.sp, pl, levels, dim, mean, f.st, b.b_upd, f.upub));
  TRY(f.close_word0(b.b_root, f.upub + 4));
  VDB_LAUNCH(k_annu_public, dim3(1), dim3(256), f.upub, f.hdr, f.iroot, 0u, pub);
  VDB_HIP(hipMemcpyAsync(new_centroid, mean, dim * sizeof(u256), hipMemcpyDeviceToDevice, ctx().stream));
  return inv_list_fixup(f.st);
}

// ------------------------------------------------------------------ the cover of the database by the index (include/vdb.h
// vdb_wit_ann_cover): the multiset of the n leaf digests under database_root is the union of the multisets of the leaf digests under
// the K cluster roots of index_root.  On leaf digests alone: no vector is hashed.  Blocks (AnncBlocks, ann_update_host.hpp): A the
// header [centroids_root | cluster roots], I the digests a (slot order) and b (grouped order), Z the one zero cell, TD the database
// tree over a, TC the K cluster trees over their stretches of b (each root tied to the header), D the sponge over the header ->
// index_root, G the sponge over [droot, index_root] -> gamma, then prod (gamma - a_i) and prod (gamma - b_j), whose last cells are tied.
// Every tree is read where it lies: tree 0 is `dbtree` (2 lp digests), tree 1 + c is segment c of `forest` (seg_off[c], 2 lp_c digests).
struct AnncLayout {
  MkLayout mw;
  AnncBlocks b;
};
static int annc_layout(const uint64_t* sizes, size_t K, size_t n, AnncLayout* o) {
  VDB_ARG(sizes, "null pointer");
  VDB_ARG(K > 0 && K <= VDB_ANN_MAX_CLUSTERS, "K = 0 or K above VDB_ANN_MAX_CLUSTERS");
  VDB_ARG(n <= VDB_ANN_MAX_VECTORS, "n above VDB_ANN_MAX_VECTORS");
  mk_layout(1, K + 1, 1, &o->mw);
  const int rc = annc_blocks(sizes, K, VDB_ANN_MAX_VECTORS, o->mw.total, NODE_CELLS, &o->b);
  VDB_ARG(rc != 1, "empty cluster: merkle_commitment is undefined over zero vectors");
  VDB_ARG(rc == 0 && o->b.n == n, "the cluster sizes do not sum to n");
  VDB_ARG(o->b.total <= ((uint64_t)1 << 34), "cover circuit above 2^34 cells");
  return VDB_OK;
}
// blocks A and I, a lane per cell: the header's word i (lane 0: the centroids' root, lane 1 + c: the root of forest segment c), then a_j
// = level 0 of the database tree, then b_j = level 0 of its cluster's segment (the cluster by bisection in the offsets).  The values
// stay in `words` (K + 1) and `ab` (2 n) for the sponge and the products; lane K + 1 leaves the database root in pubv[0]
__global__ __launch_bounds__(256) void k_annc_inputs(Streams st, const u256* __restrict__ croot, const u256* __restrict__ dbtree, const u256* __restrict__ forest,
                                                     const uint64_t* __restrict__ seg_off, const uint64_t* __restrict__ offsets,
                                                     const uint32_t* __restrict__ lp_t, uint32_t K, uint32_t n, u256* __restrict__ words,
                                                     u256* __restrict__ ab, u256* __restrict__ pubv) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (uint64_t)K + 1 + 2ull * n) return;
  u256 v;
  if (i <= K) {
    v = i ? forest[seg_off[i - 1] + 2 * (uint64_t)lp_t[i] - 2] : *croot;
    words[i] = v;
  } else {
    const uint32_t j = (uint32_t)(i - K - 1);
    if (j < n) {
      v = dbtree[j];
      if (j == 0) pubv[0] = dbtree[2 * (uint64_t)lp_t[0] - 2];
    } else {
      const uint32_t g = j - n;
      uint32_t lo = 0, hi = K;   // the cluster c with offsets[c] <= g < offsets[c + 1] (no cluster is empty)
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (offsets[mid] <= g) lo = mid; else hi = mid;
      }
      v = forest[seg_off[lo] + (g - offsets[lo])];
    }
    ab[j] = v;
  }
  if (i < st.rlo || i >= st.rhi) return;
  st.adv[i] = v;
  if (st.sel) st.sel[i] = 0;
}
// Blocks TD and TC in ONE launch: a thread per (node, permutation half) of the K + 1 trees.  The tree is found by bisection in the prefix
// sums of the node counts (node_pre, n_tree + 1 entries; a tree of one leaf has no node and shares its successor's prefix), the level
// inside the tree by k_mk_tree_trace's walk; the trees' cells follow each other, so node t of the launch has its cells at base + t NODE_CELLS
__global__ __launch_bounds__(64) void k_annc_forest_trace(Streams stq, const FpTables* __restrict__ T, const PoseidonSpec* __restrict__ sp,
                                                          const u256* __restrict__ dbtree, const u256* __restrict__ forest,
                                                          const uint64_t* __restrict__ seg_off, const uint32_t* __restrict__ lp_t,
                                                          const uint32_t* __restrict__ node_pre, uint32_t n_tree, uint64_t base) {
  const uint32_t id = blockIdx.x * 64 + threadIdx.x;
  const uint32_t t = id >> 1, j = id & 1u;
  if (t >= node_pre[n_tree]) return;
  uint32_t lo = 0, hi = n_tree;   // the last tree s with node_pre[s] <= t
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (node_pre[mid] <= t) lo = mid; else hi = mid;
  }
  const uint32_t g = t - node_pre[lo], lp = lp_t[lo];
  const u256* levels = lo ? forest + seg_off[lo - 1] : dbtree;
  uint32_t sz = lp >> 1, first = 0, in_off = 0, in_sz = lp;
  while (g >= first + sz) {
    first += sz;
    in_off += in_sz;
    in_sz = sz;
    sz >>= 1;
  }
  const u256* in = levels + in_off + 2 * (g - first);
  trace_node_half(stq, T, sp, base + (uint64_t)t * NODE_CELLS, in, in + 1, j);
}
// Blocks SA, MA (workgroup 0, over a) and SB, MB (workgroup 1, over b): t_i = g_sub(gamma, x_i) at sub + 4 i, acc_i = g_mul(acc_{i-1},
// t_i) at mul + 4 (i - 1), acc_0 = t_0.  Each thread owns a contiguous stretch: its total of (gamma - x_i), an inclusive product scan
// of the totals in LDS (block_scan_mul's scheme, polyops.hip), then the stretch again from the exclusive prefix, through the context's
// own g_sub / g_mul: the flags are theirs and push() keeps to the rank window.  gamma is read where G's sponge left it.
#define ANNC_THREADS 256
__global__ __launch_bounds__(ANNC_THREADS) void k_annc_products(Streams st, const FpTables* __restrict__ T, const u256* __restrict__ ab,
                                                                const u256* __restrict__ gamma_at, uint32_t n, uint64_t b_sa, uint64_t b_ma,
                                                                uint64_t b_sb, uint64_t b_mb) {
  __shared__ u256 sh[ANNC_THREADS];
  const uint32_t tid = threadIdx.x, side = blockIdx.x;
  const u256* x = ab + (size_t)side * n;
  const uint64_t sub = side ? b_sb : b_sa, mul = side ? b_mb : b_ma;
  const u256 gamma = *gamma_at, one = mont_one<Fr>();
  const uint32_t E = (n + ANNC_THREADS - 1) / ANNC_THREADS;
  const uint32_t lo = (uint64_t)tid * E < n ? tid * E : n, hi = lo + E < n ? lo + E : n;
  u256 v = one;
  for (uint32_t i = lo; i < hi; i++) v = fr_mul(v, fr_sub(gamma, x[i]));
  sh[tid] = v;
  __syncthreads();
  for (uint32_t o = 1; o < ANNC_THREADS; o <<= 1) {
    const u256 other = tid >= o ? sh[tid - o] : one;
    __syncthreads();
    if (tid >= o) {
      v = fr_mul(v, other);
      sh[tid] = v;
    }
    __syncthreads();
  }
  u256 acc = tid ? sh[tid - 1] : one;   // the product of every factor in front of the stretch
  WCtx c = make_ctx(st, T, 0, 0);
  Gadgets g(c);
  for (uint32_t i = lo; i < hi; i++) {
    c.pos = sub + 4ull * i;
    const u256 t = g.g_sub(gamma, x[i]);
    if (i == 0) {
      acc = t;
    } else {
      c.pos = mul + 4ull * (i - 1);
      acc = g.g_mul(acc, t);
    }
  }
}
// the tables of a call: [seg_off K + 1 | offsets K + 1] and [lp_t K + 1 | node_pre K + 2] (pageable sources of asynchronous uploads)
struct AnncTables {
  std::vector<uint64_t> u64;
  std::vector<uint32_t> u32;
};
// a_leaves / b_leaves: the n database leaf digests in slot order and the n cluster leaf digests in grouped order, read only when the
// trees are not resident (then they are hashed here, a launch per level and tree); dbtree / forest: the resident trees, both or neither;
// croot: the centroids' root; pub: [database_root | index_root].  The work space is scratch slot 7 alone: scratch slot 0 is not touched.
int wit_ann_cover_dev(const u256* a_leaves, const u256* b_leaves, const u256* croot, const uint64_t* sizes, size_t K, size_t n, const u256* dbtree,
                      const u256* forest, Streams st, u256* pub) {
  static thread_local AnncTables tb;
  AnncLayout a;
  TRY(annc_layout(sizes, K, n, &a));
  const AnncBlocks& b = a.b;
  const bool resident = dbtree != nullptr;
  tb.u64.assign(2 * (K + 1), 0);
  tb.u32.assign(2 * K + 3, 0);
  uint64_t *seg_off = tb.u64.data(), *offsets = seg_off + K + 1;
  uint32_t *lp_t = tb.u32.data(), *node_pre = lp_t + K + 1;
  lp_t[0] = (uint32_t)b.lp;
  node_pre[1] = (uint32_t)(b.lp - 1);
  for (size_t c = 0; c < K; c++) {
    uint64_t lp_c;
    uint32_t d;
    tree_shape(sizes[c], &lp_c, &d);
    lp_t[1 + c] = (uint32_t)lp_c;
    seg_off[c + 1] = seg_off[c] + 2 * lp_c;
    offsets[c + 1] = offsets[c] + sizes[c];
    node_pre[c + 2] = node_pre[c + 1] + (uint32_t)(lp_c - 1);
  }
  const uint64_t n_nodes = node_pre[K + 1], n_forest = seg_off[K];
  const size_t n_st_d = (size_t)a.mw.nperm * PSD_T, n_st_g = 2 * PSD_T;
  const size_t n_u256 = (K + 1) + 3 + n_st_d + n_st_g + 2 * n + (resident ? 0 : 2 * b.lp + n_forest) + 8;
  u256* words = (u256*)scratch_get(7, n_u256 * sizeof(u256) + 2 * (K + 1) * 8 + (2 * K + 3 + 16) * 4);
  if (!words) return VDB_ERR_OOM;
  u256 *pubv = words + K + 1, *gamma = pubv + 2, *st_d = gamma + 1, *st_g = st_d + n_st_d, *ab = st_g + n_st_g, *own = ab + 2 * n;
  uint64_t* d_u64 = (uint64_t*)(words + n_u256);
  uint32_t* d_u32 = (uint32_t*)(d_u64 + 2 * (K + 1));
  const uint64_t *d_seg = d_u64, *d_offsets = d_u64 + K + 1;
  const uint32_t *d_lp = d_u32, *d_pre = d_u32 + K + 1;
  hipStream_t s = ctx().stream;
  FpEntry* fp;
  const PoseidonSpec* sp;
  TRY(mk_begin(st, &fp, &sp));
  VDB_HIP(hipMemcpyAsync(d_u64, tb.u64.data(), 2 * (K + 1) * 8, hipMemcpyHostToDevice, s));
  VDB_HIP(hipMemcpyAsync(d_u32, tb.u32.data(), (2 * K + 3) * 4, hipMemcpyHostToDevice, s));
  if (!resident) {
    u256 *own_db = own, *own_forest = own + 2 * b.lp;
    VDB_HIP(hipMemsetAsync(own, 0, (2 * b.lp + n_forest) * sizeof(u256), s));
    VDB_HIP(hipMemcpyAsync(own_db, a_leaves, n * sizeof(u256), hipMemcpyDeviceToDevice, s));
    TRY(mk_levels_from_leaves(sp, own_db, b.lp, nullptr));
    for (size_t c = 0; c < K; c++) {
      VDB_HIP(hipMemcpyAsync(own_forest + seg_off[c], b_leaves + offsets[c], sizes[c] * sizeof(u256), hipMemcpyDeviceToDevice, s));
      TRY(mk_levels_from_leaves(sp, own_forest + seg_off[c], lp_t[1 + c], nullptr));
    }
    dbtree = own_db;
    forest = own_forest;
  }
  VDB_LAUNCH(k_annc_inputs, dim3((unsigned)((b.n_in + 255) / 256)), dim3(256), st, croot, dbtree, forest, d_seg, d_offsets, d_lp, (uint32_t)K, (uint32_t)n, words,
             ab, pubv);
  VDB_LAUNCH(k_push_cells, dim3(1), dim3(1), st, b.b_z, u256_zero(), u256_zero(), b.zero ? 1u : 0u);
  VDB_LAUNCH(k_annc_forest_trace, dim3((unsigned)((2 * n_nodes + 63) / 64 + (n_nodes == 0))), dim3(64), st, fp->dev, sp, dbtree, forest, d_seg, d_lp, d_pre,
             (uint32_t)(K + 1), b.b_td);
  // D: the sponge over the header -> index_root; G: the sponge over [droot, index_root] -> gamma (two words: a node's cells)
  TRY(mk_leaf_states(sp, words, 1u, (uint32_t)(K + 1), a.mw.nperm, st_d, pubv + 1, nullptr));
  VDB_LAUNCH(k_mk_leaf_trace, dim3((unsigned)((a.mw.nperm + 63) / 64)), dim3(64), st, fp->dev, sp, words, 1u, (uint32_t)(K + 1), a.mw.nperm, b.b_d,
             a.mw.leaf_cells, st_d, nullptr);
  TRY(mk_leaf_states(sp, pubv, 1u, 2u, 2u, st_g, gamma, nullptr));
  VDB_LAUNCH(k_mk_leaf_trace, dim3(1), dim3(64), st, fp->dev, sp, pubv, 1u, 2u, 2u, b.b_g, (uint64_t)NODE_CELLS, st_g, nullptr);
  VDB_LAUNCH(k_annc_products, dim3(2), dim3(ANNC_THREADS), st, fp->dev, ab, gamma, (uint32_t)n, b.b_sa, b.b_ma, b.b_sb, b.b_mb);
  VDB_HIP(hipMemcpyAsync(pub, pubv, 2 * sizeof(u256), hipMemcpyDeviceToDevice, s));
  return VDB_OK;
}

// the means of all K clusters as values alone (include/vdb.h vdb_ann_cluster_means_dev); `offsets`: the host's copy, already checked
static int ann_means_dev(FpEntry* fp, const u256* grouped, const uint64_t* offsets_dev, size_t K, size_t dim, int* err, u256* means) {
  Streams st{nullptr, nullptr, nullptr, err, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};   // the empty rank window: no stream is attached
  TRY(set_winv(st, fp->dev));
  VDB_LAUNCH(k_ann_means, dim3((unsigned)((dim + 63) / 64), (unsigned)K), dim3(64), grouped, offsets_dev, (uint32_t)dim, err, means);
  return VDB_OK;
}
// K > 0, dim > 0, offsets rising from 0 to n with no empty cluster: what the kernel's reads rest on
static int ann_means_check(const uint64_t* offsets, size_t n, size_t K, size_t dim) {
  VDB_ARG(K > 0 && K <= VDB_ANN_MAX_CLUSTERS && dim > 0 && dim <= ((size_t)1 << 20), "K = 0, K above VDB_ANN_MAX_CLUSTERS, dim = 0 or dim above 2^20");
  VDB_ARG(n <= VDB_ANN_MAX_VECTORS && offsets[0] == 0 && offsets[K] == n, "offsets do not run from 0 to n, or n above VDB_ANN_MAX_VECTORS");
  for (size_t k = 0; k < K; k++) VDB_ARG(offsets[k] < offsets[k + 1] && offsets[k + 1] <= n, "an empty cluster, or offsets that do not rise");
  return VDB_OK;
}

}  // namespace vdb

using namespace vdb;

// rank window applied by the *_dev witness entry points (vdb_wit_set_window); full range by default; per device context
#define g_win (vdb::ctx().win)

// the error word of a call on the caller's own buffers: scratch slot 1, cleared on the stream
static int err_word(int** derr) {
  *derr = (int*)scratch_get(1, 64);
  if (!*derr) return VDB_ERR_OOM;
  VDB_HIP(hipMemsetAsync(*derr, 0, sizeof(int), ctx().stream));
  return VDB_OK;
}
struct HostStreams {
  DevBuf adv, sel, lk, err;
  Streams st;
  int init(uint64_t cells, uint64_t lookups, bool want_sel) {
    TRY(adv.alloc(cells * sizeof(u256)));
    TRY(lk.alloc(lookups * sizeof(u256)));
    if (want_sel) TRY(sel.alloc(cells));
    TRY(err.alloc(sizeof(int)));
    VDB_HIP(hipMemsetAsync(err.p, 0, sizeof(int), ctx().stream));
    st.adv = adv.as<u256>();
    st.sel = want_sel ? sel.as<uint8_t>() : nullptr;
    st.lk = lk.as<u256>();
    st.err = err.as<int>();
    st.inv_pos = nullptr;
    st.inv_val = nullptr;
    st.inv_cnt = nullptr;
    st.inv_cap = 0;
    st.rlo = 0;
    st.rhi = ~0ull;
    st.rllo = 0;
    st.rlhi = ~0ull;
    return VDB_OK;
  }
  int finish(vdb_fr* stream_out, vdb_fr* lookup_out, uint8_t* sel_out, uint64_t cells, uint64_t lookups) {
    TRY(download(stream_out, st.adv, cells * sizeof(u256)));
    TRY(download(lookup_out, st.lk, lookups * sizeof(u256)));
    if (sel_out && st.sel) TRY(download(sel_out, st.sel, cells));
    return check_err_flag(st.err);
  }
};
// the streams of a *_dev entry point: the caller's device buffers under the current rank window (vdb_wit_set_window)
struct DevStreams {
  Streams st;
  // with the error word (distance, fp_op, nearest, kmeans)
  int init(vdb_fr* stream_dev, uint8_t* selector_dev, vdb_fr* lookup_dev) {
    int* derr;
    TRY(err_word(&derr));
    st = Streams{as_u256(stream_dev), selector_dev, as_u256(lookup_dev), derr, nullptr, nullptr, nullptr, 0, g_win[0], g_win[1], g_win[2], g_win[3]};
    return VDB_OK;
  }
  // without error word and lookups (merkle, merkle_update: GateChip primitives only)
  void init(vdb_fr* stream_dev, uint8_t* selector_dev) {
    st = Streams{as_u256(stream_dev), selector_dev, nullptr, nullptr, nullptr, nullptr, nullptr, 0, g_win[0], g_win[1], 0, ~0ull};
  }
  int finish() { return st.err ? check_err_flag(st.err) : VDB_OK; }
};

// What the host-array entry points of the two circuits against the index root share: the cluster's 2 lp levels and the K + 1 roots go
// up, run(levels, roots, streams, public) emits the circuit, the public row and the levels as the batch left them come back.
template <class Run>
static int ann_batch_host(vdb_fr* levels, uint64_t lp, const vdb_fr* roots, size_t K, uint64_t cells, size_t n_pub, vdb_fr* stream_out, uint8_t* selector_out,
                          vdb_fr* public_out, Run run) {
  DevBuf dl, dr, dpub;
  HostStreams hs;
  TRY(upload(dl, levels, 2 * lp * sizeof(u256)));
  TRY(upload(dr, roots, (K + 1) * sizeof(u256)));
  TRY(dpub.alloc(n_pub * sizeof(u256)));
  TRY(hs.init(cells, 0, selector_out != nullptr));
  TRY(run(dl.as<u256>(), dr.as<u256>(), hs.st, dpub.as<u256>()));
  TRY(download(public_out, dpub.p, n_pub * sizeof(u256)));
  TRY(download(levels, dl.p, 2 * lp * sizeof(u256)));
  return hs.finish(stream_out, nullptr, selector_out, cells, 0);
}
// What the host-array entry points of the two audits share: centroids, members and the K + 1 roots go up, run(centroids, members, roots,
// streams, flags, public) emits the circuit, the n_flags flag bytes and the public row [index_root | c] come back.
template <class Run>
static int ann_cluster_host(const vdb_fr* centroids, const vdb_fr* members, const vdb_fr* roots, size_t K, size_t n_c, size_t dim, uint64_t cells, uint64_t lookups,
                            size_t n_flags, vdb_fr* stream_out, vdb_fr* lookup_out, uint8_t* selector_out, uint8_t* flags_out, vdb_fr* public_out, Run run) {
  DevBuf dc, dm, dr, dfl, dpub;
  HostStreams hs;
  TRY(upload(dc, centroids, K * dim * sizeof(u256)));
  TRY(upload(dm, members, n_c * dim * sizeof(u256)));
  TRY(upload(dr, roots, (K + 1) * sizeof(u256)));
  TRY(dfl.alloc(n_flags));
  TRY(dpub.alloc(2 * sizeof(u256)));
  TRY(hs.init(cells, lookups, selector_out != nullptr));
  TRY(run(dc.as<u256>(), dm.as<u256>(), dr.as<u256>(), hs.st, dfl.as<uint8_t>(), dpub.as<u256>()));
  TRY(download(flags_out, dfl.p, n_flags));
  TRY(download(public_out, dpub.p, 2 * sizeof(u256)));
  return hs.finish(stream_out, lookup_out, selector_out, cells, lookups);
}
// and their _dev forms: the pointer refusals, the tables of (P, L), the caller's buffers under the rank window; run(fp, levels_c, levels_m, streams) emits
template <class Run>
static int ann_cluster_dev(uint32_t P, uint32_t L, const vdb_fr* centroids_dev, const vdb_fr* members_dev, const vdb_fr* roots_dev, const vdb_fr* centroid_levels_dev,
                           const vdb_fr* member_levels_dev, vdb_fr* stream_dev, vdb_fr* lookup_dev, uint8_t* selector_dev, const uint8_t* flags_dev, const vdb_fr* public_dev, Run run) {
  VDB_REQUIRE_INIT();
  VDB_ARG(centroids_dev && members_dev && roots_dev && stream_dev && lookup_dev && flags_dev && public_dev, "null pointer");
  VDB_ARG(!centroid_levels_dev == !member_levels_dev, "the two resident trees are given together or not at all");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DevStreams ds;
  TRY(ds.init(stream_dev, selector_dev, lookup_dev));
  TRY(run(fp, centroid_levels_dev ? as_u256(centroid_levels_dev) : nullptr, member_levels_dev ? as_u256(member_levels_dev) : nullptr, ds.st));
  return ds.finish();
}

extern "C" {

int vdb_fp_quantize(uint32_t precision_bits, const double* x, vdb_fr* out, size_t n) {
  VDB_ARG(x && out && precision_bits >= 32 && precision_bits <= 63, "bad argument");
  for (size_t i = 0; i < n; i++) {
    u256 q = quantize_host(precision_bits, x[i]);
    memcpy(&out[i], &q, 32);
  }
  return VDB_OK;
}
int vdb_fp_dequantize(uint32_t precision_bits, const vdb_fr* x, double* out, size_t n) {
  VDB_ARG(x && out && precision_bits >= 32 && precision_bits <= 63, "bad argument");
  for (size_t i = 0; i < n; i++) {
    u256 v;
    memcpy(&v, &x[i], 32);
    out[i] = dequantize_host(precision_bits, v);
  }
  return VDB_OK;
}

int vdb_wit_distance_size(int metric, uint32_t P, uint32_t L, size_t n_pairs, size_t dim, uint64_t* cells, uint64_t* lookups) {
  VDB_REQUIRE_INIT();
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DistLayout dl;
  TRY(dist_layout(fp->host, metric, dim, &dl));
  if (cells) *cells = n_pairs * dl.total_cells;
  if (lookups) *lookups = n_pairs * dl.total_lk;
  return VDB_OK;
}
int vdb_wit_distance(int metric, uint32_t P, uint32_t L, const vdb_fr* a, const vdb_fr* b, size_t n_pairs, size_t dim, vdb_fr* stream_out,
                     vdb_fr* lookup_out, uint8_t* selector_out, vdb_fr* result_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(a && b && dim > 0, "null pointer or dim == 0");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  uint64_t cells, lookups;
  TRY(vdb_wit_distance_size(metric, P, L, n_pairs, dim, &cells, &lookups));
  if (n_pairs == 0) return VDB_OK;
  DevBuf da, db, dres;
  HostStreams hs;
  TRY(upload(da, a, n_pairs * dim * sizeof(u256)));
  TRY(upload(db, b, n_pairs * dim * sizeof(u256)));
  TRY(dres.alloc(n_pairs * sizeof(u256)));
  TRY(hs.init(cells, lookups, selector_out != nullptr));
  TRY(wit_distance_dev(fp, metric, da.as<u256>(), db.as<u256>(), n_pairs, dim, hs.st, dres.as<u256>()));
  TRY(download(result_out, dres.p, n_pairs * sizeof(u256)));
  return hs.finish(stream_out, lookup_out, selector_out, cells, lookups);
}

int vdb_wit_distance_dev(int metric, uint32_t P, uint32_t L, const vdb_fr* a_dev, const vdb_fr* b_dev, size_t n_pairs, size_t dim, vdb_fr* stream_dev,
                         vdb_fr* lookup_dev, uint8_t* selector_dev, vdb_fr* result_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(a_dev && b_dev && stream_dev && lookup_dev && result_dev && n_pairs > 0 && dim > 0, "null pointer or empty input");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DevStreams ds;
  TRY(ds.init(stream_dev, selector_dev, lookup_dev));
  TRY(wit_distance_dev(fp, metric, as_u256(a_dev), as_u256(b_dev), n_pairs, dim, ds.st, as_u256(result_dev)));
  return ds.finish();
}

int vdb_wit_fp_op_size(int op, uint32_t P, uint32_t L, size_t n, uint64_t* cells, uint64_t* lookups) {
  VDB_REQUIRE_INIT();
  VDB_ARG(op >= 0 && op < FP_OP_COUNT, "unknown fixed-point operation");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  uint32_t sz[2];
  fp_op_size(fp->host, op, sz);
  if (cells) *cells = n * (uint64_t)sz[0];
  if (lookups) *lookups = n * (uint64_t)sz[1];
  return VDB_OK;
}
int vdb_wit_fp_op(int op, uint32_t P, uint32_t L, const vdb_fr* a, const vdb_fr* b, size_t n, vdb_fr* stream_out, vdb_fr* lookup_out,
                  uint8_t* selector_out, vdb_fr* result_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(a && result_out, "null pointer");
  uint64_t cells, lookups;
  TRY(vdb_wit_fp_op_size(op, P, L, n, &cells, &lookups));
  if (n == 0) return VDB_OK;
  VDB_ARG(n <= 0xffffffffull, "too many instances for one call");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DevBuf da, db, dres;
  HostStreams hs;
  TRY(upload(da, a, n * sizeof(u256)));
  if (b) TRY(upload(db, b, n * sizeof(u256)));
  TRY(dres.alloc(n * sizeof(u256)));
  TRY(hs.init(cells, lookups, selector_out != nullptr));
  TRY(wit_fp_op_dev(fp, op, da.as<u256>(), b ? db.as<u256>() : nullptr, n, hs.st, dres.as<u256>()));
  TRY(download(result_out, dres.p, n * sizeof(u256)));
  return hs.finish(stream_out, lookup_out, selector_out, cells, lookups);
}
int vdb_wit_fp_op_dev(int op, uint32_t P, uint32_t L, const vdb_fr* a_dev, const vdb_fr* b_dev, size_t n, vdb_fr* stream_dev, vdb_fr* lookup_dev,
                      uint8_t* selector_dev, vdb_fr* result_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(op >= 0 && op < FP_OP_COUNT, "unknown fixed-point operation");
  VDB_ARG(a_dev && stream_dev && lookup_dev && result_dev && n > 0 && n <= 0xffffffffull, "null pointer or empty input");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DevStreams ds;
  TRY(ds.init(stream_dev, selector_dev, lookup_dev));
  TRY(wit_fp_op_dev(fp, op, as_u256(a_dev), as_u256(b_dev), n, ds.st, as_u256(result_dev)));
  return ds.finish();
}

// the topk nearest vectors of every one of n_queries queries (include/vdb.h): nearest_vector's distances, then its closing stages once per
// round.  The batch entry points are these at topk = 1, the single-query ones at n_queries = 1 too.
int vdb_wit_nearest_topk_size(int metric, uint32_t P, uint32_t L, size_t n_queries, size_t n, size_t dim, size_t topk, uint64_t* cells,
                              uint64_t* lookups) {
  VDB_REQUIRE_INIT();
  VDB_ARG(n_queries > 0 && n > 0, "no query or empty database");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DistLayout dl;
  NvLayout nl;
  TRY(nv_layout(fp, metric, n, dim, topk, &dl, &nl));
  TRY(nv_fits(n_queries, n, dim, topk, nl));
  if (cells) *cells = n_queries * nl.total;
  if (lookups) *lookups = n_queries * nl.total_l;
  return VDB_OK;
}
int vdb_wit_nearest_topk(int metric, uint32_t P, uint32_t L, const vdb_fr* queries, const vdb_fr* vectors, size_t n_queries, size_t n, size_t dim,
                         size_t topk, vdb_fr* stream_out, vdb_fr* lookup_out, uint8_t* selector_out, vdb_fr* indicators_out, vdb_fr* results_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(queries && vectors && n_queries > 0 && n > 0 && dim > 0, "null pointer or empty input");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  uint64_t cells, lookups;
  TRY(vdb_wit_nearest_topk_size(metric, P, L, n_queries, n, dim, topk, &cells, &lookups));
  DevBuf dq, dv, dind, dres;
  HostStreams hs;
  TRY(upload(dq, queries, n_queries * dim * sizeof(u256)));
  TRY(upload(dv, vectors, n * dim * sizeof(u256)));
  TRY(dind.alloc(n_queries * topk * n * sizeof(u256)));
  TRY(dres.alloc(n_queries * topk * dim * sizeof(u256)));
  TRY(hs.init(cells, lookups, selector_out != nullptr));
  TRY(wit_nearest_dev(fp, metric, dq.as<u256>(), dv.as<u256>(), n_queries, n, dim, topk, hs.st, dind.as<u256>(), dres.as<u256>()));
  TRY(download(indicators_out, dind.p, n_queries * topk * n * sizeof(u256)));
  TRY(download(results_out, dres.p, n_queries * topk * dim * sizeof(u256)));
  return hs.finish(stream_out, lookup_out, selector_out, cells, lookups);
}
int vdb_wit_nearest_topk_dev(int metric, uint32_t P, uint32_t L, const vdb_fr* queries_dev, const vdb_fr* vectors_dev, size_t n_queries, size_t n,
                             size_t dim, size_t topk, vdb_fr* stream_dev, vdb_fr* lookup_dev, uint8_t* selector_dev, vdb_fr* indicators_dev,
                             vdb_fr* results_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(queries_dev && vectors_dev && stream_dev && lookup_dev && indicators_dev && results_dev && n_queries > 0 && n > 0 && dim > 0,
          "null pointer or empty input");
  VDB_ARG(topk > 0 && topk <= n, "topk must be at least 1 and at most n");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  // the rank window (vdb_wit_set_window): a rank stores the cells of its own columns — the distances, N-way parallel and nearly all of
  // the cells, exit early outside it — while every rank computes every value (the distances, the short minimum chains)
  DevStreams ds;
  TRY(ds.init(stream_dev, selector_dev, lookup_dev));
  TRY(wit_nearest_dev(fp, metric, as_u256(queries_dev), as_u256(vectors_dev), n_queries, n, dim, topk, ds.st, as_u256(indicators_dev),
                      as_u256(results_dev)));
  return ds.finish();
}

// the minimum distance of every query and the last vector at it, values only (include/vdb.h): no stream, no window
int vdb_nearest_values_dev(uint32_t P, uint32_t L, int metric, const vdb_fr* queries_dev, const vdb_fr* vectors_dev, size_t n_queries, size_t n, size_t dim,
                           uint32_t* idx_out_dev, vdb_fr* dist_out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(queries_dev && vectors_dev && idx_out_dev && n_queries > 0 && n > 0 && dim > 0, "null pointer or empty input");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  int* derr;
  TRY(err_word(&derr));
  TRY(nearest_values_dev(fp, metric, as_u256(queries_dev), as_u256(vectors_dev), n_queries, n, dim, derr, idx_out_dev, as_u256(dist_out_dev)));
  return check_err_flag(derr);
}
int vdb_nearest_values(uint32_t P, uint32_t L, int metric, const vdb_fr* queries, const vdb_fr* vectors, size_t n_queries, size_t n, size_t dim,
                       uint32_t* idx_out, vdb_fr* dist_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(queries && vectors && idx_out && n_queries > 0 && n > 0 && dim > 0, "null pointer or empty input");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DistLayout dl;
  NvLayout nl;
  TRY(nv_layout(fp, metric, n, dim, 1, &dl, &nl));
  TRY(nv_fits(n_queries, n, dim, 1, nl));   // before anything is uploaded
  DevBuf dq, dv, didx, ddist;
  TRY(upload(dq, queries, n_queries * dim * sizeof(u256)));
  TRY(upload(dv, vectors, n * dim * sizeof(u256)));
  TRY(didx.alloc(n_queries * sizeof(uint32_t)));
  TRY(ddist.alloc(n_queries * sizeof(u256)));
  TRY(vdb_nearest_values_dev(P, L, metric, dq.as<vdb_fr>(), dv.as<vdb_fr>(), n_queries, n, dim, didx.as<uint32_t>(), ddist.as<vdb_fr>()));
  TRY(download(idx_out, didx.p, n_queries * sizeof(uint32_t)));
  TRY(download(dist_out, ddist.p, n_queries * sizeof(u256)));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}
// every round's minimum and the last entry at it, values only (include/vdb.h): no stream, no window
int vdb_nearest_topk_values_dev(uint32_t P, uint32_t L, int metric, const vdb_fr* queries_dev, const vdb_fr* vectors_dev, size_t n_queries, size_t n,
                                size_t dim, size_t p, uint32_t* idx_out_dev, vdb_fr* dist_out_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(queries_dev && vectors_dev && idx_out_dev && n_queries > 0 && n > 0 && dim > 0, "null pointer or empty input");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  int* derr;
  TRY(err_word(&derr));
  TRY(nearest_topk_values_dev(fp, metric, as_u256(queries_dev), as_u256(vectors_dev), n_queries, n, dim, p, derr, idx_out_dev, as_u256(dist_out_dev)));
  return check_err_flag(derr);
}
int vdb_nearest_topk_values(uint32_t P, uint32_t L, int metric, const vdb_fr* queries, const vdb_fr* vectors, size_t n_queries, size_t n, size_t dim,
                            size_t p, uint32_t* idx_out, vdb_fr* dist_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(queries && vectors && idx_out && n_queries > 0 && n > 0 && dim > 0, "null pointer or empty input");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DistLayout dl;
  NvLayout nl;
  TRY(nv_layout(fp, metric, n, dim, p, &dl, &nl));
  TRY(nv_fits(n_queries, n, dim, p, nl));   // before anything is uploaded
  DevBuf dq, dv, didx, ddist;
  TRY(upload(dq, queries, n_queries * dim * sizeof(u256)));
  TRY(upload(dv, vectors, n * dim * sizeof(u256)));
  TRY(didx.alloc(n_queries * p * sizeof(uint32_t)));
  TRY(ddist.alloc(n_queries * p * sizeof(u256)));
  TRY(vdb_nearest_topk_values_dev(P, L, metric, dq.as<vdb_fr>(), dv.as<vdb_fr>(), n_queries, n, dim, p, didx.as<uint32_t>(), ddist.as<vdb_fr>()));
  TRY(download(idx_out, didx.p, n_queries * p * sizeof(uint32_t)));
  TRY(download(dist_out, ddist.p, n_queries * p * sizeof(u256)));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}

// nearest_vector (vectordb.rs:122-163) for n_queries queries over one database, the calls end to end in the streams
int vdb_wit_nearest_batch_size(int metric, uint32_t P, uint32_t L, size_t n_queries, size_t n, size_t dim, uint64_t* cells, uint64_t* lookups) {
  return vdb_wit_nearest_topk_size(metric, P, L, n_queries, n, dim, 1, cells, lookups);
}
int vdb_wit_nearest_batch(int metric, uint32_t P, uint32_t L, const vdb_fr* queries, const vdb_fr* vectors, size_t n_queries, size_t n, size_t dim,
                          vdb_fr* stream_out, vdb_fr* lookup_out, uint8_t* selector_out, vdb_fr* indicators_out, vdb_fr* results_out) {
  return vdb_wit_nearest_topk(metric, P, L, queries, vectors, n_queries, n, dim, 1, stream_out, lookup_out, selector_out, indicators_out, results_out);
}
int vdb_wit_nearest_batch_dev(int metric, uint32_t P, uint32_t L, const vdb_fr* queries_dev, const vdb_fr* vectors_dev, size_t n_queries, size_t n,
                              size_t dim, vdb_fr* stream_dev, vdb_fr* lookup_dev, uint8_t* selector_dev, vdb_fr* indicators_dev, vdb_fr* results_dev) {
  return vdb_wit_nearest_topk_dev(metric, P, L, queries_dev, vectors_dev, n_queries, n, dim, 1, stream_dev, lookup_dev, selector_dev, indicators_dev,
                                  results_dev);
}

// nearest_vector (vectordb.rs:122-163) for one query
int vdb_wit_nearest_size(int metric, uint32_t P, uint32_t L, size_t n, size_t dim, uint64_t* cells, uint64_t* lookups) {
  return vdb_wit_nearest_topk_size(metric, P, L, 1, n, dim, 1, cells, lookups);
}
int vdb_wit_nearest(int metric, uint32_t P, uint32_t L, const vdb_fr* query, const vdb_fr* vectors, size_t n, size_t dim, vdb_fr* stream_out,
                    vdb_fr* lookup_out, uint8_t* selector_out, vdb_fr* indicator_out, vdb_fr* result_out) {
  return vdb_wit_nearest_topk(metric, P, L, query, vectors, 1, n, dim, 1, stream_out, lookup_out, selector_out, indicator_out, result_out);
}
int vdb_wit_nearest_dev(int metric, uint32_t P, uint32_t L, const vdb_fr* query_dev, const vdb_fr* vectors_dev, size_t n, size_t dim, vdb_fr* stream_dev,
                        vdb_fr* lookup_dev, uint8_t* selector_dev, vdb_fr* indicator_dev, vdb_fr* result_dev) {
  return vdb_wit_nearest_topk_dev(metric, P, L, query_dev, vectors_dev, 1, n, dim, 1, stream_dev, lookup_dev, selector_dev, indicator_dev, result_dev);
}

int vdb_wit_kmeans_size(int metric, uint32_t P, uint32_t L, size_t n, size_t dim, size_t K, size_t I, int zero_cached, uint64_t* cells,
                        uint64_t* lookups) {
  VDB_REQUIRE_INIT();
  if (!(K < n) || K == 0) {
    set_error("kmeans requires 0 < K < #vectors (vectordb.rs:238 assert)");
    return VDB_ERR_DOMAIN;
  }
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DistLayout dl;
  KmLayout kl;
  TRY(km_layout(fp, metric, n, dim, K, &dl, &kl));
  if (cells) *cells = (zero_cached ? 1 : 2) + I * kl.iter;
  if (lookups) *lookups = I * kl.iter_l;
  return VDB_OK;
}
int vdb_wit_set_window(uint64_t adv_lo, uint64_t adv_hi, uint64_t lookup_lo, uint64_t lookup_hi) {
  VDB_ARG(adv_lo <= adv_hi && lookup_lo <= lookup_hi, "empty or inverted window");
  g_win[0] = adv_lo;
  g_win[1] = adv_hi;
  g_win[2] = lookup_lo;
  g_win[3] = lookup_hi;
  return VDB_OK;
}
int vdb_wit_kmeans_dev(int metric, uint32_t P, uint32_t L, const vdb_fr* vectors_dev, size_t n, size_t dim, size_t K, size_t I, int zero_cached,
                       vdb_fr* stream_dev, vdb_fr* lookup_dev, uint8_t* selector_dev, vdb_fr* centroids_dev, vdb_fr* indicators_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(vectors_dev && stream_dev && lookup_dev && centroids_dev && indicators_dev && dim > 0, "null pointer");
  uint64_t cells, lookups;
  TRY(vdb_wit_kmeans_size(metric, P, L, n, dim, K, I, zero_cached, &cells, &lookups));
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DevStreams ds;
  TRY(ds.init(stream_dev, selector_dev, lookup_dev));
  TRY(wit_kmeans_dev(fp, metric, as_u256(vectors_dev), n, dim, K, I, zero_cached, ds.st, as_u256(centroids_dev), as_u256(indicators_dev)));
  return ds.finish();
}
int vdb_wit_kmeans(int metric, uint32_t P, uint32_t L, const vdb_fr* vectors, size_t n, size_t dim, size_t K, size_t I, int zero_cached,
                   vdb_fr* stream_out, vdb_fr* lookup_out, uint8_t* selector_out, vdb_fr* centroids_out, vdb_fr* indicators_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(vectors && dim > 0, "null pointer");
  uint64_t cells, lookups;
  TRY(vdb_wit_kmeans_size(metric, P, L, n, dim, K, I, zero_cached, &cells, &lookups));
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DevBuf dv, dc, di;
  HostStreams hs;
  TRY(upload(dv, vectors, n * dim * sizeof(u256)));
  TRY(dc.alloc(K * dim * sizeof(u256)));
  TRY(di.alloc(n * K * sizeof(u256)));
  TRY(hs.init(cells, lookups, selector_out != nullptr));
  TRY(wit_kmeans_dev(fp, metric, dv.as<u256>(), n, dim, K, I, zero_cached, hs.st, dc.as<u256>(), di.as<u256>()));
  TRY(download(centroids_out, dc.p, K * dim * sizeof(u256)));
  TRY(download(indicators_out, di.p, n * K * sizeof(u256)));
  return hs.finish(stream_out, lookup_out, selector_out, cells, lookups);
}

int vdb_wit_merkle_size(size_t n, size_t dim, int zero_cached, uint64_t* cells) {
  VDB_ARG(n > 0 && cells, "empty database");
  MkLayout ml;
  mk_layout(n, dim, zero_cached, &ml);
  *cells = ml.total;
  return VDB_OK;
}
int vdb_wit_merkle_dev(const vdb_fr* vectors_dev, size_t n, size_t dim, int zero_cached, vdb_fr* stream_dev, uint8_t* selector_dev, vdb_fr* root_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(vectors_dev && stream_dev && root_dev && n > 0, "null pointer");
  DevStreams ds;
  ds.init(stream_dev, selector_dev);
  TRY(wit_merkle_dev(as_u256(vectors_dev), n, dim, zero_cached, ds.st, as_u256(root_dev)));
  return ds.finish();
}
int vdb_wit_merkle(const vdb_fr* vectors, size_t n, size_t dim, int zero_cached, vdb_fr* stream_out, uint8_t* selector_out, vdb_fr* root_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(vectors && n > 0, "null pointer or empty database");
  uint64_t cells;
  TRY(vdb_wit_merkle_size(n, dim, zero_cached, &cells));
  DevBuf dv, droot;
  HostStreams hs;
  TRY(upload(dv, vectors, n * dim * sizeof(u256)));
  TRY(droot.alloc(sizeof(u256)));
  TRY(hs.init(cells, 0, selector_out != nullptr));
  TRY(wit_merkle_dev(dv.as<u256>(), n, dim, zero_cached, hs.st, droot.as<u256>()));
  TRY(download(root_out, droot.p, sizeof(u256)));
  return hs.finish(stream_out, nullptr, selector_out, cells, 0);
}

// batches of path updates against the resident tree (include/vdb.h; the tree itself: resident.hip)
int vdb_wit_merkle_update_ops_size(size_t n, size_t dim, size_t m, const uint8_t* kinds, unsigned grow, uint64_t* cells, uint64_t* input_cells) {
  MkuLayout ml;
  TRY(mku_layout(n, dim, m, kinds, grow, &ml, nullptr, nullptr, nullptr));
  if (cells) *cells = ml.total;
  if (input_cells) *input_cells = ml.n_in;
  return VDB_OK;
}
int vdb_wit_merkle_update_ops_dev(vdb_fr* levels_dev, size_t n, size_t dim, unsigned grow, const vdb_fr* new_vectors_dev, const uint64_t* indices,
                                  const uint8_t* kinds, size_t m, vdb_fr* stream_dev, uint8_t* selector_dev, vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels_dev && indices && stream_dev && public_dev, "null pointer");
  DevStreams ds;
  ds.init(stream_dev, selector_dev);
  TRY(wit_merkle_update_dev(as_u256(levels_dev), n, dim, grow, new_vectors_dev ? as_u256(new_vectors_dev) : nullptr, indices, kinds, m, ds.st,
                            as_u256(public_dev)));
  return ds.finish();
}
int vdb_wit_merkle_update_ops(vdb_fr* levels, size_t n, size_t dim, unsigned grow, const vdb_fr* new_vectors, const uint64_t* indices, const uint8_t* kinds,
                              size_t m, vdb_fr* stream_out, uint8_t* selector_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels && indices, "null pointer");
  MkuLayout ml;
  uint64_t lp;
  TRY(mku_layout(n, dim, m, kinds, grow, &ml, &lp, nullptr, nullptr));
  VDB_ARG(new_vectors || ml.w == 0, "null pointer");
  for (size_t j = 0; j < m; j++) VDB_ARG(indices[j] < lp, "update index outside the padded tree (grow it first: vdb_merkle_tree_grow_dev)");
  DevBuf dl, dv, dpub;
  HostStreams hs;
  TRY(upload(dl, levels, 2 * lp * sizeof(u256)));
  if (ml.w) TRY(upload(dv, new_vectors, ml.n_vec * sizeof(u256)));
  TRY(dpub.alloc((3 * m + 2) * sizeof(u256)));
  TRY(hs.init(ml.total, 0, selector_out != nullptr));
  TRY(wit_merkle_update_dev(dl.as<u256>(), n, dim, grow, ml.w ? dv.as<u256>() : nullptr, indices, kinds, m, hs.st, dpub.as<u256>()));
  TRY(download(public_out, dpub.p, (3 * m + 2) * sizeof(u256)));
  TRY(download(levels, dl.p, 2 * lp * sizeof(u256)));
  return hs.finish(stream_out, nullptr, selector_out, ml.total, 0);
}
// a plain batch: every update a write, the tree not grown
int vdb_wit_merkle_update_size(size_t n, size_t dim, size_t m, uint64_t* cells, uint64_t* input_cells) {
  return vdb_wit_merkle_update_ops_size(n, dim, m, nullptr, 0, cells, input_cells);
}
int vdb_wit_merkle_update_dev(vdb_fr* levels_dev, size_t n, size_t dim, const vdb_fr* new_vectors_dev, const uint64_t* indices, size_t m, vdb_fr* stream_dev,
                              uint8_t* selector_dev, vdb_fr* public_dev) {
  return vdb_wit_merkle_update_ops_dev(levels_dev, n, dim, 0, new_vectors_dev, indices, nullptr, m, stream_dev, selector_dev, public_dev);
}
int vdb_wit_merkle_update(vdb_fr* levels, size_t n, size_t dim, const vdb_fr* new_vectors, const uint64_t* indices, size_t m, vdb_fr* stream_out,
                          uint8_t* selector_out, vdb_fr* public_out) {
  return vdb_wit_merkle_update_ops(levels, n, dim, 0, new_vectors, indices, nullptr, m, stream_out, selector_out, public_out);
}

// openings of the resident tree (include/vdb.h)
int vdb_wit_merkle_open_size(size_t n, size_t dim, size_t m, int with_vectors, uint64_t* cells, uint64_t* input_cells) {
  MkoLayout ml;
  TRY(mko_layout(n, dim, m, with_vectors, &ml, nullptr));
  if (cells) *cells = ml.total;
  if (input_cells) *input_cells = ml.n_in;
  return VDB_OK;
}
int vdb_wit_merkle_open_dev(const vdb_fr* levels_dev, size_t n, size_t dim, const vdb_fr* vectors_dev, const uint64_t* indices, size_t m, vdb_fr* stream_dev,
                            uint8_t* selector_dev, vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels_dev && indices && stream_dev && public_dev, "null pointer");
  DevStreams ds;
  ds.init(stream_dev, selector_dev);
  TRY(wit_merkle_open_dev(as_u256(levels_dev), n, dim, vectors_dev ? as_u256(vectors_dev) : nullptr, indices, m, ds.st, as_u256(public_dev)));
  return ds.finish();
}
int vdb_wit_merkle_open(const vdb_fr* levels, size_t n, size_t dim, const vdb_fr* vectors, const uint64_t* indices, size_t m, vdb_fr* stream_out,
                        uint8_t* selector_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels && indices, "null pointer");
  MkoLayout ml;
  uint64_t lp;
  TRY(mko_layout(n, dim, m, vectors != nullptr, &ml, &lp));
  TRY(mko_check_indices(indices, m, lp, n, vectors != nullptr));
  const size_t n_pub = 1 + 2 * m + (vectors ? m * dim : 0);
  DevBuf dl, dv, dpub;
  HostStreams hs;
  TRY(upload(dl, levels, 2 * lp * sizeof(u256)));
  if (vectors) TRY(upload(dv, vectors, m * dim * sizeof(u256)));
  TRY(dpub.alloc(n_pub * sizeof(u256)));
  TRY(hs.init(ml.total, 0, selector_out != nullptr));
  TRY(wit_merkle_open_dev(dl.as<u256>(), n, dim, vectors ? dv.as<u256>() : nullptr, indices, m, hs.st, dpub.as<u256>()));
  TRY(download(public_out, dpub.p, n_pub * sizeof(u256)));
  return hs.finish(stream_out, nullptr, selector_out, ml.total, 0);
}

// the approximate-nearest-neighbour query over the p nearest clusters (include/vdb.h)
int vdb_wit_ann_probe_size(int metric, uint32_t P, uint32_t L, size_t K, size_t dim, size_t p, const size_t* n_c, size_t t, uint64_t* cells,
                           uint64_t* lookups, uint64_t* input_cells) {
  VDB_REQUIRE_INIT();
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  AnnpLayout a;
  TRY(annp_layout(fp, metric, K, dim, p, n_c, t, &a));
  if (cells) *cells = a.total;
  if (lookups) *lookups = a.total_l;
  if (input_cells) *input_cells = a.n_in;
  return VDB_OK;
}
int vdb_wit_ann_probe_dev(int metric, uint32_t P, uint32_t L, const vdb_fr* query_dev, const vdb_fr* centroids_dev, const vdb_fr* const* members_dev,
                          const vdb_fr* cluster_roots_dev, const vdb_fr* centroid_levels_dev, const vdb_fr* const* member_levels_dev, size_t K, size_t dim,
                          size_t p, const size_t* n_c, size_t t, vdb_fr* stream_dev, vdb_fr* lookup_dev, uint8_t* selector_dev,
                          vdb_fr* centroid_indicators_dev, vdb_fr* candidate_indicators_dev, vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(query_dev && centroids_dev && members_dev && cluster_roots_dev && n_c && stream_dev && lookup_dev && centroid_indicators_dev &&
              candidate_indicators_dev && public_dev,
          "null pointer");
  VDB_ARG(p >= 1 && p <= VDB_ANN_PROBE_MAX, "probes: at least 1 and at most VDB_ANN_PROBE_MAX");
  size_t n_resident = centroid_levels_dev ? 1 : 0;
  for (size_t r = 0; r < p; r++) {
    VDB_ARG(members_dev[r], "null pointer");
    if (member_levels_dev && member_levels_dev[r]) n_resident++;
  }
  VDB_ARG(n_resident == 0 || n_resident == p + 1, "the resident trees are given all together or not at all");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DevStreams ds;
  TRY(ds.init(stream_dev, selector_dev, lookup_dev));
  TRY(wit_ann_probe_dev(fp, metric, as_u256(query_dev), as_u256(centroids_dev), (const u256* const*)members_dev, as_u256(cluster_roots_dev),
                        n_resident ? as_u256(centroid_levels_dev) : nullptr, n_resident ? (const u256* const*)member_levels_dev : nullptr, K, dim, p, n_c, t,
                        ds.st, as_u256(centroid_indicators_dev), as_u256(candidate_indicators_dev), as_u256(public_dev)));
  return ds.finish();
}
int vdb_wit_ann_probe(int metric, uint32_t P, uint32_t L, const vdb_fr* query, const vdb_fr* centroids, const vdb_fr* candidates,
                      const vdb_fr* cluster_roots, size_t K, size_t dim, size_t p, const size_t* n_c, size_t t, vdb_fr* stream_out, vdb_fr* lookup_out,
                      uint8_t* selector_out, vdb_fr* centroid_indicators_out, vdb_fr* candidate_indicators_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(query && centroids && candidates && cluster_roots && n_c, "null pointer");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  AnnpLayout a;
  TRY(annp_layout(fp, metric, K, dim, p, n_c, t, &a));
  const uint64_t total = a.total, total_l = a.total_l;
  const size_t N = a.N;
  DevBuf dq, dc, dm, dr, dic, dim_, dpub;
  HostStreams hs;
  TRY(upload(dq, query, dim * sizeof(u256)));
  TRY(upload(dc, centroids, K * dim * sizeof(u256)));
  TRY(upload(dm, candidates, N * dim * sizeof(u256)));
  TRY(upload(dr, cluster_roots, K * sizeof(u256)));
  TRY(dic.alloc(p * K * sizeof(u256)));
  TRY(dim_.alloc(t * N * sizeof(u256)));
  TRY(dpub.alloc((t * dim + 1) * sizeof(u256)));
  const u256* rows[VDB_ANN_PROBE_MAX];
  for (size_t r = 0; r < p; r++) rows[r] = dm.as<u256>() + a.off[r] * dim;
  TRY(hs.init(total, total_l, selector_out != nullptr));
  TRY(wit_ann_probe_dev(fp, metric, dq.as<u256>(), dc.as<u256>(), rows, dr.as<u256>(), nullptr, nullptr, K, dim, p, n_c, t, hs.st, dic.as<u256>(),
                        dim_.as<u256>(), dpub.as<u256>()));
  TRY(download(centroid_indicators_out, dic.p, p * K * sizeof(u256)));
  TRY(download(candidate_indicators_out, dim_.p, t * N * sizeof(u256)));
  TRY(download(public_out, dpub.p, (t * dim + 1) * sizeof(u256)));
  return hs.finish(stream_out, lookup_out, selector_out, total, total_l);
}

// the single-cluster query is the query over the p nearest clusters at p = t = 1 (include/vdb.h)
int vdb_wit_ann_query_size(int metric, uint32_t P, uint32_t L, size_t K, size_t n_c, size_t dim, uint64_t* cells, uint64_t* lookups, uint64_t* input_cells) {
  return vdb_wit_ann_probe_size(metric, P, L, K, dim, 1, &n_c, 1, cells, lookups, input_cells);
}
int vdb_wit_ann_query(int metric, uint32_t P, uint32_t L, const vdb_fr* query, const vdb_fr* centroids, const vdb_fr* members, const vdb_fr* cluster_roots,
                      size_t K, size_t n_c, size_t dim, vdb_fr* stream_out, vdb_fr* lookup_out, uint8_t* selector_out, vdb_fr* centroid_indicator_out,
                      vdb_fr* member_indicator_out, vdb_fr* public_out) {
  return vdb_wit_ann_probe(metric, P, L, query, centroids, members, cluster_roots, K, dim, 1, &n_c, 1, stream_out, lookup_out, selector_out,
                           centroid_indicator_out, member_indicator_out, public_out);
}
// the one cluster's rows and its resident tree as arrays of one
int vdb_wit_ann_query_dev(int metric, uint32_t P, uint32_t L, const vdb_fr* query_dev, const vdb_fr* centroids_dev, const vdb_fr* members_dev,
                          const vdb_fr* cluster_roots_dev, const vdb_fr* centroid_levels_dev, const vdb_fr* member_levels_dev, size_t K, size_t n_c,
                          size_t dim, vdb_fr* stream_dev, vdb_fr* lookup_dev, uint8_t* selector_dev, vdb_fr* centroid_indicator_dev,
                          vdb_fr* member_indicator_dev, vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(members_dev, "null pointer");
  return vdb_wit_ann_probe_dev(metric, P, L, query_dev, centroids_dev, &members_dev, cluster_roots_dev, centroid_levels_dev, &member_levels_dev, K, dim, 1,
                               &n_c, 1, stream_dev, lookup_dev, selector_dev, centroid_indicator_dev, member_indicator_dev, public_dev);
}

// inserts and replacements against the index root, and the index after them (include/vdb.h)
int vdb_wit_ann_update_size(size_t K, size_t n_c, size_t dim, size_t m, unsigned grow, uint64_t* cells, uint64_t* input_cells, uint64_t* update_base) {
  AnnuLayout a;
  MkuLayout ml;
  TRY(annu_layout(K, 0, n_c, dim, m, grow, &a, &ml));
  if (cells) *cells = a.b.total;
  if (input_cells) *input_cells = a.b.h.n_in;
  if (update_base) *update_base = a.b.b_upd;
  return VDB_OK;
}
int vdb_wit_ann_update_dev(vdb_fr* levels_dev, const vdb_fr* roots_dev, size_t K, size_t cluster, size_t n_c, size_t dim, unsigned grow,
                           const vdb_fr* new_vectors_dev, const uint64_t* indices, size_t m, vdb_fr* stream_dev, uint8_t* selector_dev,
                           vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels_dev && roots_dev && new_vectors_dev && indices && stream_dev && public_dev, "null pointer");
  DevStreams ds;
  ds.init(stream_dev, selector_dev);
  TRY(wit_ann_update_dev(as_u256(levels_dev), as_u256(roots_dev), K, cluster, n_c, dim, grow, as_u256(new_vectors_dev), indices, m, ds.st,
                         as_u256(public_dev)));
  return ds.finish();
}
int vdb_wit_ann_update(vdb_fr* levels, const vdb_fr* roots, size_t K, size_t cluster, size_t n_c, size_t dim, unsigned grow, const vdb_fr* new_vectors,
                       const uint64_t* indices, size_t m, vdb_fr* stream_out, uint8_t* selector_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels && roots && new_vectors && indices, "null pointer");
  AnnuLayout a;
  MkuLayout ml;
  TRY(annu_layout(K, cluster, n_c, dim, m, grow, &a, &ml));
  uint64_t lp;
  uint32_t d;
  tree_shape(n_c, &lp, &d);
  lp <<= grow;
  VDB_ARG(annu_track_fill(indices, m, n_c, lp, nullptr, nullptr) == 0, "a write above the cluster's fill at its turn or outside the grown tree");
  DevBuf dv;
  TRY(upload(dv, new_vectors, ml.n_vec * sizeof(u256)));
  return ann_batch_host(levels, lp, roots, K, a.b.total, 3 * m + 3, stream_out, selector_out, public_out, [&](u256* dl, const u256* dr, Streams st, u256* dpub) {
    return wit_ann_update_dev(dl, dr, K, cluster, n_c, dim, grow, dv.as<u256>(), indices, m, st, dpub);
  });
}

// deletes against the index root (include/vdb.h); the index after them: resident.hip
int vdb_wit_ann_delete_size(size_t K, size_t n_c, size_t dim, size_t m, uint64_t* cells, uint64_t* input_cells, uint64_t* update_base, uint64_t* shrink_base,
                            unsigned* shrink) {
  AnnuLayout a;
  MkuLayout ml;
  AnndPlan dp;
  TRY(annd_layout(K, 0, n_c, dim, nullptr, m, &a, &ml, &dp));
  if (cells) *cells = a.b.total;
  if (input_cells) *input_cells = a.b.h.n_in;
  if (update_base) *update_base = a.b.b_upd;
  if (shrink_base) *shrink_base = a.b.b_shr;
  if (shrink) *shrink = dp.shrink;
  return VDB_OK;
}
int vdb_wit_ann_delete_dev(vdb_fr* levels_dev, const vdb_fr* roots_dev, size_t K, size_t cluster, size_t n_c, size_t dim, const uint64_t* slots, size_t m,
                           vdb_fr* stream_dev, uint8_t* selector_dev, vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels_dev && roots_dev && slots && stream_dev && public_dev, "null pointer");
  DevStreams ds;
  ds.init(stream_dev, selector_dev);
  TRY(wit_ann_delete_dev(as_u256(levels_dev), as_u256(roots_dev), K, cluster, n_c, dim, slots, m, ds.st, as_u256(public_dev)));
  return ds.finish();
}
int vdb_wit_ann_delete(vdb_fr* levels, const vdb_fr* roots, size_t K, size_t cluster, size_t n_c, size_t dim, const uint64_t* slots, size_t m,
                       vdb_fr* stream_out, uint8_t* selector_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels && roots && slots, "null pointer");
  AnnuLayout a;
  MkuLayout ml;
  AnndPlan dp;
  TRY(annd_layout(K, cluster, n_c, dim, slots, m, &a, &ml, &dp));
  return ann_batch_host(levels, dp.lp, roots, K, a.b.total, 4 * m + 3, stream_out, selector_out, public_out, [&](u256* dl, const u256* dr, Streams st, u256* dpub) {
    return wit_ann_delete_dev(dl, dr, K, cluster, n_c, dim, slots, m, st, dpub);
  });
}

// moves from one cluster to another against the index root (include/vdb.h); the index after them: resident.hip
int vdb_wit_ann_move_size(size_t K, size_t n_a, size_t n_b, size_t m, uint64_t* cells, uint64_t* input_cells, uint64_t* delete_base, uint64_t* shrink_base,
                          uint64_t* append_base, unsigned* shrink, unsigned* grow) {
  AnnMoveLayout L;
  AnnMovePlan mp;
  TRY(annmv_layout(K, 0, 1, n_a, n_b, -1, nullptr, m, &L, &mp));
  if (cells) *cells = L.b.total;
  if (input_cells) *input_cells = L.b.n_in;
  if (delete_base) *delete_base = L.b.b_upd_a;
  if (shrink_base) *shrink_base = L.b.b_shr;
  if (append_base) *append_base = L.b.b_upd_b;
  if (shrink) *shrink = mp.d.shrink;
  if (grow) *grow = mp.grow;
  return VDB_OK;
}
int vdb_wit_ann_move_dev(vdb_fr* levels_src_dev, vdb_fr* levels_dst_dev, const vdb_fr* roots_dev, size_t K, size_t src, size_t dst, size_t n_a, size_t n_b,
                         unsigned grow, const uint64_t* slots, size_t m, vdb_fr* stream_dev, uint8_t* selector_dev, vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels_src_dev && levels_dst_dev && roots_dev && slots && stream_dev && public_dev, "null pointer");
  VDB_ARG(grow <= 30, "more than 30 doublings");
  DevStreams ds;
  ds.init(stream_dev, selector_dev);
  TRY(wit_ann_move_dev(as_u256(levels_src_dev), as_u256(levels_dst_dev), as_u256(roots_dev), K, src, dst, n_a, n_b, (int)grow, slots, m, ds.st,
                       as_u256(public_dev)));
  return ds.finish();
}
int vdb_wit_ann_move(vdb_fr* levels_src, vdb_fr* levels_dst, const vdb_fr* roots, size_t K, size_t src, size_t dst, size_t n_a, size_t n_b, unsigned grow,
                     const uint64_t* slots, size_t m, vdb_fr* stream_out, uint8_t* selector_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels_src && levels_dst && roots && slots && stream_out && public_out, "null pointer");
  VDB_ARG(grow <= 30, "more than 30 doublings");
  AnnMoveLayout L;
  AnnMovePlan mp;
  TRY(annmv_layout(K, src, dst, n_a, n_b, (int)grow, slots, m, &L, &mp));
  DevBuf da, db, dr, dpub;
  HostStreams hs;
  const size_t n_pub = 6 * m + 4;
  TRY(upload(da, levels_src, 2 * mp.d.lp * sizeof(u256)));
  TRY(upload(db, levels_dst, 2 * mp.glp_b * sizeof(u256)));
  TRY(upload(dr, roots, (K + 1) * sizeof(u256)));
  TRY(dpub.alloc(n_pub * sizeof(u256)));
  TRY(hs.init(L.b.total, 0, selector_out != nullptr));
  TRY(wit_ann_move_dev(da.as<u256>(), db.as<u256>(), dr.as<u256>(), K, src, dst, n_a, n_b, (int)grow, slots, m, hs.st, dpub.as<u256>()));
  TRY(download(public_out, dpub.p, n_pub * sizeof(u256)));
  TRY(download(levels_src, da.p, 2 * mp.d.lp * sizeof(u256)));
  TRY(download(levels_dst, db.p, 2 * mp.glp_b * sizeof(u256)));
  return hs.finish(stream_out, nullptr, selector_out, L.b.total, 0);
}

// linked writes: one batch against the database root and the index root (include/vdb.h); the index after them: resident.hip
int vdb_wit_ann_write_size(size_t K, size_t n_c, size_t n_db, size_t dim, size_t m, size_t appends, uint64_t* cells, uint64_t* input_cells,
                           uint64_t* update_base, uint64_t* update_db_base, unsigned* grow_c, unsigned* grow_db) {
  AnnwLayout L;
  AnnwPlan wp;
  VDB_ARG(n_c > 0 && n_c <= VDB_ANN_MAX_VECTORS && appends <= m, "empty cluster, cluster larger than VDB_ANN_MAX_VECTORS or more appends than writes");
  uint64_t lp, glp;
  uint32_t d, gd;
  tree_shape(n_c, &lp, &d);
  tree_shape(n_c + appends, &glp, &gd);
  TRY(annw_layout(K, 0, n_c, n_db, dim, gd - d, -1, nullptr, appends, nullptr, nullptr, m, &L, &wp));
  if (cells) *cells = L.b.u.total;
  if (input_cells) *input_cells = L.b.u.h.n_in;
  if (update_base) *update_base = L.b.u.b_upd;
  if (update_db_base) *update_db_base = L.b.b_upd_db;
  if (grow_c) *grow_c = gd - d;
  if (grow_db) *grow_db = wp.grow_db;
  return VDB_OK;
}
// the database slots of a batch from the cluster's recorded slots (annw_expand with the slots known): values only, host arrays, no device call
int vdb_ann_write_db_indices(const uint64_t* cluster_slots, size_t n_c, size_t n_db, const uint64_t* indices, size_t m, uint64_t* db_indices, uint64_t* appends,
                             unsigned* grow_db) {
  AnnwPlan wp;
  VDB_ARG(cluster_slots && indices && db_indices, "null pointer");
  VDB_ARG(m > 0 && m <= MKU_MAX_UPDATES, "a batch holds 1 .. VDB_MERKLE_UPDATE_MAX_UPDATES updates");
  VDB_ARG(n_c > 0 && n_db <= VDB_ANN_MAX_VECTORS, "empty cluster or n_db above VDB_ANN_MAX_VECTORS");
  const int rc = annw_expand(cluster_slots, indices, m, n_c, n_db, nullptr, -1, &wp, nullptr);
  VDB_ARG(rc != 1, "a write above the cluster's fill at its turn");
  VDB_ARG(rc != 2, "empty database, or a cluster larger than its database");
  VDB_ARG(rc == 0, "a member's database slot at or above n_db");
  memcpy(db_indices, wp.db_idx.data(), m * sizeof(uint64_t));
  if (appends) *appends = wp.appends;
  if (grow_db) *grow_db = wp.grow_db;
  return VDB_OK;
}
int vdb_wit_ann_write_dev(vdb_fr* levels_c_dev, vdb_fr* levels_db_dev, const vdb_fr* roots_dev, size_t K, size_t cluster, size_t n_c, size_t n_db, size_t dim,
                          unsigned grow_c, unsigned grow_db, const vdb_fr* new_vectors_dev, const uint64_t* indices, const uint64_t* db_indices, size_t m,
                          vdb_fr* stream_dev, uint8_t* selector_dev, vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels_c_dev && levels_db_dev && roots_dev && new_vectors_dev && indices && db_indices && stream_dev && public_dev, "null pointer");
  VDB_ARG(grow_c <= 30 && grow_db <= 30, "more than 30 doublings");
  DevStreams ds;
  ds.init(stream_dev, selector_dev);
  TRY(wit_ann_write_dev(as_u256(levels_c_dev), as_u256(levels_db_dev), as_u256(roots_dev), K, cluster, n_c, n_db, dim, grow_c, (int)grow_db,
                        as_u256(new_vectors_dev), indices, db_indices, m, ds.st, as_u256(public_dev)));
  return ds.finish();
}
int vdb_wit_ann_write(vdb_fr* levels_c, vdb_fr* levels_db, const vdb_fr* roots, size_t K, size_t cluster, size_t n_c, size_t n_db, size_t dim, unsigned grow_c,
                      unsigned grow_db, const vdb_fr* new_vectors, const uint64_t* indices, const uint64_t* db_indices, size_t m, vdb_fr* stream_out,
                      uint8_t* selector_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(levels_c && levels_db && roots && new_vectors && indices && db_indices && stream_out && public_out, "null pointer");
  VDB_ARG(grow_c <= 30 && grow_db <= 30, "more than 30 doublings");
  AnnwLayout L;
  AnnwPlan wp;
  TRY(annw_layout(K, cluster, n_c, n_db, dim, grow_c, (int)grow_db, indices, 0, nullptr, db_indices, m, &L, &wp));
  uint64_t lp_c;
  uint32_t d;
  tree_shape(n_c, &lp_c, &d);
  lp_c <<= grow_c;
  DevBuf dc, db, dr, dv, dpub;
  HostStreams hs;
  const size_t n_pub = L.b.n_pub;
  TRY(upload(dc, levels_c, 2 * lp_c * sizeof(u256)));
  TRY(upload(db, levels_db, 2 * wp.glp_db * sizeof(u256)));
  TRY(upload(dr, roots, (K + 1) * sizeof(u256)));
  TRY(upload(dv, new_vectors, L.me.n_vec * sizeof(u256)));
  TRY(dpub.alloc(n_pub * sizeof(u256)));
  TRY(hs.init(L.b.u.total, 0, selector_out != nullptr));
  TRY(wit_ann_write_dev(dc.as<u256>(), db.as<u256>(), dr.as<u256>(), K, cluster, n_c, n_db, dim, grow_c, (int)grow_db, dv.as<u256>(), indices, db_indices, m,
                        hs.st, dpub.as<u256>()));
  TRY(download(public_out, dpub.p, n_pub * sizeof(u256)));
  TRY(download(levels_c, dc.p, 2 * lp_c * sizeof(u256)));
  TRY(download(levels_db, db.p, 2 * wp.glp_db * sizeof(u256)));
  return hs.finish(stream_out, nullptr, selector_out, L.b.u.total, 0);
}

// the audit of one cluster's routing (include/vdb.h)
int vdb_wit_ann_audit_size(int metric, uint32_t P, uint32_t L, size_t K, size_t n_c, size_t dim, uint64_t* cells, uint64_t* lookups, uint64_t* input_cells) {
  VDB_REQUIRE_INIT();
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  AnnaLayout a;
  TRY(anna_layout(fp, metric, K, 0, n_c, dim, &a));
  if (cells) *cells = a.b.f.total;
  if (lookups) *lookups = a.b.total_l;
  if (input_cells) *input_cells = a.b.f.h.n_in;
  return VDB_OK;
}
int vdb_wit_ann_audit_dev(int metric, uint32_t P, uint32_t L, const vdb_fr* centroids_dev, const vdb_fr* members_dev, const vdb_fr* roots_dev,
                          const vdb_fr* centroid_levels_dev, const vdb_fr* member_levels_dev, size_t K, size_t cluster, size_t n_c, size_t dim,
                          vdb_fr* stream_dev, vdb_fr* lookup_dev, uint8_t* selector_dev, uint8_t* routed_dev, vdb_fr* public_dev) {
  const auto run = [&](FpEntry* fp, const u256* levels_c, const u256* levels_m, Streams st) {
    return wit_ann_audit_dev(fp, metric, as_u256(centroids_dev), as_u256(members_dev), as_u256(roots_dev), levels_c, levels_m, K, cluster, n_c, dim, st, routed_dev, as_u256(public_dev));
  };
  return ann_cluster_dev(P, L, centroids_dev, members_dev, roots_dev, centroid_levels_dev, member_levels_dev, stream_dev, lookup_dev, selector_dev, routed_dev, public_dev, run);
}
int vdb_wit_ann_audit(int metric, uint32_t P, uint32_t L, const vdb_fr* centroids, const vdb_fr* members, const vdb_fr* roots, size_t K, size_t cluster,
                      size_t n_c, size_t dim, vdb_fr* stream_out, vdb_fr* lookup_out, uint8_t* selector_out, uint8_t* routed_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(centroids && members && roots && routed_out && public_out, "null pointer");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  AnnaLayout a;
  TRY(anna_layout(fp, metric, K, cluster, n_c, dim, &a));
  const auto run = [&](const u256* dc, const u256* dm, const u256* dr, Streams st, uint8_t* routed, u256* dpub) {
    return wit_ann_audit_dev(fp, metric, dc, dm, dr, nullptr, nullptr, K, cluster, n_c, dim, st, routed, dpub);
  };
  return ann_cluster_host(centroids, members, roots, K, n_c, dim, a.b.f.total, a.b.total_l, n_c, stream_out, lookup_out, selector_out, routed_out, public_out, run);
}

// the mean audit of one cluster (include/vdb.h)
int vdb_wit_ann_mean_size(uint32_t P, uint32_t L, size_t K, size_t n_c, size_t dim, uint64_t* cells, uint64_t* lookups, uint64_t* input_cells) {
  VDB_REQUIRE_INIT();
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  AnnmLayout a;
  TRY(annm_layout(fp, K, 0, n_c, dim, &a));
  if (cells) *cells = a.b.f.total;
  if (lookups) *lookups = a.b.total_l;
  if (input_cells) *input_cells = a.b.f.h.n_in;
  return VDB_OK;
}
int vdb_wit_ann_mean_dev(uint32_t P, uint32_t L, const vdb_fr* centroids_dev, const vdb_fr* members_dev, const vdb_fr* roots_dev,
                         const vdb_fr* centroid_levels_dev, const vdb_fr* member_levels_dev, size_t K, size_t cluster, size_t n_c, size_t dim,
                         vdb_fr* stream_dev, vdb_fr* lookup_dev, uint8_t* selector_dev, uint8_t* mean_ok_dev, vdb_fr* public_dev) {
  const auto run = [&](FpEntry* fp, const u256* levels_c, const u256* levels_m, Streams st) {
    return wit_ann_mean_dev(fp, as_u256(centroids_dev), as_u256(members_dev), as_u256(roots_dev), levels_c, levels_m, K, cluster, n_c, dim, st, mean_ok_dev, as_u256(public_dev));
  };
  return ann_cluster_dev(P, L, centroids_dev, members_dev, roots_dev, centroid_levels_dev, member_levels_dev, stream_dev, lookup_dev, selector_dev, mean_ok_dev, public_dev, run);
}
int vdb_wit_ann_mean(uint32_t P, uint32_t L, const vdb_fr* centroids, const vdb_fr* members, const vdb_fr* roots, size_t K, size_t cluster, size_t n_c,
                     size_t dim, vdb_fr* stream_out, vdb_fr* lookup_out, uint8_t* selector_out, uint8_t* mean_ok_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(centroids && members && roots && mean_ok_out && public_out, "null pointer");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  AnnmLayout a;
  TRY(annm_layout(fp, K, cluster, n_c, dim, &a));
  const auto run = [&](const u256* dc, const u256* dm, const u256* dr, Streams st, uint8_t* mean_ok, u256* dpub) {
    return wit_ann_mean_dev(fp, dc, dm, dr, nullptr, nullptr, K, cluster, n_c, dim, st, mean_ok, dpub);
  };
  return ann_cluster_host(centroids, members, roots, K, n_c, dim, a.b.f.total, a.b.total_l, dim, stream_out, lookup_out, selector_out, mean_ok_out, public_out, run);
}

// the recentre of one cluster (include/vdb.h)
int vdb_wit_ann_recentre_size(uint32_t P, uint32_t L, size_t K, size_t n_c, size_t dim, uint64_t* cells, uint64_t* lookups, uint64_t* input_cells,
                              uint64_t* update_base) {
  VDB_REQUIRE_INIT();
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  AnnrLayout a;
  TRY(annr_layout(fp, K, 0, n_c, dim, &a));
  if (cells) *cells = a.b.total;
  if (lookups) *lookups = a.b.total_l;
  if (input_cells) *input_cells = a.b.h.n_in;
  if (update_base) *update_base = a.b.b_upd;
  return VDB_OK;
}
int vdb_wit_ann_recentre_dev(uint32_t P, uint32_t L, vdb_fr* centroid_levels_dev, const vdb_fr* members_dev, const vdb_fr* roots_dev,
                             const vdb_fr* member_levels_dev, size_t K, size_t cluster, size_t n_c, size_t dim, vdb_fr* stream_dev, vdb_fr* lookup_dev,
                             uint8_t* selector_dev, vdb_fr* new_centroid_dev, vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(centroid_levels_dev && members_dev && roots_dev && stream_dev && lookup_dev && new_centroid_dev && public_dev, "null pointer");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  DevStreams ds;
  TRY(ds.init(stream_dev, selector_dev, lookup_dev));
  TRY(wit_ann_recentre_dev(fp, as_u256(centroid_levels_dev), as_u256(members_dev), as_u256(roots_dev), member_levels_dev ? as_u256(member_levels_dev) : nullptr, K,
                           cluster, n_c, dim, ds.st, as_u256(new_centroid_dev), as_u256(public_dev)));
  return ds.finish();
}
int vdb_wit_ann_recentre(uint32_t P, uint32_t L, vdb_fr* centroid_levels, const vdb_fr* members, const vdb_fr* roots, size_t K, size_t cluster, size_t n_c,
                         size_t dim, vdb_fr* stream_out, vdb_fr* lookup_out, uint8_t* selector_out, vdb_fr* new_centroid_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(centroid_levels && members && roots && new_centroid_out && public_out, "null pointer");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  AnnrLayout a;
  TRY(annr_layout(fp, K, cluster, n_c, dim, &a));
  uint64_t lp;
  uint32_t d;
  tree_shape(K, &lp, &d);
  DevBuf dl, dm, dr, dnew, dpub;
  HostStreams hs;
  TRY(upload(dl, centroid_levels, 2 * lp * sizeof(u256)));
  TRY(upload(dm, members, n_c * dim * sizeof(u256)));
  TRY(upload(dr, roots, (K + 1) * sizeof(u256)));
  TRY(dnew.alloc(dim * sizeof(u256)));
  TRY(dpub.alloc(3 * sizeof(u256)));
  TRY(hs.init(a.b.total, a.b.total_l, selector_out != nullptr));
  TRY(wit_ann_recentre_dev(fp, dl.as<u256>(), dm.as<u256>(), dr.as<u256>(), nullptr, K, cluster, n_c, dim, hs.st, dnew.as<u256>(), dpub.as<u256>()));
  TRY(download(new_centroid_out, dnew.p, dim * sizeof(u256)));
  TRY(download(public_out, dpub.p, 3 * sizeof(u256)));
  TRY(download(centroid_levels, dl.p, 2 * lp * sizeof(u256)));
  return hs.finish(stream_out, lookup_out, selector_out, a.b.total, a.b.total_l);
}

// the cover of the database by the index (include/vdb.h)
int vdb_wit_ann_cover_size(const uint64_t* cluster_sizes, size_t K, size_t n, uint64_t* cells, uint64_t* input_cells) {
  VDB_REQUIRE_INIT();
  AnncLayout a;
  TRY(annc_layout(cluster_sizes, K, n, &a));
  if (cells) *cells = a.b.total;
  if (input_cells) *input_cells = a.b.n_in;
  return VDB_OK;
}
int vdb_wit_ann_cover_dev(const vdb_fr* db_leaves_dev, const vdb_fr* cluster_leaves_dev, const vdb_fr* centroids_root_dev, const uint64_t* cluster_sizes,
                          size_t K, size_t n, const vdb_fr* db_tree_dev, const vdb_fr* forest_dev, vdb_fr* stream_dev, uint8_t* selector_dev,
                          vdb_fr* public_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(centroids_root_dev && stream_dev && public_dev, "null pointer");
  VDB_ARG(!db_tree_dev == !forest_dev, "the resident database tree and the forest are given together or not at all");
  VDB_ARG(db_tree_dev || (db_leaves_dev && cluster_leaves_dev), "null pointer: without the resident trees the call reads the two leaf arrays");
  DevStreams ds;
  ds.init(stream_dev, selector_dev);
  TRY(wit_ann_cover_dev(db_leaves_dev ? as_u256(db_leaves_dev) : nullptr, cluster_leaves_dev ? as_u256(cluster_leaves_dev) : nullptr,
                        as_u256(centroids_root_dev), cluster_sizes, K, n, db_tree_dev ? as_u256(db_tree_dev) : nullptr,
                        forest_dev ? as_u256(forest_dev) : nullptr, ds.st, as_u256(public_dev)));
  return ds.finish();
}
int vdb_wit_ann_cover(const vdb_fr* db_leaves, const vdb_fr* cluster_leaves, const vdb_fr* centroids_root, const uint64_t* cluster_sizes, size_t K, size_t n,
                      vdb_fr* stream_out, uint8_t* selector_out, vdb_fr* public_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(db_leaves && cluster_leaves && centroids_root && public_out, "null pointer");
  AnncLayout a;
  TRY(annc_layout(cluster_sizes, K, n, &a));
  DevBuf da, db, dc, dpub;
  HostStreams hs;
  TRY(upload(da, db_leaves, n * sizeof(u256)));
  TRY(upload(db, cluster_leaves, n * sizeof(u256)));
  TRY(upload(dc, centroids_root, sizeof(u256)));
  TRY(dpub.alloc(2 * sizeof(u256)));
  TRY(hs.init(a.b.total, 0, selector_out != nullptr));
  TRY(wit_ann_cover_dev(da.as<u256>(), db.as<u256>(), dc.as<u256>(), cluster_sizes, K, n, nullptr, nullptr, hs.st, dpub.as<u256>()));
  TRY(download(public_out, dpub.p, 2 * sizeof(u256)));
  return hs.finish(stream_out, nullptr, selector_out, a.b.total, 0);
}

// the means of all K clusters of a resident index, values only (include/vdb.h): no stream, no window
int vdb_ann_cluster_means_dev(uint32_t P, uint32_t L, const vdb_fr* grouped_dev, const uint64_t* offsets_dev, size_t n, size_t K, size_t dim,
                              vdb_fr* means_dev) {
  VDB_REQUIRE_INIT();
  VDB_ARG(grouped_dev && offsets_dev && means_dev, "null pointer");
  VDB_ARG(K > 0 && K <= VDB_ANN_MAX_CLUSTERS, "K = 0 or K above VDB_ANN_MAX_CLUSTERS");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  std::vector<uint64_t> off(K + 1);   // the kernel's reads rest on the offsets: they are checked on the host before it is launched
  TRY(download(off.data(), offsets_dev, (K + 1) * sizeof(uint64_t)));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  TRY(ann_means_check(off.data(), n, K, dim));
  int* derr;
  TRY(err_word(&derr));
  TRY(ann_means_dev(fp, as_u256(grouped_dev), offsets_dev, K, dim, derr, as_u256(means_dev)));
  return check_err_flag(derr);
}
int vdb_ann_cluster_means(uint32_t P, uint32_t L, const vdb_fr* grouped, const uint64_t* offsets, size_t n, size_t K, size_t dim, vdb_fr* means_out) {
  VDB_REQUIRE_INIT();
  VDB_ARG(grouped && offsets && means_out, "null pointer");
  VDB_ARG(K > 0 && K <= VDB_ANN_MAX_CLUSTERS, "K = 0 or K above VDB_ANN_MAX_CLUSTERS");
  FpEntry* fp;
  TRY(get_fp(P, L, &fp));
  TRY(ann_means_check(offsets, n, K, dim));   // before anything is uploaded
  DevBuf dg, doff, dmeans;
  TRY(upload(dg, grouped, n * dim * sizeof(u256)));
  TRY(upload(doff, offsets, (K + 1) * sizeof(uint64_t)));
  TRY(dmeans.alloc(K * dim * sizeof(u256)));
  int* derr;
  TRY(err_word(&derr));
  TRY(ann_means_dev(fp, dg.as<u256>(), doff.as<uint64_t>(), K, dim, derr, dmeans.as<u256>()));
  TRY(check_err_flag(derr));
  TRY(download(means_out, dmeans.p, K * dim * sizeof(u256)));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  return VDB_OK;
}

}  // extern "C"
