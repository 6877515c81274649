// Batched radix-2 NTT over BN254 Fr for gfx950.
//
// Replaces halo2 `arithmetic::best_fft` and `EvaluationDomain::{lagrange_to_coeff, coeff_to_extended}`
// (third-party halo2-axiom, reached from /root/reference/src/scaffold/mod.rs:296).
// Semantics: X[i] = sum_j a[j] * omega^(i*j), natural order in and out.
//
// Structure (MI355X-first, not a port of the CPU recursion):
//   n = m_0 * m_1 * ... * m_{L-1}, every m_l = 2^S_l <= 512.  Pass l performs, for every residue of
//   the other digits, a size-m_l DFT along digit l inside LDS (decimation in frequency, 2 butterflies
//   per thread per stage), multiplies by the inter-pass twiddle omega_{N_l}^(q*i) and writes back.
//   A workgroup owns a tile of m_l x G elements (G*32 B contiguous = whole 128-B lines in HBM).
//   The last pass reads contiguous rows and scatters to the digit-reversed natural-order position,
//   G consecutive outputs per row group so stores are again whole lines.
//   LDS holds the tile as two 16-byte planes with a one-element row pad: conflict-free ds_read_b128 /
//   ds_write_b128 both along rows and along columns.
// Roofline: 64 B/element algorithmic HBM traffic per transform; the kernel is integer-ALU bound
// (one 254-bit Montgomery product per butterfly), see DESIGN.md.
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "limb9.hpp"
#include "ntt_plan.hpp"
#include "shoup_tables.hpp"

namespace vdb {

#define NTT_THREADS 256
#define NTT_TILE 1024

struct NttPass {
  uint32_t log_n, S, log_inner, logG;
  uint32_t nprev;                 // last pass: number of previous passes
  uint32_t prevS[NTT_MAX_PASSES]; // their sizes (S_0 .. S_{L-2})
  uint32_t first;                 // this is pass 0 (input staging rules apply)
  uint32_t coset;                 // 1: multiply input element e by zeta^(e mod 3); 2: by s zeta^(e mod 3) for a scalar s (zeta0 = 32 s);
                                  // 3: by in_tab[slot][e] (32 g^e for the coset shift g of the column's slot: vdb_coeff_to_cosets_dev)
  uint32_t vslots;                // > 0: the launch's columns are virtual — column c transforms input column c / vslots for slot c % vslots
  const u256* in_tab[4];          // coset == 3: the slots' tables of input factors (n entries each)
  uint32_t coset_out;             // last pass: multiply output element e by zeta^-(e mod 3) (extended_to_coeff)
  uint32_t scale;                 // multiply output by n^{-1}
  uint32_t s0;                    // first butterfly stage to run (2 when the top three quarters of every row are zero padding)
  uint64_t in_len;                // elements >= in_len of the input column read as zero
  uint64_t in_stride, out_stride; // column strides (elements)
  uint32_t ren_mask;              // bit i: butterfly step i starts with a carry pass over its operands
  uint32_t ren_out;               // the write-out starts with a carry pass (the last step left limbs a product cannot take)
  uint32_t blk0;                  // the step at stage 2 takes the product-free path for its block 0
  const ColSrc* srcs;             // pass 0 only: columns still lying in a witness stream (null: read `in`)
  uint32_t n_blind;
  uint32_t n_cols;                // columns of this launch
  uint32_t col_group;             // 0: workgroups run column after column; g > 0: inside groups of g columns they run tile
                                  // after tile (the same tile of all g columns back to back), so a tile's 32-B inter-pass
                                  // twiddles and stage twiddles are L2 hits for every column after the first on an XCD
  u256 zeta1, zeta2, fin;         // 32*zeta, 32*zeta^2, 32/n — all mod r, Montgomery (zeta^-1 = zeta^2: the same two serve coset_out)
  u256 zeta0;                     // coset == 2: 32 s (and zeta1, zeta2 carry the factor s too)
  uint32_t ckp[9];                // 14 r as limbs that dominate any normalised operand (see l9_sub)
  // Shoup products for the stage twiddles (shoup_core29, field.hpp): per twiddle index e that is a multiple of 2^sh_res_log the
  // plain residue of omega_m^e and its quotient floor(omega_m^e 2^261 / r), 2 x 9 limbs; null: every product is a Montgomery product
  const uint32_t* sh_tab;
  uint32_t sh_res_log, sh_ns;     // resolution and number of entries (m / 2 >> sh_res_log)
  int32_t sh_max_s;               // radix-4 steps starting at stage s <= sh_max_s find both their stages' twiddles in the table
  // the SA instantiations (VDB_NTT_SHOUP_ALL): every product by a constant is a Shoup product.  No LDS table of Montgomery-form stage
  // twiddles then; the first step's omega_4 comes from the Shoup table, the radix-2 stage's twiddles from sh2_tab in global memory
  const uint32_t* sh2_tab;        // sh_tab's layout at full resolution (m / 2 entries): the radix-2 stage of an odd-size pass
  const uint4* tw_rec;            // non-last pass: tw_inter's entries as (w, w') limbs, 80 B each (k_shoup_records)
  uint32_t zsh[3][18];            // coset == 1, 2: the factors of residues 0, 1, 2 (1 or s; zeta; zeta^2 — times s), plain and quotient
};

__device__ __forceinline__ uint32_t bitrev_s(uint32_t x, uint32_t bits) { return bits ? (__brev(x) >> (32 - bits)) : 0u; }
// nine limbs of a kernel-argument constant
__device__ __forceinline__ L9 kconst(const uint32_t* k) {
  L9 r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = k[i];
  return r;
}
// nine limbs from a global table of 18-word entries (NttPass::sh_tab's layout; 8-byte aligned)
__device__ __forceinline__ void ld_pair18(const uint32_t* e, L9& w, L9& wq) {
  const uint2* q = reinterpret_cast<const uint2*>(e);
  uint32_t t[18];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const uint2 v = q[i];
    t[2 * i] = v.x;
    t[2 * i + 1] = v.y;
  }
#pragma unroll
  for (int i = 0; i < 9; i++) {
    w.l[i] = t[i];
    wq.l[i] = t[9 + i];
  }
}

// products and the final conditional subtraction are over Fr in this file
__device__ __forceinline__ L9 l9_mul(const L9& a, const L9& W) { return l9_mul<Fr>(a, W); }
__device__ __forceinline__ u256 l9_canon(const L9& t) { return l9_canon<Fr>(t); }

struct L9Planes {
  uint4* a;      // limbs 0..3
  uint4* b;      // limbs 4..7
  uint32_t* c;   // limb 8
};
__device__ __forceinline__ L9 lds_get(const L9Planes& P, uint32_t idx) {
  uint4 a = P.a[idx], b = P.b[idx];
  L9 r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  r.l[8] = P.c[idx];
  return r;
}
__device__ __forceinline__ void lds_put(const L9Planes& P, uint32_t idx, const L9& v) {
  P.a[idx] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  P.b[idx] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
  P.c[idx] = v.l[8];
}

// One pass = a size-2^S DFT along one digit of the index for a tile of 2^S x G elements held in LDS as L9.
// Cooley-Tukey butterflies, natural order in, bit-reversed order out: (u, v) -> (u + w v, u - w v) with one twiddle
// per block, w = omega_m^(bitrev(block)).  Stage 0 has w = 1 everywhere (no product).  Values stay lazy: a product
// is normalised and below 1.2 r, sums and differences just add limbs; every third stage starts with a carry pass so
// multiplier inputs stay below 6 * 2^29 per limb and nothing reaches 2^32.  Values stay below 22 r over ten stages.
// `VS`: the first pass of vdb_coeff_to_cosets_dev (virtual columns, the slot's table of input factors) — an instantiation of its own,
// so that the step's transforms carry none of its branches
// `CS` > 0: the pass size is a compile-time constant, and with it the tile shape (G = 1024 / 2^CS), the first stage (`CS0`), the carry
// schedule (`CREN` = NttPass::ren_mask) and the Shoup table's resolution — the host launches such an instantiation for the sizes of
// the prover's transforms (256- and 512-point passes) when the pass's parameters are exactly these, the generic one (CS = 0)
// otherwise.  Every step then knows its stage: LDS offsets are immediates, the steps' variants that the schedule never takes are not
// instantiated, the loops over a thread's elements have constant trip counts.
template <uint32_t CS, uint32_t s, uint32_t step, class F>
__device__ __forceinline__ void ntt_static_steps(F&& f) {
  if constexpr (s < CS) {
    f(std::integral_constant<uint32_t, s>{}, std::integral_constant<uint32_t, step>{});
    ntt_static_steps<CS, (s + 1 < CS ? s + 2 : s + 1), step + 1>(f);
  }
}
// `SA` (specialised instantiations only): every product by a constant is a Shoup product (NttPass::sh_tab, sh2_tab, tw_rec, zsh).  A
// Shoup product of v (limbs below 6.1 * 2^29, the bound every Montgomery operand here already keeps) is below (1 + v / 2^261 + 2^-23) r
// with exactly normalised limbs (shoup_core29) — below 1.14 r for the v < 22 r of these passes, as a Montgomery product by a normalised
// twiddle is (v r / 2^261 + r) — so every limb and value bound of the carry schedule, the 14 r offsets and the stores without a final
// subtraction holds unchanged.
template <bool LAST, bool VS = false, uint32_t CS = 0, uint32_t CS0 = 0, uint32_t CREN = 0, bool SA = false>
__global__ __launch_bounds__(NTT_THREADS) void k_ntt_pass(const u256* __restrict__ in, u256* __restrict__ out,
                                                         const u256* __restrict__ tw, const u256* __restrict__ tw_inter, NttPass p,
                                                         uint32_t tiles_per_col) {
  extern __shared__ uint4 smem[];
  constexpr bool SPEC = CS > 0;
  static_assert(!SA || ((CS == 8 || CS == 9) && !VS), "SA: the 256- and 512-point instantiations, not the virtual-column one");
  const uint32_t S = SPEC ? CS : p.S, P_logG = SPEC ? 10u - CS : p.logG, P_s0 = SPEC ? CS0 : p.s0, P_ren_mask = SPEC ? CREN : p.ren_mask;
  const uint32_t P_sh_res_log = SPEC ? ntt_spec_sh_res_log(CS, SA) : p.sh_res_log, P_sh_ns = SPEC ? ((1u << (CS ? CS - 1 : 0)) >> ntt_spec_sh_res_log(CS, SA)) : p.sh_ns;
  const int32_t P_sh_max_s = SPEC ? (int32_t)CS - 2 - (int32_t)ntt_spec_sh_res_log(CS, SA) : p.sh_max_s;
  const bool P_shoup = SPEC ? true : p.sh_tab != nullptr, P_blk0 = SPEC ? true : p.blk0 != 0;
  const uint32_t m = 1u << S, G = 1u << P_logG, T = m * G;
  const uint32_t row = m + 1, NE = G * row, NW = SA ? 0u : (m / 2 ? m / 2 : 1);
  L9Planes D, W;
  D.a = smem;
  D.b = D.a + NE;
  W.a = D.b + NE;
  W.b = W.a + NW;
  const uint32_t NS = P_shoup ? P_sh_ns : 0;
  L9Planes WS, WQ;
  WS.a = W.b + NW;
  WS.b = WS.a + NS;
  WQ.a = WS.b + NS;
  WQ.b = WQ.a + NS;
  D.c = reinterpret_cast<uint32_t*>(WQ.b + NS);
  W.c = D.c + NE;
  WS.c = W.c + NW;
  WQ.c = WS.c + NS;
  const uint32_t tid = threadIdx.x;
  uint32_t col, tile;
  if (p.col_group == 0) {
    col = blockIdx.x / tiles_per_col;
    tile = blockIdx.x % tiles_per_col;
  } else {
    const uint32_t per_group = p.col_group * tiles_per_col;
    const uint32_t grp = blockIdx.x / per_group, r = blockIdx.x % per_group;
    const uint32_t left = p.n_cols - grp * p.col_group, ncg = left < p.col_group ? left : p.col_group;
    col = grp * p.col_group + r % ncg;
    tile = r / ncg;
  }
  const u256* cin = in + (size_t)(VS ? col / p.vslots : col) * p.in_stride;
  const u256* ctab = nullptr;
  if constexpr (VS) {
    const uint32_t slot = col % p.vslots;
    ctab = slot == 0 ? p.in_tab[0] : (slot == 1 ? p.in_tab[1] : (slot == 2 ? p.in_tab[2] : p.in_tab[3]));
  }
  ColSrc csrc;
  const bool from_src = p.first && p.srcs != nullptr;
  if (from_src) csrc = p.srcs[col];
  u256* cout = out + (size_t)col * p.out_stride;

  // tile geometry
  uint64_t base;      // element index of (j=0, g=0)
  uint64_t jstride;   // index step along j
  uint64_t gstride;   // index step along g
  uint32_t i0 = 0, q0_base = 0, rdig = 0, rest = 1;
  if (!LAST) {
    uint32_t tiles_inner = (1u << p.log_inner) >> P_logG;
    uint32_t o = tile / tiles_inner;
    i0 = (tile % tiles_inner) << P_logG;
    base = ((uint64_t)o << (S + p.log_inner)) + i0;
    jstride = 1ull << p.log_inner;
    gstride = 1;
  } else {
    if (p.nprev == 0) {
      base = 0;
      jstride = 1;
      gstride = 0;
    } else {
      rest = 1u << (p.log_n - S - p.prevS[0]);
      q0_base = (tile / rest) << P_logG;
      rdig = tile % rest;
      base = ((uint64_t)q0_base * rest + rdig) << S;
      jstride = 1;
      gstride = (uint64_t)rest << S;
    }
  }

  // stage twiddles 32 * omega_m^e = tw[e * n/m], as limbs
  if (!SA)
    for (uint32_t e = tid; e < m / 2; e += NTT_THREADS) lds_put(W, e, l9_split(ld256(tw + ((size_t)e << (p.log_n - S)))));
  for (uint32_t e = tid; e < NS; e += NTT_THREADS) {
    L9 ws, wq;
#pragma unroll
    for (int k = 0; k < 9; k++) {
      ws.l[k] = p.sh_tab[18 * e + k];
      wq.l[k] = p.sh_tab[18 * e + 9 + k];
    }
    lds_put(WS, e, ws);
    lds_put(WQ, e, wq);
  }
  // load tile.  With s0 == 2 only the first quarter of every row is data; the two skipped stages would just copy
  // it into the other three quarters.
  const uint32_t mload = m >> P_s0, Tload = mload * G;
  L9 Z0, Z1, Z2;
  if (!VS && p.coset) {
    Z1 = l9_split(p.zeta1);
    Z2 = l9_split(p.zeta2);
    if (p.coset == 2) Z0 = l9_split(p.zeta0);
  }
  for (uint32_t e = tid; e < Tload; e += NTT_THREADS) {
    uint32_t j, g;
    if (!LAST) {
      g = e & (G - 1);
      j = e >> P_logG;
    } else {
      j = e & (mload - 1);
      g = e / mload;
    }
    uint64_t idx = base + j * jstride + g * gstride;
    L9 v;
    if (!p.first || idx < p.in_len) {
      v = l9_split(from_src ? colsrc_fetch(csrc, idx, 1ull << p.log_n, p.n_blind) : ld256(cin + idx));
      if constexpr (VS) {
        v = l9_mul(v, l9_split(ld256(ctab + idx)));
      } else if (SA && p.coset) {
        // a loaded value is canonical: the product is below 1.01 r
        const uint32_t r3 = (uint32_t)(idx % 3);
        if (r3 == 1) v = l9_mul_shoup<Fr>(v, kconst(p.zsh[1]), kconst(p.zsh[1] + 9));
        else if (r3 == 2) v = l9_mul_shoup<Fr>(v, kconst(p.zsh[2]), kconst(p.zsh[2] + 9));
        else if (p.coset == 2) v = l9_mul_shoup<Fr>(v, kconst(p.zsh[0]), kconst(p.zsh[0] + 9));
      } else if (p.coset) {
        uint32_t r3 = (uint32_t)(idx % 3);
        if (r3 == 1) v = l9_mul(v, Z1);
        else if (r3 == 2) v = l9_mul(v, Z2);
        else if (p.coset == 2) v = l9_mul(v, Z0);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 9; k++) v.l[k] = 0;
    }
    for (uint32_t rep = 0; rep < (1u << P_s0); rep++) lds_put(D, g * row + j + rep * mload, v);
  }
  __syncthreads();
  // butterfly steps: two stages at a time on four elements held in registers (one LDS round trip and one barrier
  // per two stages), a single radix-2 stage at the end when the number of stages is odd
  // SA, odd S: the radix-2 stage's (w, w') from global memory.  Its 2^(S-1) G butterflies are 2 per thread with the same block —
  // b & (m / 2 - 1) == tid when m / 2 == NTT_THREADS — so one entry per thread, fetched at the start of the step before, whose
  // butterflies hide the latency
  L9 r2w, r2q;
  auto do_step = [&](auto s_c, auto step_c) {
    const uint32_t s = s_c, step = step_c;
    const uint32_t logh = S - 1 - s, h = 1u << logh;
    const bool ren = (P_ren_mask >> step) & 1;
    if (SA && (S & 1) && s + 3 == S) ld_pair18(p.sh2_tab + 18 * bitrev_s(tid & ((m >> 1) - 1), S - 1), r2w, r2q);
    if (s + 1 < S) {
      const uint32_t h2 = h >> 1, lh1 = logh ? logh - 1 : 0;   // (logh >= 1 here; the guard keeps the dead instantiations of a compile-time schedule well formed)
      // (the body is instantiated per (first step, carry pass) combination: a run-time `if (ren)` inside one body makes the
      // compiler merge the two register sets with ~30 moves per step on the path that does not renormalise)
      // `s2_c`: the step that starts at stage 2.  Its block 0 — a quarter of its butterflies — has the twiddles of the very first step
      // (1, 1 and omega_4): three of its four products are products by one.  The threads are numbered block-major there (block,
      // row, position), so that with 1024-element tiles a wavefront lies inside one block and the branch costs nothing.
      auto radix4 = [&](auto first_c, auto ren_c, auto shoup_c, auto s2_c) {
        constexpr bool FIRST = decltype(first_c)::value, REN = decltype(ren_c)::value, SHOUP = decltype(shoup_c)::value, S2 = decltype(s2_c)::value;
        for (uint32_t t = tid; t < T / 4; t += NTT_THREADS) {
          uint32_t g, r, blk;
          if (S2) {
            const uint32_t lb = P_logG + lh1;   // log2(threads per block) = log2(G h2)
            // (rotated by the workgroup's number: a CU's resident workgroups then put their light wavefront on different SIMDs)
            blk = ((t >> lb) + blockIdx.x + (blockIdx.x >> 8)) & 3u;
            g = (t >> lh1) & (G - 1);
            r = t & (h2 - 1);
          } else {
            const uint32_t gi = t & ((m >> 2) - 1);
            g = t >> (S - 2);
            r = gi & (h2 - 1);
            blk = gi >> lh1;
          }
          const uint32_t j0 = g * row + (blk << (logh + 1)) + r;
          L9 x0 = lds_get(D, j0), x1 = lds_get(D, j0 + h2), x2 = lds_get(D, j0 + h), x3 = lds_get(D, j0 + h + h2);
          if (REN) {
            l9_renorm(x0);
            l9_renorm(x1);
            l9_renorm(x2);
            l9_renorm(x3);
          }
          if (FIRST) {
            // stage 0: every twiddle is 1.  stage 1: block 0 has twiddle 1, block 1 has omega_4.
            // x2, x3 are subtracted as loaded: exactly normalised, because the carry bit is never set for the step that starts at stage 0
            // (ntt_dev refuses such a schedule)
            L9 a0 = l9_add(x0, x2), a2 = l9_sub(x0, x2, p.ckp);
            L9 a1 = l9_add(x1, x3), a3 = l9_sub(x1, x3, p.ckp);
            l9_carry(a1);  // a1 is subtracted below: its limbs must be below 2^29 again
            L9 t3;
            if (SA) {
              // omega_4 from the Shoup table (index m / 4 is a multiple of its resolution), which is in LDS before the first barrier
              const uint32_t iq = (m >> 2) >> P_sh_res_log;
              t3 = l9_mul_shoup<Fr>(a3, lds_get(WS, iq), lds_get(WQ, iq));
            } else {
              t3 = l9_mul(a3, lds_get(W, m >> 2));
            }
            x0 = l9_add(a0, a1);
            x1 = l9_sub(a0, a1, p.ckp);
            x2 = l9_add(a2, t3);
            x3 = l9_sub(a2, t3, p.ckp);
          } else if (S2 && blk == 0) {
            // twiddles 1, 1, omega_4.  x2, x3 and a1 are subtracted as they are: their limbs are brought below 2^29 first (their values,
            // at most 4.8 r and 9.6 r — block 0 holds the sums of sums of the first step, or freshly loaded values — stay below the
            // 13 r the offset covers); every limb bound stays below the general path's
            l9_carry(x2);
            l9_carry(x3);
            L9 a0 = l9_add(x0, x2), a2 = l9_sub(x0, x2, p.ckp);
            L9 a1 = l9_add(x1, x3), a3 = l9_sub(x1, x3, p.ckp);
            l9_carry(a1);
            L9 t3;
            if (SHOUP) {
              const uint32_t iq = (m >> 2) >> P_sh_res_log;
              t3 = l9_mul_shoup<Fr>(a3, lds_get(WS, iq), lds_get(WQ, iq));
            } else {
              t3 = l9_mul(a3, lds_get(W, m >> 2));
            }
            x0 = l9_add(a0, a1);
            x1 = l9_sub(a0, a1, p.ckp);
            x2 = l9_add(a2, t3);
            x3 = l9_sub(a2, t3, p.ckp);
          } else if (SHOUP) {
            // both stages' twiddles lie in the quarter- (or full-) resolution table of plain residues and quotients: the products
            // come out below 3 r with normalised limbs, which is all the sums and differences below ask of them
            const uint32_t e = bitrev_s(blk, s) << logh, rl = P_sh_res_log;
            const uint32_t i0 = e >> rl, i1 = (e >> 1) >> rl, i2 = ((e >> 1) + (m >> 2)) >> rl;
            const L9 ws = lds_get(WS, i0), wq = lds_get(WQ, i0);
            const L9 t2 = l9_mul_shoup<Fr>(x2, ws, wq), t3 = l9_mul_shoup<Fr>(x3, ws, wq);
            const L9 a0 = l9_add(x0, t2), a2 = l9_sub(x0, t2, p.ckp);
            const L9 a1 = l9_add(x1, t3), a3 = l9_sub(x1, t3, p.ckp);
            const L9 u1 = l9_mul_shoup<Fr>(a1, lds_get(WS, i1), lds_get(WQ, i1));
            const L9 u3 = l9_mul_shoup<Fr>(a3, lds_get(WS, i2), lds_get(WQ, i2));
            x0 = l9_add(a0, u1);
            x1 = l9_sub(a0, u1, p.ckp);
            x2 = l9_add(a2, u3);
            x3 = l9_sub(a2, u3, p.ckp);
          } else {
            const uint32_t e = bitrev_s(blk, s) << logh;
            const L9 w = lds_get(W, e);
            const L9 t2 = l9_mul(x2, w), t3 = l9_mul(x3, w);
            const L9 a0 = l9_add(x0, t2), a2 = l9_sub(x0, t2, p.ckp);
            const L9 a1 = l9_add(x1, t3), a3 = l9_sub(x1, t3, p.ckp);
            const L9 u1 = l9_mul(a1, lds_get(W, e >> 1));
            const L9 u3 = l9_mul(a3, lds_get(W, (e >> 1) + (m >> 2)));
            x0 = l9_add(a0, u1);
            x1 = l9_sub(a0, u1, p.ckp);
            x2 = l9_add(a2, u3);
            x3 = l9_sub(a2, u3, p.ckp);
          }
          lds_put(D, j0, x0);
          lds_put(D, j0 + h2, x1);
          lds_put(D, j0 + h, x2);
          lds_put(D, j0 + h + h2, x3);
        }
      };
      using T_ = std::true_type;
      using F_ = std::false_type;
      const bool s2 = s == 2 && !ren && P_blk0;   // (the schedule never carries at the start of this step; if it ever did: the general body)
      if (s == 0) {
        if (ren) radix4(T_{}, T_{}, F_{}, F_{});
        else radix4(T_{}, F_{}, F_{}, F_{});
      } else if (P_shoup && (int32_t)s <= P_sh_max_s) {
        if (ren) radix4(F_{}, T_{}, T_{}, F_{});
        else if (s2) radix4(F_{}, F_{}, T_{}, T_{});
        else radix4(F_{}, F_{}, T_{}, F_{});
      } else {
        if (ren) radix4(F_{}, T_{}, F_{}, F_{});
        else if (s2) radix4(F_{}, F_{}, F_{}, T_{});
        else radix4(F_{}, F_{}, F_{}, F_{});
      }
    } else {
      for (uint32_t b = tid; b < T / 2; b += NTT_THREADS) {
        const uint32_t g = b >> (S - 1), pj = b & ((m >> 1) - 1);
        const uint32_t r = pj & (h - 1), blk = pj >> logh, j0 = (blk << (logh + 1)) + r;
        const uint32_t a0 = g * row + j0, a1 = a0 + h;
        L9 u = lds_get(D, a0), v = lds_get(D, a1);
        if (ren) {
          l9_renorm(u);
          l9_renorm(v);
        }
        if (SA) v = l9_mul_shoup<Fr>(v, r2w, r2q);   // (s == S - 1 >= 8 here: blk == pj == tid, the entry fetched above)
        else if (s) v = l9_mul(v, lds_get(W, bitrev_s(blk, s) << logh));
        lds_put(D, a0, l9_add(u, v));
        lds_put(D, a1, l9_sub(u, v, p.ckp));
      }
    }
    __syncthreads();
  };
  if constexpr (SPEC) {
    ntt_static_steps<CS, CS0, 0>(do_step);
  } else {
    uint32_t step = 0;
    for (uint32_t s = P_s0; s < S; step++) {
      do_step(s, step);
      s += (s + 1 < S) ? 2 : 1;
    }
  }
  // write out: the inter-pass twiddle product (or the 1/n product of an inverse transform) brings the value below 2r
  // on its own; a forward transform's last pass reduces without a product (l9_canon_wide)
  L9 FIN, ZO1, ZO2;
  if (LAST && p.scale) FIN = l9_split(p.fin);
  if (LAST && p.coset_out) {
    ZO1 = l9_split(p.zeta2);  // zeta^-1
    ZO2 = l9_split(p.zeta1);  // zeta^-2
  }
  // inter-pass twiddles are fetched for all of the thread's elements up front: on gfx9 a load that follows stores
  // waits for their acknowledgement too (one in-order vmcnt), which would put a store round trip between elements
  constexpr uint32_t EPT = NTT_TILE / NTT_THREADS;
  u256 twv[EPT];
  L9 trw[SA ? EPT : 1], trq[SA ? EPT : 1];   // SA: the records (w, w') instead, already in limbs
  if (!LAST) {
#pragma unroll
    for (uint32_t it = 0; it < EPT; it++) {
      const uint32_t e = tid + it * NTT_THREADS;
      const uint32_t g = e & (G - 1), q = e >> P_logG;
      const uint64_t ex = ((uint64_t)q * ((uint64_t)i0 + g)) << (p.log_n - S - p.log_inner);
      if (e < T) {
        if constexpr (SA) {
          const uint4* rp = p.tw_rec + 5 * ex;
          const uint4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4];
          trw[it] = L9{{r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x}};
          trq[it] = L9{{r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w, r4.x, r4.y}};
        } else {
          twv[it] = ld256(tw_inter + ex);
        }
      }
    }
  }
#pragma unroll
  for (uint32_t it = 0; it < EPT; it++) {
    const uint32_t e = tid + it * NTT_THREADS;
    if (e >= T) break;
    uint32_t g = e & (G - 1), q = e >> P_logG;
    L9 v = lds_get(D, g * row + bitrev_s(q, S));
    if (p.ren_out) l9_renorm(v);
    if (!LAST) {
      if constexpr (SA) v = l9_mul_shoup<Fr>(v, trw[it], trq[it]);
      else v = l9_mul(v, l9_split(twv[it]));
      // below 1.2 r and exactly normalised: stored without the final conditional subtraction (the next pass only needs
      // normalised limbs below 1.9 r)
      st256(cout + base + (uint64_t)q * jstride + g, l9_pack(v));
    } else {
      uint64_t pos;
      if (p.nprev == 0) {
        pos = q;
      } else {
        pos = (uint64_t)q0_base + g;
        uint32_t r = rdig;
        uint32_t shift = 0;
        for (uint32_t l = 0; l < p.nprev; l++) shift += p.prevS[l];
        // peel digits q_{L-2} .. q_1 (least significant first)
        for (int l = (int)p.nprev - 1; l >= 1; l--) {
          shift -= p.prevS[l];
          uint32_t ql = r & ((1u << p.prevS[l]) - 1);
          r >>= p.prevS[l];
          pos += (uint64_t)ql << shift;
        }
        pos += (uint64_t)q << (p.log_n - S);
      }
      if (p.scale) {
        v = l9_mul(v, FIN);  // single-pass inverse transform: 1/n here
        const uint32_t r3 = p.coset_out ? (uint32_t)(pos % 3) : 0u;
        if (r3) v = l9_mul(v, r3 == 1 ? ZO1 : ZO2);
        st256(cout + pos, l9_canon(v));
      } else {
        const uint32_t r3 = p.coset_out ? (uint32_t)(pos % 3) : 0u;
        st256(cout + pos, r3 ? l9_canon(l9_mul(v, r3 == 1 ? ZO1 : ZO2)) : l9_canon_wide(v));
      }
    }
  }
}

// tw[e] = 32 * omega^e for e < n (the factor 32 = 2^261 / 2^256 makes a 9 x 29-bit product with the table entry an
// ordinary Montgomery product, see mont_core29); `m32` is 32 in Montgomery form
__global__ __launch_bounds__(256) void k_twiddles(u256* __restrict__ tw, u256 omega, u256 m32, uint64_t n, uint32_t chunk) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t lo = t * chunk;
  if (lo >= n) return;
  u256 w = mont_pow<Fr>(omega, u256_from_u64(lo));
  for (uint32_t i = 0; i < chunk && lo + i < n; i++) {
    st256(tw + lo + i, fr_mul(w, m32));
    w = fr_mul(w, omega);
  }
}

// `factor`: what every entry is multiplied by — 32 (plain table) or 32 / n (`scaled`: the inter-pass table of an inverse
// transform, which folds the final 1/n into a product that is made anyway)
static const u256* get_twiddles(uint32_t log_n, const u256& omega, const u256& factor, bool scaled, int* err) {
  Context& c = ctx();
  Context::TwKey key{log_n | (scaled ? 0x80000000u : 0u), omega};
  auto it = c.twiddles.find(key);
  if (it != c.twiddles.end()) return it->second;
  uint64_t n = 1ull << log_n;
  u256* tw = nullptr;
  hipError_t e = hipMalloc(&tw, n * sizeof(u256));
  if (e != hipSuccess) {
    *err = hip_fail(e, "hipMalloc(twiddles)", __FILE__, __LINE__);
    return nullptr;
  }
  uint32_t chunk = 16;
  uint64_t threads = (n + chunk - 1) / chunk;
  {
    VDB_PROF("k_twiddles");
    hipLaunchKernelGGL(k_twiddles, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c.stream, tw, omega, factor, n, chunk);
  }
  e = hipGetLastError();
  if (e != hipSuccess) {
    *err = hip_fail(e, "k_twiddles", __FILE__, __LINE__);
    (void)hipFree(tw);
    return nullptr;
  }
  c.twiddles[key] = tw;
  return tw;
}

// Shoup table of one pass size (see NttPass::sh_tab): entry j holds, for e = j << res_log, the plain residue of
// omega_m^e = omega^(e n / m) and floor(that * 2^261 / r), nine 29-bit limbs each.  Built on the host (a few hundred entries, a
// 261-step long division each: shoup_stage_entries), cached per device beside the twiddle tables.
static const uint32_t* get_shoup_table(uint32_t log_n, const u256& omega, uint32_t S, uint32_t res_log, int* err) {
  Context& c = ctx();
  Context::TwKey key{log_n | (S << 8) | (res_log << 16) | 0x40000000u, omega};
  auto it = c.twiddles.find(key);
  if (it != c.twiddles.end()) return reinterpret_cast<const uint32_t*>(it->second);
  const std::vector<uint32_t> tab = shoup_stage_entries(log_n, omega, S, res_log);
  uint32_t* d = nullptr;
  hipError_t e = hipMalloc(&d, tab.size() * sizeof(uint32_t));
  if (e != hipSuccess) {
    *err = hip_fail(e, "hipMalloc(shoup table)", __FILE__, __LINE__);
    return nullptr;
  }
  e = hipMemcpy(d, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    *err = hip_fail(e, "hipMemcpy(shoup table)", __FILE__, __LINE__);
    (void)hipFree(d);
    return nullptr;
  }
  c.twiddles[key] = reinterpret_cast<u256*>(d);
  return d;
}

// The inter-pass records of a twiddle table (NttPass::tw_rec): entry e of `tw` as (c, c') limbs, 80 B (shoup_record_of_tw).  n long
// divisions: built on the device, one lane per entry, once per (log_n, omega, table) and cached beside the table it mirrors.
__global__ __launch_bounds__(256) void k_shoup_records(const u256* __restrict__ tw, uint64_t n, u256 inv32, uint4* __restrict__ rec) {
  const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  uint32_t o[20];
  shoup_record_of_tw(ld256(tw + e), inv32, o);
#pragma unroll
  for (int i = 0; i < 5; i++) rec[5 * e + i] = make_uint4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
}
static const uint4* get_shoup_records(uint32_t log_n, const u256& omega, bool scaled, const u256* tw, int* err) {
  Context& c = ctx();
  Context::TwKey key{log_n | (scaled ? 0x80000000u : 0u) | 0x20000000u, omega};
  auto it = c.twiddles.find(key);
  if (it != c.twiddles.end()) return reinterpret_cast<const uint4*>(it->second);
  const uint64_t n = 1ull << log_n;
  uint4* d = nullptr;
  hipError_t e = hipMalloc(&d, n * 5 * sizeof(uint4));
  if (e != hipSuccess) {
    *err = hip_fail(e, "hipMalloc(shoup records)", __FILE__, __LINE__);
    return nullptr;
  }
  const u256 inv32 = mont_inv<Fr>(host_fr_from_u64(32));
  {
    VDB_PROF("k_shoup_records");
    hipLaunchKernelGGL(k_shoup_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, tw, n, inv32, d);
  }
  e = hipGetLastError();
  if (e != hipSuccess) {
    *err = hip_fail(e, "k_shoup_records", __FILE__, __LINE__);
    (void)hipFree(d);
    return nullptr;
  }
  c.twiddles[key] = reinterpret_cast<u256*>(d);
  return d;
}

static_assert(NTT_PLAN_OK == VDB_OK && NTT_PLAN_REFUSED == VDB_ERR_ARG, "ntt_plan.hpp returns the C ABI's codes");

// The process's settings, read from the environment once
static const NttKnobs& ntt_knobs() {
  static const NttKnobs knobs = [] {
    const auto off = [](const char* name) {
      const char* e = getenv(name);
      return e && e[0] == '0';
    };
    NttKnobs k;
    if (const char* e = getenv("VDB_NTT_MAX_S")) k.max_s = (uint32_t)atoi(e);
    k.shoup = !off("VDB_NTT_SHOUP");
    k.spec = !off("VDB_NTT_SPEC");
    k.shoup_all = !off("VDB_NTT_SHOUP_ALL");
    k.blk0 = !off("VDB_NTT_BLK0");
    return k;
  }();
  return knobs;
}

// One batched transform: the job (ntt_plan.hpp; a caller sets what it asks for by name) with the pointers.  has_in_scale, has_in_tabs,
// has_srcs and in_place are not a caller's to set: ntt_dev derives them from in_scale, in_tabs, srcs and out.
struct NttRun : NttJob {
  u256* data;                            // n_cols columns of in_len elements (n when in_len == 0); null with `srcs`
  u256* out;                             // n_cols columns of n elements; null: the result goes back into data
  u256 omega;
  const ColSrc* srcs = nullptr;          // per column: where it still lies in a witness stream
  uint32_t n_blind = 0;
  const u256* in_scale = nullptr;        // coset_in: the polynomial s p(X) on the coset
  // n_cols counts virtual columns — column c is input column c / vslots multiplied element by element by in_tabs[c % vslots] (the
  // cosets of one polynomial, one after the other in the output)
  const u256* const* in_tabs = nullptr;
  NttRun(u256* data_, u256* out_, size_t n_cols_, uint32_t log_n_, const u256& omega_) : data(data_), out(out_), omega(omega_) {
    n_cols = n_cols_;
    log_n = log_n_;
  }
};

// The kernel argument of a pass as far as its plan fills it; ntt_dev adds the pointers, strides and constants
static NttPass ntt_pass_arg(uint32_t log_n, const NttPassPlan& q) {
  NttPass p;
  memset(&p, 0, sizeof(p));
  p.log_n = log_n;
  p.S = q.S;
  p.log_inner = q.log_inner;
  p.logG = q.logG;
  p.nprev = q.nprev;
  memcpy(p.prevS, q.prevS, sizeof(p.prevS));
  p.first = q.first;
  p.coset = q.coset;
  p.coset_out = q.coset_out;
  p.scale = q.scale;
  p.s0 = q.s0;
  p.ren_mask = q.ren_mask;
  p.ren_out = q.ren_out;
  p.blk0 = q.blk0;
  p.sh_res_log = q.sh_res_log;
  p.sh_ns = q.sh_ns;
  p.sh_max_s = q.sh_max_s;
  return p;
}

// Plans the passes (ntt_plan.hpp), fetches what the plan asks for, and launches them chunk by chunk.
static int ntt_dev(const NttRun& t) {
  if (t.n_cols == 0) return VDB_OK;
  NttJob job = t;
  job.has_in_scale = t.in_scale != nullptr;
  job.has_in_tabs = t.in_tabs != nullptr;
  job.has_srcs = t.srcs != nullptr;
  job.in_place = t.out == nullptr;
  NttPlan plan;
  const char* why = nullptr;
  if (int rc = ntt_plan(job, ntt_knobs(), &plan, &why)) {
    set_error("%s", why);
    return rc;
  }
  Context& c = ctx();
  const uint32_t log_n = t.log_n, L = plan.L;
  const uint64_t n = 1ull << log_n, in_len = t.in_len ? t.in_len : n;
  int err = VDB_OK;
  const u256 m32 = host_fr_from_u64(32);
  const u256* tw = get_twiddles(log_n, t.omega, m32, false, &err);
  if (!tw) return err;
  const u256 fin = t.scale_ninv ? fr_mul(mont_inv<Fr>(host_fr_from_u64(n)), m32) : m32;
  // multi-pass inverse transforms take 1/n with the inter-pass twiddles of pass 0; their last pass then ends like a
  // forward transform's, without a product
  const u256* tw_scaled = tw;
  if (plan.needs_scaled_twiddles) {
    tw_scaled = get_twiddles(log_n, t.omega, fin, true, &err);
    if (!tw_scaled) return err;
  }
  // the coset factors 1, zeta, zeta^2 — for the polynomial s p(X) the scalar rides on them (one more product on a third of the inputs) —
  // as Shoup constants for SA (zsh) and times 32 for the Montgomery products
  u256 zc[3] = {mont_one<Fr>(), host_zeta(), fr_mul(host_zeta(), host_zeta())}, z[3];
  for (int i = 0; i < 3; i++) {
    if (t.in_scale) zc[i] = fr_mul(zc[i], *t.in_scale);
    z[i] = fr_mul(zc[i], m32);
  }

  // the passes' kernel arguments, but for what changes from chunk to chunk
  NttPass args[NTT_MAX_PASSES];
  const u256* twi[NTT_MAX_PASSES];
  for (uint32_t l = 0; l < L; l++) {
    const NttPassPlan& q = plan.passes[l];
    NttPass& p = args[l] = ntt_pass_arg(log_n, q);
    p.vslots = t.vslots;
    for (uint32_t s = 0; s < t.vslots; s++) p.in_tab[s] = t.in_tabs[s];
    p.in_len = in_len;
    p.in_stride = l == 0 ? in_len : n;
    p.out_stride = n;
    p.n_blind = t.n_blind;
    p.zeta0 = z[0];
    p.zeta1 = z[1];
    p.zeta2 = z[2];
    p.fin = fin;
    memcpy(p.ckp, plan.ckp, sizeof(p.ckp));
    twi[l] = (l == 0 && !q.last) ? tw_scaled : tw;
    if (q.has_sh_tab) {
      p.sh_tab = get_shoup_table(log_n, t.omega, q.S, q.sh_res_log, &err);
      if (!p.sh_tab) return err;
    }
    if (q.needs_sh2_tab) {
      p.sh2_tab = get_shoup_table(log_n, t.omega, q.S, 0, &err);
      if (!p.sh2_tab) return err;
    }
    if (q.needs_tw_rec) {
      p.tw_rec = get_shoup_records(log_n, t.omega, twi[l] != tw, twi[l], &err);
      if (!p.tw_rec) return err;
    }
    if (q.sa)
      for (int i = 0; i < 3; i++) shoup_const_of_mont(zc[i], p.zsh[i]);
  }

  const size_t chunk_cols = plan.chunk_cols(t.n_cols);
  u256* scratch = nullptr;
  if (L > 1) {
    scratch = (u256*)scratch_get(3, chunk_cols * n * sizeof(u256));
    if (!scratch) return VDB_ERR_OOM;
  }
  u256* dst = t.out ? t.out : t.data;
  for (size_t c0 = 0; c0 < t.n_cols; c0 += chunk_cols) {
    const size_t nc = t.n_cols - c0 < chunk_cols ? t.n_cols - c0 : chunk_cols;
    for (uint32_t l = 0; l < L; l++) {
      const NttPassPlan& q = plan.passes[l];
      NttPass& p = args[l];
      p.srcs = (l == 0 && t.srcs) ? t.srcs + c0 : nullptr;
      p.n_cols = (uint32_t)nc;
      // non-last passes run tile-major over all columns of the launch: a tile's inter-pass and stage twiddles are L2 hits for every
      // column after the first (measured equal to column-major within noise; 4x less twiddle refetch).  The last pass reads none
      p.col_group = q.last ? 0u : (uint32_t)nc;
      // (with column sources `in` is not read)
      const u256* src = (l > 0 || t.srcs) ? scratch : t.data + (t.vslots ? c0 / t.vslots : c0) * in_len;
      u256* out = q.last ? dst + c0 * n : scratch;
      const dim3 grid((unsigned)(nc * q.tiles));
#define NTT_LAUNCH(...) \
  hipLaunchKernelGGL((k_ntt_pass<__VA_ARGS__>), grid, dim3(NTT_THREADS), q.lds_bytes, c.stream, src, out, tw, twi[l], p, q.tiles)
      {
        VDB_PROF("k_ntt_pass");
        switch (q.kernel) {
          case NTT_K_LAST: NTT_LAUNCH(true, false); break;
          case NTT_K_GENERIC: NTT_LAUNCH(false, false); break;
          case NTT_K_LAST_VS: NTT_LAUNCH(true, true); break;
          case NTT_K_VS: NTT_LAUNCH(false, true); break;
          case NTT_K_LAST_256_SA: NTT_LAUNCH(true, false, 8, 0, 4, true); break;
          case NTT_K_LAST_512_SA: NTT_LAUNCH(true, false, 9, 0, 20, true); break;
          case NTT_K_LAST_256: NTT_LAUNCH(true, false, 8, 0, 4); break;
          case NTT_K_LAST_512: NTT_LAUNCH(true, false, 9, 0, 20); break;
          case NTT_K_VS_256: NTT_LAUNCH(false, true, 8, 0, 4); break;
          case NTT_K_256_SA: NTT_LAUNCH(false, false, 8, 0, 4, true); break;
          case NTT_K_512_PAD_SA: NTT_LAUNCH(false, false, 9, 2, 4, true); break;
          case NTT_K_512_SA: NTT_LAUNCH(false, false, 9, 0, 20, true); break;
          case NTT_K_256: NTT_LAUNCH(false, false, 8, 0, 4); break;
          case NTT_K_512_PAD: NTT_LAUNCH(false, false, 9, 2, 4); break;
          case NTT_K_512: NTT_LAUNCH(false, false, 9, 0, 20); break;
          case NTT_K_COUNT: break;
        }
      }
#undef NTT_LAUNCH
      VDB_LAUNCH_CHECK();
    }
  }
  return VDB_OK;
}

// out[j][i] = sum_t C[j][t] * tab_t[i] * P[t][i]: the pieces of a polynomial of degree below n_slots n from its residues modulo
// X^n - u_t (what an inverse transform of its values on the coset g_t H gives, once coefficient i is divided by g_t^i)
struct CosetMix {
  const u256* tab[4];  // g_t^-i, Montgomery
  u256 c[4][4];
};
__global__ __launch_bounds__(256) void k_cosets_combine(const u256* __restrict__ P, uint64_t n, uint32_t n_slots, CosetMix mx, u256* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u256 v[4];
#pragma unroll
  for (uint32_t t = 0; t < 4; t++)
    if (t < n_slots) v[t] = fr_mul(ld256(P + t * n + i), ld256(mx.tab[t] + i));
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    if (j >= n_slots) break;
    u256 acc = fr_mul(v[0], mx.c[j][0]);
#pragma unroll
    for (uint32_t t = 1; t < 4; t++)
      if (t < n_slots) acc = fr_add(acc, fr_mul(v[t], mx.c[j][t]));
    st256(out + j * n + i, acc);
  }
}

u256 host_coset_shift(uint32_t k, uint32_t t) {
  static const uint32_t rev[4] = {0, 2, 1, 3};
  return fr_mul(host_zeta(), mont_pow<Fr>(host_root_of_unity(k + 2), u256_from_u64(rev[t & 3])));
}

static int host_cols_roundtrip(vdb_fr* const* cols, size_t n_cols, size_t n, u256** dbuf, bool upload) {
  Context& c = ctx();
  size_t bytes = n * sizeof(u256);
  if (upload) {
    *dbuf = (u256*)scratch_get(0, n_cols * bytes);
    if (!*dbuf) return VDB_ERR_OOM;
    for (size_t i = 0; i < n_cols; i++) VDB_HIP(hipMemcpyAsync(*dbuf + i * n, cols[i], bytes, hipMemcpyHostToDevice, c.stream));
  } else {
    for (size_t i = 0; i < n_cols; i++) VDB_HIP(hipMemcpyAsync(cols[i], *dbuf + i * n, bytes, hipMemcpyDeviceToHost, c.stream));
    VDB_HIP(hipStreamSynchronize(c.stream));
  }
  return VDB_OK;
}

}  // namespace vdb

using namespace vdb;

extern "C" {

int vdb_ntt_batch_dev(vdb_fr* cols_dev, size_t n_cols, uint32_t log_n, const vdb_fr* omega, int flags) {
  VDB_REQUIRE_INIT();
  VDB_ARG(cols_dev && omega, "null pointer");
  u256 w;
  memcpy(&w, omega, 32);
  NttRun t(as_u256(cols_dev), nullptr, n_cols, log_n, w);
  t.scale_ninv = (flags & VDB_NTT_INVERSE_SCALE) != 0;
  return ntt_dev(t);
}
int vdb_ntt_batch(vdb_fr* const* cols, size_t n_cols, uint32_t log_n, const vdb_fr* omega, int flags) {
  VDB_REQUIRE_INIT();
  VDB_ARG(cols && omega, "null pointer");
  if (n_cols == 0) return VDB_OK;
  u256* d = nullptr;
  int rc = host_cols_roundtrip(cols, n_cols, (size_t)1 << log_n, &d, true);
  if (rc) return rc;
  rc = vdb_ntt_batch_dev(reinterpret_cast<vdb_fr*>(d), n_cols, log_n, omega, flags);
  if (rc) return rc;
  return host_cols_roundtrip(cols, n_cols, (size_t)1 << log_n, &d, false);
}
int vdb_lagrange_to_coeff_dev(vdb_fr* cols_dev, size_t n_cols, uint32_t k) {
  VDB_REQUIRE_INIT();
  VDB_ARG(cols_dev && k <= 26, "bad argument");
  NttRun t(as_u256(cols_dev), nullptr, n_cols, k, mont_inv<Fr>(host_root_of_unity(k)));
  t.scale_ninv = true;
  return ntt_dev(t);
}
int vdb_lagrange_to_coeff_src_dev(const vdb_colsrc* src_dev, vdb_fr* coeff_dev, size_t n_cols, uint32_t k, uint32_t n_blind) {
  VDB_REQUIRE_INIT();
  VDB_ARG(src_dev && coeff_dev && k <= 26 && k > 10, "bad argument (column sources are supported for k > 10)");
  NttRun t(nullptr, as_u256(coeff_dev), n_cols, k, mont_inv<Fr>(host_root_of_unity(k)));
  t.srcs = reinterpret_cast<const ColSrc*>(src_dev);
  t.n_blind = n_blind;
  t.scale_ninv = true;
  return ntt_dev(t);
}
int vdb_lagrange_to_coeff(vdb_fr* const* cols, size_t n_cols, uint32_t k) {
  VDB_REQUIRE_INIT();
  VDB_ARG(cols, "null pointer");
  if (n_cols == 0) return VDB_OK;
  u256* d = nullptr;
  int rc = host_cols_roundtrip(cols, n_cols, (size_t)1 << k, &d, true);
  if (rc) return rc;
  rc = vdb_lagrange_to_coeff_dev(reinterpret_cast<vdb_fr*>(d), n_cols, k);
  if (rc) return rc;
  return host_cols_roundtrip(cols, n_cols, (size_t)1 << k, &d, false);
}
int vdb_coeff_to_extended_dev(const vdb_fr* coeff_dev, vdb_fr* ext_dev, size_t n_cols, uint32_t k, uint32_t ext_k) {
  VDB_REQUIRE_INIT();
  VDB_ARG(coeff_dev && ext_dev && k + ext_k <= 26, "bad argument");
  NttRun t(const_cast<u256*>(as_u256(coeff_dev)), as_u256(ext_dev), n_cols, k + ext_k, host_root_of_unity(k + ext_k));
  t.in_len = (size_t)1 << k;
  t.coset_in = true;
  return ntt_dev(t);
}
int vdb_coeff_to_extended_scaled_dev(const vdb_fr* coeff_dev, vdb_fr* ext_dev, size_t n_cols, uint32_t k, uint32_t ext_k, const vdb_fr* scale) {
  VDB_REQUIRE_INIT();
  VDB_ARG(coeff_dev && ext_dev && scale && k + ext_k <= 26, "bad argument");
  u256 sv;
  memcpy(&sv, scale, 32);
  NttRun t(const_cast<u256*>(as_u256(coeff_dev)), as_u256(ext_dev), n_cols, k + ext_k, host_root_of_unity(k + ext_k));
  t.in_len = (size_t)1 << k;
  t.coset_in = true;
  t.in_scale = &sv;
  return ntt_dev(t);
}
int vdb_extended_to_coeff_dev(vdb_fr* ext_dev, size_t n_cols, uint32_t k, uint32_t ext_k) {
  VDB_REQUIRE_INIT();
  VDB_ARG(ext_dev && k + ext_k <= 26, "bad argument");
  NttRun t(as_u256(ext_dev), nullptr, n_cols, k + ext_k, mont_inv<Fr>(host_root_of_unity(k + ext_k)));
  t.scale_ninv = true;
  t.coset_out = true;
  return ntt_dev(t);
}
// The cosets of the extended domain one by one ("slots"): slot t of a column is the polynomial on g_t H, H the 2^k-th roots of unity,
// g_t = zeta w_{4n}^(bitrev2(t)) — g_0 = zeta, g_1 = zeta w_{2n}, g_2 = zeta w_{4n}, g_3 = zeta w_{4n}^3: together the 4 n points of
// coeff_to_extended (slot t, row r = point 4 r + bitrev2(t) of the natural order), the first two the coset of 2 n points.  A quotient of
// degree below 3 n is determined on three of them, one of degree below 2 n on two: a quarter / a half of the transform is not made at all.
int vdb_coeff_to_cosets_dev(const vdb_fr* coeff_dev, vdb_fr* cosets_dev, size_t n_cols, uint32_t k, uint32_t n_slots, const vdb_fr* scale_or_null) {
  VDB_REQUIRE_INIT();
  VDB_ARG(coeff_dev && cosets_dev && k + 2 <= 26 && n_slots >= 1 && n_slots <= 4, "bad argument");
  if (n_cols == 0) return VDB_OK;
  Context& c = ctx();
  const uint64_t n = 1ull << k;
  const u256 m32 = host_fr_from_u64(32);
  const u256* tabs[4] = {nullptr, nullptr, nullptr, nullptr};
  int err = VDB_OK;
  if (scale_or_null) {
    // s p(X) on the cosets: the scalar rides on the input factors — tables of this call alone
    u256 sv;
    memcpy(&sv, scale_or_null, 32);
    u256* buf = (u256*)scratch_get(6, (size_t)n_slots * n * sizeof(u256));
    if (!buf) return VDB_ERR_OOM;
    const uint32_t chunk = 16;
    const uint64_t threads = (n + chunk - 1) / chunk;
    for (uint32_t t = 0; t < n_slots; t++) {
      hipLaunchKernelGGL(k_twiddles, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c.stream, buf + t * n, host_coset_shift(k, t), fr_mul(m32, sv), n, chunk);
      tabs[t] = buf + t * n;
    }
    VDB_LAUNCH_CHECK();
  } else {
    for (uint32_t t = 0; t < n_slots; t++) {
      tabs[t] = get_twiddles(k, host_coset_shift(k, t), m32, false, &err);
      if (!tabs[t]) return err;
    }
  }
  NttRun t(const_cast<u256*>(as_u256(coeff_dev)), as_u256(cosets_dev), n_cols * n_slots, k, host_root_of_unity(k));
  t.in_tabs = tabs;
  t.vslots = n_slots;
  return ntt_dev(t);
}
// The way back for ONE polynomial, the quotient: `cosets_dev` holds the numerator's values on the first n_slots cosets ([slot][row];
// overwritten); they are divided by X^n - 1 (a constant per coset), brought back to the residues modulo X^n - g_t^n, and the n_slots
// pieces h_0 .. of n coefficients each of h = sum_j X^(n j) h_j — a polynomial of degree below n_slots n, which is what the caller
// asserts — are solved from the Vandermonde system in u_t = g_t^n (h mod (X^n - u_t) = sum_j u_t^j h_j).
int vdb_cosets_to_coeff_dev(vdb_fr* cosets_dev, vdb_fr* coeff_dev, uint32_t k, uint32_t n_slots) {
  VDB_REQUIRE_INIT();
  VDB_ARG(cosets_dev && coeff_dev && k + 2 <= 26 && n_slots >= 1 && n_slots <= 4, "bad argument");
  Context& c = ctx();
  const uint64_t n = 1ull << k;
  NttRun back(as_u256(cosets_dev), nullptr, n_slots, k, mont_inv<Fr>(host_root_of_unity(k)));
  back.scale_ninv = true;
  if (int rc = ntt_dev(back)) return rc;
  CosetMix mx;
  memset(&mx, 0, sizeof(mx));
  u256 u[4];
  const u256 one = mont_one<Fr>();
  int err = VDB_OK;
  for (uint32_t t = 0; t < n_slots; t++) {
    const u256 g = host_coset_shift(k, t);
    // (tables of plain powers: cached under the base g^-1, which no transform uses as its root)
    mx.tab[t] = get_twiddles(k, mont_inv<Fr>(g), one, false, &err);
    if (!mx.tab[t]) return err;
    u[t] = g;
    for (uint32_t i = 0; i < k; i++) u[t] = fr_mul(u[t], u[t]);
  }
  // column t of the inverse Vandermonde matrix = the coefficients of the Lagrange polynomial L_t over the nodes u; times 1 / (u_t - 1)
  for (uint32_t t = 0; t < n_slots; t++) {
    u256 poly[5] = {one, u256_zero(), u256_zero(), u256_zero(), u256_zero()};  // prod_{s != t} (X - u_s)
    uint32_t deg = 0;
    u256 den = fr_sub(u[t], one);                                               // (u_t - 1) prod_{s != t} (u_t - u_s)
    for (uint32_t s2 = 0; s2 < n_slots; s2++) {
      if (s2 == t) continue;
      for (int d = (int)deg + 1; d >= 0; d--) {
        u256 lower = d > 0 ? poly[d - 1] : u256_zero();
        poly[d] = fr_sub(lower, d <= (int)deg ? fr_mul(poly[d], u[s2]) : u256_zero());
      }
      deg++;
      den = fr_mul(den, fr_sub(u[t], u[s2]));
    }
    const u256 inv = mont_inv<Fr>(den);
    for (uint32_t j = 0; j < n_slots; j++) mx.c[j][t] = fr_mul(poly[j], inv);
  }
  {
    VDB_PROF("k_cosets_combine");
    hipLaunchKernelGGL(k_cosets_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, as_u256(cosets_dev), n, n_slots, mx, as_u256(coeff_dev));
  }
  VDB_LAUNCH_CHECK();
  return VDB_OK;
}
int vdb_coeff_to_extended(const vdb_fr* const* coeff_cols, vdb_fr* const* ext_cols, size_t n_cols, uint32_t k, uint32_t ext_k) {
  VDB_REQUIRE_INIT();
  VDB_ARG(coeff_cols && ext_cols, "null pointer");
  if (n_cols == 0) return VDB_OK;
  Context& c = ctx();
  size_t n = (size_t)1 << k, ne = (size_t)1 << (k + ext_k);
  u256* din = (u256*)scratch_get(0, n_cols * n * sizeof(u256));
  u256* dout = (u256*)scratch_get(1, n_cols * ne * sizeof(u256));
  if (!din || !dout) return VDB_ERR_OOM;
  for (size_t i = 0; i < n_cols; i++) VDB_HIP(hipMemcpyAsync(din + i * n, coeff_cols[i], n * sizeof(u256), hipMemcpyHostToDevice, c.stream));
  int rc = vdb_coeff_to_extended_dev(reinterpret_cast<vdb_fr*>(din), reinterpret_cast<vdb_fr*>(dout), n_cols, k, ext_k);
  if (rc) return rc;
  for (size_t i = 0; i < n_cols; i++) VDB_HIP(hipMemcpyAsync(ext_cols[i], dout + i * ne, ne * sizeof(u256), hipMemcpyDeviceToHost, c.stream));
  VDB_HIP(hipStreamSynchronize(c.stream));
  return VDB_OK;
}

}  // extern "C"
