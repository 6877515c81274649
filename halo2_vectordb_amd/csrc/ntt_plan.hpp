// The plan of a batched NTT: everything ntt_dev (ntt.hip) decides before it touches a pointer — the passes, the carry-pass schedule of
// every pass, its tile shape, LDS and Shoup table sizing, and which k_ntt_pass instantiation runs it — in a header of its own, with no
// HIP runtime call, so that tools/ntt_plan_probe.hip reaches the very function the driver plans with and tests/test_ntt_plan_cpu.py can
// hold it to a Python model (tests/ntt_plan_model.py) and state what the kernels rely on: products take limbs below 6.1 * 2^29, nothing
// reaches 2^32, and the specialised instantiations are launched exactly where their template constants are the plan's.
#pragma once
#include "limb9.hpp"

namespace vdb {

#define NTT_MAX_PASSES 4

// The return codes of ntt_plan: VDB_OK and VDB_ERR_ARG of include/vdb.h (ntt.hip asserts the equality).
constexpr int NTT_PLAN_OK = 0, NTT_PLAN_REFUSED = -3;

// what the LDS budget gives 256- / 512-point passes: the 512-point passes' table at half resolution once the Montgomery-form table
// is gone (SA), which then holds both twiddles of the step at stage 6 too
constexpr uint32_t ntt_spec_sh_res_log(uint32_t cs, bool sa) { return cs == 8 ? 0u : (sa ? 1u : 2u); }

// The process's settings (ntt.hip reads them from the environment once).
struct NttKnobs {
  uint32_t max_s = 9;      // VDB_NTT_MAX_S: the largest pass of a multi-pass transform, 2^4 .. 2^9 points (any other value: 9)
  bool shoup = true;       // VDB_NTT_SHOUP=0: no Shoup table of stage twiddles, every product a Montgomery product
  bool spec = true;        // VDB_NTT_SPEC=0: the generic kernel everywhere
  bool shoup_all = true;   // VDB_NTT_SHOUP_ALL=0: the specialised instantiations with Montgomery products (no SA)
  bool blk0 = true;        // VDB_NTT_BLK0=0: the step at stage 2 multiplies in its block 0 too (generic kernel only)
};

// One transform of 2^log_n points per column, as its caller asks for it.
struct NttJob {
  uint32_t log_n = 0;
  uint64_t in_len = 0;         // elements of an input column (its stride too); the rest reads as zero.  0: n
  bool scale_ninv = false;     // multiply by 1 / n
  bool coset_in = false;       // input element e times zeta^(e mod 3)
  bool has_in_scale = false;   // ... times a scalar as well
  bool coset_out = false;      // output element e times zeta^-(e mod 3)
  uint32_t vslots = 0;         // > 0: virtual columns — column c is input column c / vslots times the table of slot c % vslots
  bool has_in_tabs = false;    // the slots' tables are given
  size_t n_cols = 0;           // columns (virtual ones when vslots > 0; read for their divisibility by vslots alone)
  bool has_srcs = false;       // the columns still lie in a witness stream (ColSrc)
  bool in_place = false;       // no output buffer
};

// One value per k_ntt_pass instantiation the driver launches: <LAST, VS, CS, CS0, CREN, SA>.
enum NttKernel : uint32_t {
  NTT_K_LAST_VS,         // <true, true>
  NTT_K_LAST_256_SA,     // <true, false, 8, 0, 4, true>
  NTT_K_LAST_512_SA,     // <true, false, 9, 0, 20, true>
  NTT_K_LAST_256,        // <true, false, 8, 0, 4>
  NTT_K_LAST_512,        // <true, false, 9, 0, 20>
  NTT_K_LAST,            // <true, false>
  NTT_K_VS_256,          // <false, true, 8, 0, 4>
  NTT_K_VS,              // <false, true>
  NTT_K_256_SA,          // <false, false, 8, 0, 4, true>
  NTT_K_512_PAD_SA,      // <false, false, 9, 2, 4, true>
  NTT_K_512_SA,          // <false, false, 9, 0, 20, true>
  NTT_K_256,             // <false, false, 8, 0, 4>
  NTT_K_512_PAD,         // <false, false, 9, 2, 4>
  NTT_K_512,             // <false, false, 9, 0, 20>
  NTT_K_GENERIC,         // <false, false>
  NTT_K_COUNT
};

// What one pass needs beyond pointers (the fields of the same names in NttPass, ntt.hip, are copies of these).
struct NttPassPlan {
  uint32_t S, log_inner;
  bool first, last;
  uint32_t coset;         // 0: none; 1: zeta^(e mod 3); 2: the same with a scalar; 3: the slot's table
  uint32_t s0;            // first butterfly stage to run (2: the top three quarters of every row are zero padding)
  uint32_t ren_mask;      // bit i: butterfly step i starts with a carry pass
  uint32_t ren_out;       // the write-out starts with a carry pass
  uint32_t blk0;
  uint32_t scale;         // the write-out multiplies by 1 / n (single-pass inverse transforms)
  uint32_t coset_out;
  uint32_t logG;          // a tile is 2^S x 2^logG elements
  uint32_t nprev, prevS[NTT_MAX_PASSES];
  uint32_t tiles;         // per column
  uint32_t lds_bytes;     // dynamic LDS of the launch
  bool has_sh_tab;        // Shoup table of the pass's stage twiddles, at resolution sh_res_log: sh_ns entries in LDS
  uint32_t sh_res_log, sh_ns;
  int32_t sh_max_s;
  bool sa;                // an SA instantiation: every product by a constant is a Shoup product
  bool needs_sh2_tab;     // SA, odd size: the full-resolution table for the radix-2 stage
  bool needs_tw_rec;      // SA, not last: the inter-pass twiddles as 80-B records
  NttKernel kernel;
};

struct NttPlan {
  uint32_t log_n, L, vslots;
  NttPassPlan passes[NTT_MAX_PASSES];
  bool needs_scaled_twiddles;   // multi-pass inverse transforms take 1 / n with the inter-pass twiddles of pass 0
  uint32_t ckp[9];              // 14 r with limbs that dominate a normalised subtrahend (l9_sub)
  // columns of one chunk: multi-pass transforms go through a scratch buffer of at most 2 GiB (one column when a column alone is
  // larger), whole groups of virtual columns
  size_t chunk_cols(size_t n_cols) const {
    if (L == 1) return n_cols;
    size_t max_cols = ((size_t)2 << 30) / (((size_t)1 << log_n) * 32);
    if (max_cols < 1) max_cols = 1;
    size_t chunk = n_cols < max_cols ? n_cols : max_cols;
    if (vslots) chunk = chunk / vslots * vslots ? chunk / vslots * vslots : vslots;
    return chunk;
  }
};

// The carry-pass schedule of one pass of 2^S points from stage s0: limb bounds in units of 2^29 (a sum adds the operands' bounds, a
// difference adds cmax); products need operands below 6.1, nothing may reach 8.  Returns the bound the last step leaves.
static inline double ntt_plan_carries(uint32_t S, uint32_t s0, double cmax, uint32_t* ren_mask) {
  double b = 1.0001;
  uint32_t step = 0;
  *ren_mask = 0;
  for (uint32_t st = s0; st < S; step++) {
    if (st + 1 < S) {
      if (st == 0) {
        b = 1.0 + 2.0 * cmax;
      } else {
        if (b + cmax >= 6.1 || b + 2.0 * cmax >= 7.95) {
          *ren_mask |= 1u << step;
          b = 1.0001;
        }
        b += 2.0 * cmax;
      }
      st += 2;
    } else {
      if (st == 0) {
        b = 1.0 + cmax;
      } else {
        if (b >= 6.1 || b + cmax >= 7.95) {
          *ren_mask |= 1u << step;
          b = 1.0001;
        }
        b += cmax;
      }
      st += 1;
    }
  }
  return b;
}

// NTT_PLAN_OK and the plan, or NTT_PLAN_REFUSED and the reason.  Allocates nothing.
static inline int ntt_plan(const NttJob& j, const NttKnobs& kn, NttPlan* plan, const char** why) {
  const auto refuse = [why](const char* msg) {
    *why = msg;
    return NTT_PLAN_REFUSED;
  };
  const uint32_t log_n = j.log_n, vslots = j.vslots;
  if (log_n > 26) return refuse("ntt: log_n > 26 unsupported");
  const uint64_t n = 1ull << log_n, in_len = j.in_len ? j.in_len : n;
  if (j.in_place && in_len != n) return refuse("ntt: in-place transform needs in_len == n");
  if (vslots && (j.in_place || !j.has_in_tabs || vslots > 4 || j.has_srcs || j.coset_in || j.n_cols % vslots))
    return refuse("ntt: virtual columns need an output buffer and their input tables");
  if (j.has_srcs && (j.in_place || in_len != n || log_n <= 10)) return refuse("ntt: column sources need an output buffer and a multi-pass size");

  NttPlan& P = *plan;
  P.log_n = log_n;
  P.vslots = vslots;
  // pass sizes
  uint32_t L, S[NTT_MAX_PASSES];
  if (log_n <= 10) {
    L = 1;
    S[0] = log_n;
  } else {
    uint32_t ms = kn.max_s >= 4 && kn.max_s <= 9 ? kn.max_s : 9u;
    while ((log_n + ms - 1) / ms > NTT_MAX_PASSES) ms++;  // at most NTT_MAX_PASSES digits
    L = (log_n + ms - 1) / ms;  // passes of up to 512 points: 2^16 = 256 x 256, 2^18 = 512 x 512
    for (uint32_t l = 0; l < L; l++) S[l] = log_n / L + (l < log_n % L ? 1 : 0);
  }
  P.L = L;
  P.needs_scaled_twiddles = j.scale_ninv && L > 1;
  const double cmax = l9_offset_limbs<FrParams>(14, P.ckp);

  uint32_t done_bits = 0;
  for (uint32_t l = 0; l < L; l++) {
    NttPassPlan& p = P.passes[l];
    p = NttPassPlan{};
    p.S = S[l];
    p.log_inner = log_n - done_bits - S[l];
    done_bits += S[l];
    p.first = l == 0;
    p.last = l == L - 1;
    const bool last = p.last, vs = l == 0 && vslots;
    p.coset = (l == 0 && j.coset_in) ? (j.has_in_scale ? 2u : 1u) : (vs ? 3u : 0u);
    p.scale = last && j.scale_ninv && L == 1;
    p.coset_out = last && j.coset_out;
    // zero-padded input (coeff_to_extended): when rows of pass 0 run along the top digit and only their first
    // quarter is data, stages 0 and 1 are pure replication
    p.s0 = (l == 0 && !last && S[0] >= 3 && in_len * 4 <= n) ? 2 : 0;
    const double b = ntt_plan_carries(p.S, p.s0, cmax, &p.ren_mask);
    // the step that starts at stage 0 subtracts its operands as loaded (k_ntt_pass, the FIRST branch and the radix-2 stage of a
    // one-stage pass) and its limb bounds assume exactly normalised input.  The schedule never puts a carry pass in front
    // of it; keep it so.  (Limbs of 2^29 + 7 would still be inside l9_sub's domain for the 14 r offset, but not for every offset:
    // tests/test_l9_cpu.py::test_sub_renormalised_subtrahend)
    if (p.s0 == 0 && (p.ren_mask & 1u)) return refuse("ntt: the carry schedule put a carry pass in front of the step at stage 0");
    // the write-out multiplies (inter-pass twiddle, 1/n, zeta) unless it is a forward transform's last pass, whose reduction
    // carries on its own (l9_canon_wide): a carry pass only when the last step left limbs above what a product takes
    const bool out_mul = !last || p.scale || p.coset_out;
    p.blk0 = kn.blk0 ? 1u : 0u;
    p.ren_out = (out_mul && b >= 6.1) ? 1u : 0u;
    const uint32_t m = 1u << S[l];
    if (L > 1) {
      p.logG = 10 - S[l];  // 1024-element tiles: G = 4 for 256-point, G = 2 for 512-point DFTs
      // a tile cannot be wider than the digit it is cut from: the inner index of a non-last pass, the first digit of the last
      const uint32_t room = last ? S[0] : p.log_inner;
      if (p.logG > room) p.logG = room;
      p.nprev = l;  // only read when last
      for (uint32_t q = 0; q < l; q++) p.prevS[q] = S[q];
    }
    const uint32_t G = 1u << p.logG;
    p.tiles = (uint32_t)(n / ((uint64_t)m * G));
    // the instantiation with this pass's size, first stage, carry schedule and Shoup resolution as compile-time constants when there is
    // one (the 256- and 512-point passes of the prover's transforms), the generic kernel otherwise
    const auto spec_shape = [&](uint32_t cs, uint32_t cs0, uint32_t cren) {
      return kn.spec && L > 1 && p.S == cs && p.s0 == cs0 && p.ren_mask == cren && p.logG == 10 - cs && p.blk0;
    };
    // SA instantiation: a specialised, non-virtual pass, with the 80-B inter-pass records bounded to n <= 2^22 (335 MB)
    p.sa = kn.shoup_all && kn.shoup && !vs && log_n <= 22 && (spec_shape(8, 0, 4) || spec_shape(9, 0, 20) || (!last && spec_shape(9, 2, 4)));
    // (SA holds no Montgomery-form stage twiddles in LDS)
    size_t lds = (size_t)(G * (m + 1) + (p.sa ? 0 : (m / 2 ? m / 2 : 1))) * (2 * 16 + 4);
    // Shoup table in what is left of a third of the CU's LDS (three workgroups per CU stay resident): full resolution for the
    // 256-point passes, a quarter for the 512-point ones (a half under SA); passes too small to have a general radix-4 step do without
    p.sh_max_s = -1;
    if (kn.shoup && S[l] >= 4) {
      const size_t room = (160 * 1024) / 3;
      uint32_t rl = 0;
      while (rl + 2 < S[l] && lds + (size_t)((m / 2) >> rl) * 72 > room) rl++;
      const int32_t max_s = (int32_t)S[l] - 2 - (int32_t)rl;
      if (lds + (size_t)((m / 2) >> rl) * 72 <= room && max_s >= 1) {
        p.has_sh_tab = true;
        p.sh_res_log = rl;
        p.sh_ns = (m / 2) >> rl;
        p.sh_max_s = max_s;
        lds += (size_t)p.sh_ns * 72;
      }
    }
    // what every k_ntt_pass instantiation may ask for without a raised limit
    if (lds > 64 * 1024) return refuse("ntt: a pass needs more than 64 KiB of LDS");
    p.lds_bytes = (uint32_t)lds;
    // a specialised instantiation takes its Shoup table's shape from ntt_spec_sh_res_log, not from its argument
    const auto spec = [&](uint32_t cs, uint32_t cs0, uint32_t cren, bool sa) {
      const uint32_t rl = ntt_spec_sh_res_log(cs, sa);
      return spec_shape(cs, cs0, cren) && p.has_sh_tab && p.sh_res_log == rl && p.sh_ns == ((1u << (cs - 1)) >> rl) &&
             p.sh_max_s == (int32_t)cs - 2 - (int32_t)rl;
    };
    // (the LDS plan above gives the SA resolution to these shapes: tests/test_ntt_plan_cpu.py)
    if (p.sa && !spec(p.S, p.s0, p.ren_mask, true)) return refuse("ntt: SA plan does not match its instantiation");
    p.needs_sh2_tab = p.sa && (S[l] & 1);
    p.needs_tw_rec = p.sa && !last;
    if (last) {
      p.kernel = vs                      ? NTT_K_LAST_VS
                 : p.sa && p.S == 8      ? NTT_K_LAST_256_SA
                 : p.sa                  ? NTT_K_LAST_512_SA
                 : spec(8, 0, 4, false)  ? NTT_K_LAST_256
                 : spec(9, 0, 20, false) ? NTT_K_LAST_512
                                         : NTT_K_LAST;
    } else {
      p.kernel = vs && spec(8, 0, 4, false) ? NTT_K_VS_256
                 : vs                       ? NTT_K_VS
                 : p.sa && p.S == 8         ? NTT_K_256_SA
                 : p.sa && p.s0 == 2        ? NTT_K_512_PAD_SA
                 : p.sa                     ? NTT_K_512_SA
                 : spec(8, 0, 4, false)     ? NTT_K_256
                 : spec(9, 2, 4, false)     ? NTT_K_512_PAD
                 : spec(9, 0, 20, false)    ? NTT_K_512
                                            : NTT_K_GENERIC;
    }
  }
  return NTT_PLAN_OK;
}

}  // namespace vdb
