// Probe of the NTT driver's planner (halo2_vectordb_amd/csrc/ntt_plan.hpp: ntt_plan, NttPlan::chunk_cols) on the host, for
// tests/test_ntt_plan_cpu.py, which holds every field to the Python model of tests/ntt_plan_model.py:
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -o ntt_plan_probe tools/ntt_plan_probe.hip
//   ntt_plan_probe --host cases.bin out.bin      calls no HIP runtime function
// The files have the layout of tools/l9_probe.hip with a magic of their own: little-endian uint32 words  MAGIC, number of blocks, then per
// block  op (0), knobs, count  followed by count records.  knobs: max_s | shoup << 8 | spec << 9 | shoup_all << 10 | blk0 << 11.
// A case is a job, 7 words:  log_n, in_len (low, high), n_cols (low, high), vslots, flags — bit 0 scale_ninv, 1 coset_in, 2 has_in_scale,
// 3 coset_out, 4 has_in_tabs, 5 has_srcs, 6 in_place.  A result is NP_OUT words:
//   return code (as uint32), the refusal's message (24 words of bytes, zero padded; all zero when the plan was made)
//   L, needs_scaled_twiddles, chunk_cols(n_cols) (low, high), ckp[9]
//   per pass, NTT_MAX_PASSES times (zero beyond L):  S, log_inner, first, last, coset, s0, ren_mask, ren_out, blk0, scale, coset_out, logG,
//     nprev, prevS[4], tiles, lds_bytes, has_sh_tab, sh_res_log, sh_ns, sh_max_s (as uint32), sa, needs_sh2_tab, needs_tw_rec, kernel,
//     ntt_spec_sh_res_log(S, sa) — the table resolution a specialised k_ntt_pass instantiation of this size takes for itself
// Everything after the message is zero for a refused job.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../halo2_vectordb_amd/csrc/ntt_plan.hpp"
using namespace vdb;

#define NP_MAGIC 0x4E54504Cu
#define NP_IN 7
#define NP_MSG 24
#define NP_PASS 28
#define NP_OUT (1 + NP_MSG + 4 + 9 + NTT_MAX_PASSES * NP_PASS)

static void eval(uint32_t knobs, const uint32_t* in, uint32_t* out) {
  NttKnobs kn;
  kn.max_s = knobs & 0xffu;
  kn.shoup = (knobs >> 8) & 1;
  kn.spec = (knobs >> 9) & 1;
  kn.shoup_all = (knobs >> 10) & 1;
  kn.blk0 = (knobs >> 11) & 1;
  NttJob j;
  j.log_n = in[0];
  j.in_len = (uint64_t)in[1] | (uint64_t)in[2] << 32;
  j.n_cols = (size_t)((uint64_t)in[3] | (uint64_t)in[4] << 32);
  j.vslots = in[5];
  const uint32_t fl = in[6];
  j.scale_ninv = fl & 1;
  j.coset_in = (fl >> 1) & 1;
  j.has_in_scale = (fl >> 2) & 1;
  j.coset_out = (fl >> 3) & 1;
  j.has_in_tabs = (fl >> 4) & 1;
  j.has_srcs = (fl >> 5) & 1;
  j.in_place = (fl >> 6) & 1;
  NttPlan plan;
  const char* why = nullptr;
  const int rc = ntt_plan(j, kn, &plan, &why);
  out[0] = (uint32_t)rc;
  if (rc) {
    const size_t len = strlen(why);
    memcpy(out + 1, why, len < 4 * NP_MSG ? len : 4 * NP_MSG);
    return;
  }
  uint32_t* o = out + 1 + NP_MSG;
  const uint64_t chunk = plan.chunk_cols(j.n_cols);
  *o++ = plan.L;
  *o++ = plan.needs_scaled_twiddles;
  *o++ = (uint32_t)chunk;
  *o++ = (uint32_t)(chunk >> 32);
  for (int k = 0; k < 9; k++) *o++ = plan.ckp[k];
  for (uint32_t l = 0; l < plan.L; l++) {
    const NttPassPlan& p = plan.passes[l];
    uint32_t* q = o + l * NP_PASS;
    *q++ = p.S;
    *q++ = p.log_inner;
    *q++ = p.first;
    *q++ = p.last;
    *q++ = p.coset;
    *q++ = p.s0;
    *q++ = p.ren_mask;
    *q++ = p.ren_out;
    *q++ = p.blk0;
    *q++ = p.scale;
    *q++ = p.coset_out;
    *q++ = p.logG;
    *q++ = p.nprev;
    for (int k = 0; k < NTT_MAX_PASSES; k++) *q++ = p.prevS[k];
    *q++ = p.tiles;
    *q++ = p.lds_bytes;
    *q++ = p.has_sh_tab;
    *q++ = p.sh_res_log;
    *q++ = p.sh_ns;
    *q++ = (uint32_t)p.sh_max_s;
    *q++ = p.sa;
    *q++ = p.needs_sh2_tab;
    *q++ = p.needs_tw_rec;
    *q++ = (uint32_t)p.kernel;
    *q++ = ntt_spec_sh_res_log(p.S, p.sa);
  }
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "--host")) {
    fprintf(stderr, "usage: ntt_plan_probe --host cases.bin out.bin\n");
    return 2;
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f) {
    fprintf(stderr, "ntt_plan_probe: cannot read %s\n", argv[2]);
    return 2;
  }
  std::vector<uint32_t> in;
  {
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
  }
  if (in.size() < 2 || in[0] != NP_MAGIC) {
    fprintf(stderr, "ntt_plan_probe: not a case file\n");
    return 2;
  }
  std::vector<uint32_t> out = {NP_MAGIC, in[1]};
  size_t pos = 2;
  for (uint32_t b = 0; b < in[1]; b++) {
    if (pos + 3 > in.size()) {
      fprintf(stderr, "ntt_plan_probe: truncated case file (block %u)\n", b);
      return 2;
    }
    const uint32_t op = in[pos], knobs = in[pos + 1], n = in[pos + 2];
    pos += 3;
    if (op != 0 || n == 0 || (in.size() - pos) / NP_IN < n) {
      fprintf(stderr, "ntt_plan_probe: bad block %u (op %u, %u cases)\n", b, op, n);
      return 2;
    }
    out.push_back(op);
    out.push_back(knobs);
    out.push_back(n);
    const size_t o0 = out.size();
    out.resize(o0 + (size_t)n * NP_OUT, 0u);
    for (uint32_t t = 0; t < n; t++) eval(knobs, in.data() + pos + (size_t)t * NP_IN, out.data() + o0 + (size_t)t * NP_OUT);
    pos += (size_t)n * NP_IN;
  }
  if (pos != in.size()) {
    fprintf(stderr, "ntt_plan_probe: %zu words after the last block\n", in.size() - pos);
    return 2;
  }
  f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) {
    fprintf(stderr, "ntt_plan_probe: cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
