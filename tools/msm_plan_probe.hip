// Probe of the MSM driver's planner (halo2_vectordb_amd/csrc/msm_plan.hpp: msm_window, msm_plan) on the host, for
// tests/test_msm_plan_cpu.py, which holds every field to the Python model of tests/msm_plan_model.py:
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -o msm_plan_probe tools/msm_plan_probe.hip
//   msm_plan_probe --host cases.bin out.bin      calls no HIP runtime function
// The files have the layout of tools/l9_probe.hip with a magic of their own: little-endian uint32 words  MAGIC, number of blocks, then per
// block  op, knob, count  followed by count records.  knob: MsmKnobs::window.  64-bit values are two words, low first.
//   op 0, 12 words:  k, window_bits, n, n_cols, free_bytes, held_bytes, cap_bytes       the table's shape from msm_window
//   op 1, 15 words:  c, W, B, table_n, n, n_cols, free_bytes, held_bytes, cap_bytes     a shape as given (no table has it: msm_plan's own refusals)
// A result is MP_OUT words:
//   return code of msm_window, of msm_plan (as uint32), the refusal's message (24 words of bytes, zero padded; all zero without one)
//   c, W, B, table_n                                                               zero from here on when msm_window refused
//   lcap, ent_cap, range_cap_col, seg_cap_col, seg_cap, range_cap, idx_bits, fine_bits, bin_cap, scatter2_bins_x, sort_lds, scatter2_lds,
//   combine_passes, nb, n_batches, bytes, off[MSM_N_REGIONS]                       zero when msm_plan refused
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../halo2_vectordb_amd/csrc/msm_plan.hpp"
using namespace vdb;

#define MP_MAGIC 0x4D53504Cu
#define MP_MSG 24
#define MP_OUT (2 + MP_MSG + 5 + 1 + 6 + 2 + 4 + 3 + 6 + 2 * MSM_N_REGIONS)
static const uint32_t MP_IN[2] = {12, 15};

static uint64_t get64(const uint32_t*& in) {
  const uint64_t v = (uint64_t)in[0] | (uint64_t)in[1] << 32;
  in += 2;
  return v;
}
static void put64(uint32_t*& o, uint64_t v) {
  *o++ = (uint32_t)v;
  *o++ = (uint32_t)(v >> 32);
}
static void put_msg(uint32_t* out, const char* why) {
  const size_t len = strlen(why);
  memcpy(out + 2, why, len < 4 * MP_MSG ? len : 4 * MP_MSG);
}

static void eval(uint32_t op, uint32_t knob, const uint32_t* in, uint32_t* out) {
  MsmKnobs kn;
  kn.window = knob;
  MsmShape s;
  const char* why = nullptr;
  if (op == 0) {
    const uint32_t k = *in++, window_bits = *in++;
    const int rc = msm_window(k, window_bits, kn, &s, &why);
    out[0] = (uint32_t)rc;
    if (rc) {
      put_msg(out, why);
      return;
    }
  } else {
    s.c = *in++;
    s.W = *in++;
    s.B = *in++;
    s.table_n = (size_t)get64(in);
  }
  MsmJob j;
  j.n = (size_t)get64(in);
  j.n_cols = (size_t)get64(in);
  MsmMem mem;
  mem.free_bytes = (size_t)get64(in);
  mem.held_bytes = (size_t)get64(in);
  mem.cap_bytes = (size_t)get64(in);
  uint32_t* o = out + 2 + MP_MSG;
  *o++ = s.c;
  *o++ = s.W;
  *o++ = s.B;
  put64(o, s.table_n);
  MsmPlan P;
  const int rc = msm_plan(s, j, mem, &P, &why);
  out[1] = (uint32_t)rc;
  if (rc) {
    put_msg(out, why);
    return;
  }
  *o++ = P.lcap;
  put64(o, P.ent_cap);
  put64(o, P.range_cap_col);
  put64(o, P.seg_cap_col);
  *o++ = P.seg_cap;
  *o++ = P.range_cap;
  *o++ = P.idx_bits;
  *o++ = P.fine_bits;
  *o++ = P.bin_cap;
  *o++ = P.scatter2_bins_x;
  *o++ = P.sort_lds;
  *o++ = P.scatter2_lds;
  *o++ = P.combine_passes;
  put64(o, P.nb);
  put64(o, P.n_batches);
  put64(o, P.bytes);
  for (uint32_t r = 0; r < MSM_N_REGIONS; r++) put64(o, P.off[r]);
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "--host")) {
    fprintf(stderr, "usage: msm_plan_probe --host cases.bin out.bin\n");
    return 2;
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f) {
    fprintf(stderr, "msm_plan_probe: cannot read %s\n", argv[2]);
    return 2;
  }
  std::vector<uint32_t> in;
  {
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
  }
  if (in.size() < 2 || in[0] != MP_MAGIC) {
    fprintf(stderr, "msm_plan_probe: not a case file\n");
    return 2;
  }
  std::vector<uint32_t> out = {MP_MAGIC, in[1]};
  size_t pos = 2;
  for (uint32_t b = 0; b < in[1]; b++) {
    if (pos + 3 > in.size()) {
      fprintf(stderr, "msm_plan_probe: truncated case file (block %u)\n", b);
      return 2;
    }
    const uint32_t op = in[pos], knob = in[pos + 1], n = in[pos + 2];
    pos += 3;
    if (op > 1 || n == 0 || (in.size() - pos) / MP_IN[op] < n) {
      fprintf(stderr, "msm_plan_probe: bad block %u (op %u, %u cases)\n", b, op, n);
      return 2;
    }
    out.push_back(op);
    out.push_back(knob);
    out.push_back(n);
    const size_t o0 = out.size();
    out.resize(o0 + (size_t)n * MP_OUT, 0u);
    for (uint32_t t = 0; t < n; t++) eval(op, knob, in.data() + pos + (size_t)t * MP_IN[op], out.data() + o0 + (size_t)t * MP_OUT);
    pos += (size_t)n * MP_IN[op];
  }
  if (pos != in.size()) {
    fprintf(stderr, "msm_plan_probe: %zu words after the last block\n", in.size() - pos);
    return 2;
  }
  f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) {
    fprintf(stderr, "msm_plan_probe: cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
