// Probe of the bucket folding's nine-limb group law (xyzz_add_l9, xyzz_dbl_l9 of halo2_vectordb_amd/csrc/ec_l9.hpp) on the host, for
// tests/test_ecl9_cpu.py, which holds every output to Python integers (tests/l9_model.py) and to the eight-word xyzz_add of ec.hpp, run
// here on the same operands:
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -o ecl9_probe tools/ecl9_probe.hip
//   ecl9_probe --host cases.bin out.bin      the C++ forms; calls no HIP runtime function
// The files have the layout of tools/l9_probe.hip with a magic of their own: little-endian uint32 words  MAGIC, number of blocks, then per
// block  op, field (1 = Fq), count  followed by count records of NIN[op] words (cases) resp. NOUT[op] words (results).  An accumulator is
// 37 words: x y zz zzz as nine limbs each (the 2^261 Montgomery form of the MSM accumulator) and the identity flag; an XYZZ point is
// x y zz zzz as eight words each in the ordinary Montgomery form.
//   op  name           in                     out
//    0  xyzz_add_l9    A B (accumulators)     A + B (accumulator), then the eight-word xyzz_add of A and B brought to XYZZ (32 words)
//    1  xyzz_dbl_l9    A                      2 A (accumulator), then the eight-word xyzz_double of A brought to XYZZ
//    2  fold chain     22 accumulators P_s    the loop of k_msm_reduce with no canonical form in between: running += P_s, total += running;
//                                             running and total after every step (22 x 74 words), then the eight-word total (32 words)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../halo2_vectordb_amd/csrc/ec_l9.hpp"
using namespace vdb;

#define EL9_MAGIC 0x454C3950u
#define EL9_NOPS 3
#define EL9_CHAIN 22
static constexpr uint32_t NIN[EL9_NOPS] = {74, 37, EL9_CHAIN * 37};
static constexpr uint32_t NOUT[EL9_NOPS] = {37 + 32, 37 + 32, EL9_CHAIN * 74 + 32};

static MsmL9Consts consts() {
  MsmL9Consts K;
  l9_offset_limbs<FqParams>(2, K.c2);
  l9_offset_limbs<FqParams>(8, K.c8);
  K.one_rp = to_mont<Fq>(u256_from_u64(32));
  K.to_std = mont_one<Fq>();
  K.to_rp = to_mont<Fq>(u256_from_u64(1024));
  return K;
}
static void get_acc(const uint32_t* p, AccL9& a, bool& ident) {
  for (int k = 0; k < 9; k++) {
    a.x.l[k] = p[k];
    a.y.l[k] = p[9 + k];
    a.zz.l[k] = p[18 + k];
    a.zzz.l[k] = p[27 + k];
  }
  ident = p[36] != 0;
}
static void put_acc(uint32_t* p, const AccL9& a, bool ident) {
  for (int k = 0; k < 9; k++) {
    p[k] = ident ? 0u : a.x.l[k];
    p[9 + k] = ident ? 0u : a.y.l[k];
    p[18 + k] = ident ? 0u : a.zz.l[k];
    p[27 + k] = ident ? 0u : a.zzz.l[k];
  }
  p[36] = ident ? 1u : 0u;
}
// the accumulator as an eight-word XYZZ value (what k_msm_normalise does before it inverts)
static XYZZ to_xyzz(const AccL9& a, bool ident, const MsmL9Consts& K) {
  if (ident) return xyzz_identity();
  const L9 ts = l9_split(K.to_std);
  XYZZ p;
  p.x = l9_canon<Fq>(l9_mul<Fq>(a.x, ts));
  p.y = l9_canon<Fq>(l9_mul<Fq>(a.y, ts));
  p.zz = l9_canon<Fq>(l9_mul<Fq>(a.zz, ts));
  p.zzz = l9_canon<Fq>(l9_mul<Fq>(a.zzz, ts));
  return p;
}
static void put_xyzz(uint32_t* p, const XYZZ& a) {
  for (int k = 0; k < 8; k++) {
    p[k] = a.x.w[k];
    p[8 + k] = a.y.w[k];
    p[16 + k] = a.zz.w[k];
    p[24 + k] = a.zzz.w[k];
  }
}

static void eval(uint32_t op, const uint32_t* in, uint32_t* out, const MsmL9Consts& K) {
  if (op == 0) {
    AccL9 a, b;
    bool ai, bi;
    get_acc(in, a, ai);
    get_acc(in + 37, b, bi);
    XYZZ wa = to_xyzz(a, ai, K);
    xyzz_add(wa, to_xyzz(b, bi, K));
    xyzz_add_l9(a, ai, b, bi, K);
    put_acc(out, a, ai);
    put_xyzz(out + 37, wa);
  } else if (op == 1) {
    AccL9 a;
    bool ai;
    get_acc(in, a, ai);
    const XYZZ wa = xyzz_double(to_xyzz(a, ai, K));
    xyzz_dbl_l9(a, ai, K);
    put_acc(out, a, ai);
    put_xyzz(out + 37, wa);
  } else {
    AccL9 running = {}, total = {};
    bool ri = true, ti = true;
    XYZZ wr = xyzz_identity(), wt = xyzz_identity();
    for (int s = 0; s < EL9_CHAIN; s++) {
      AccL9 p;
      bool pi;
      get_acc(in + 37 * s, p, pi);
      xyzz_add(wr, to_xyzz(p, pi, K));
      xyzz_add(wt, wr);
      xyzz_add_l9(running, ri, p, pi, K);
      xyzz_add_l9(total, ti, running, ri, K);
      put_acc(out + 74 * s, running, ri);
      put_acc(out + 74 * s + 37, total, ti);
    }
    put_xyzz(out + 74 * EL9_CHAIN, wt);
  }
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "--host")) {
    fprintf(stderr, "usage: ecl9_probe --host cases.bin out.bin\n");
    return 2;
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f) {
    fprintf(stderr, "ecl9_probe: cannot read %s\n", argv[2]);
    return 2;
  }
  std::vector<uint32_t> in;
  {
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
  }
  if (in.size() < 2 || in[0] != EL9_MAGIC) {
    fprintf(stderr, "ecl9_probe: not a case file\n");
    return 2;
  }
  const MsmL9Consts K = consts();
  std::vector<uint32_t> out = {EL9_MAGIC, in[1]};
  size_t pos = 2;
  for (uint32_t b = 0; b < in[1]; b++) {
    if (pos + 3 > in.size()) {
      fprintf(stderr, "ecl9_probe: truncated case file (block %u)\n", b);
      return 2;
    }
    const uint32_t op = in[pos], mod = in[pos + 1], n = in[pos + 2];
    pos += 3;
    if (op >= EL9_NOPS || mod != 1 || n == 0 || (in.size() - pos) / NIN[op] < n) {
      fprintf(stderr, "ecl9_probe: bad block %u (op %u, field %u, %u cases)\n", b, op, mod, n);
      return 2;
    }
    out.push_back(op);
    out.push_back(mod);
    out.push_back(n);
    const size_t o0 = out.size();
    out.resize(o0 + (size_t)n * NOUT[op]);
    for (uint32_t t = 0; t < n; t++) eval(op, in.data() + pos + (size_t)t * NIN[op], out.data() + o0 + (size_t)t * NOUT[op], K);
    pos += (size_t)n * NIN[op];
  }
  if (pos != in.size()) {
    fprintf(stderr, "ecl9_probe: %zu words after the last block\n", in.size() - pos);
    return 2;
  }
  f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) {
    fprintf(stderr, "ecl9_probe: cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
