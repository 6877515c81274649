// Probe of the MSM sort's digit code (halo2_vectordb_amd/csrc/msm_digits.hpp: sign fold, signed window digits, the scaled-short record)
// on the host, for tests/test_msm_digits_cpu.py, which holds every output to Python integers:
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -o msm_digits_probe tools/msm_digits_probe.hip
//   msm_digits_probe --host cases.bin out.bin      the C++ forms; calls no HIP runtime function
// The files have the layout of tools/l9_probe.hip with a magic of their own: little-endian uint32 words  MAGIC, number of blocks, then per
// block  op, window bits c (2..14), count  followed by count records.  A case is one canonical scalar below r (eight words).  With
// W = ceil(254 / c) windows a result is 2 (W + 1) + 6 words:
//   full walk     n, then W words: the n callbacks of emit_digits over the folded 256-bit magnitude, in order, unused words zero
//   class         kind (0 zero, 1 short, 2 long), j0, nb', s'  (j0 and nb' for every non-zero scalar, s' for a short one)
//   record        low word, high word (zero unless short)
//   from record   n, then W words: the callbacks of emit_digits_short on the decoded record (n = 0 unless short)
// A callback (window j, digit d, negative) is the word  j << 16 | negative << 15 | d.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../halo2_vectordb_amd/csrc/msm_digits.hpp"
using namespace vdb;

#define MD_MAGIC 0x4D534444u

static void eval(uint32_t c, uint32_t W, const uint32_t* in, uint32_t* out) {
  u256 s;
  for (int k = 0; k < 8; k++) s.w[k] = in[k];
  uint32_t* full = out;
  uint32_t* cls = out + W + 1;
  uint32_t* rec = cls + 4;
  uint32_t* dec = rec + 2;
  if (u256_is_zero(s)) return;  // the kernels skip a zero before any of this
  const bool neg = fold_scalar(s);
  const uint32_t nb = u256_bits(s);
  // a callback past the W-th would be a bug of the walk: count it, keep the first W
  auto put = [W](uint32_t* list) {
    return [list, W](uint32_t j, uint32_t d, bool ng, size_t) {
      if (list[0] < W) list[1 + list[0]] = j << 16 | (ng ? 1u << 15 : 0u) | d;
      list[0]++;
    };
  };
  emit_digits(s, neg, nb, c, W, put(full));
  uint32_t mag, nbs, j0;
  const bool is_short = msm_classify(s, nb, c, msm_recip16(c), msm_short_bits(c), mag, nbs, j0);
  cls[0] = is_short ? 1u : 2u;
  cls[1] = j0;
  cls[2] = nbs;
  cls[3] = mag;
  if (!is_short) return;
  const unsigned long long r = msm_rec_encode(mag, neg, nbs, j0);
  rec[0] = (uint32_t)r;
  rec[1] = (uint32_t)(r >> 32);
  const MsmRec sr = msm_rec_decode(r);
  emit_digits_short(sr.mag, sr.neg, sr.nbs, sr.j0, c, W, put(dec), 0);
}

int main(int argc, char** argv) {
  if (argc != 4 || strcmp(argv[1], "--host")) {
    fprintf(stderr, "usage: msm_digits_probe --host cases.bin out.bin\n");
    return 2;
  }
  FILE* f = fopen(argv[2], "rb");
  if (!f) {
    fprintf(stderr, "msm_digits_probe: cannot read %s\n", argv[2]);
    return 2;
  }
  std::vector<uint32_t> in;
  {
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
  }
  if (in.size() < 2 || in[0] != MD_MAGIC) {
    fprintf(stderr, "msm_digits_probe: not a case file\n");
    return 2;
  }
  std::vector<uint32_t> out = {MD_MAGIC, in[1]};
  size_t pos = 2;
  for (uint32_t b = 0; b < in[1]; b++) {
    if (pos + 3 > in.size()) {
      fprintf(stderr, "msm_digits_probe: truncated case file (block %u)\n", b);
      return 2;
    }
    const uint32_t op = in[pos], c = in[pos + 1], n = in[pos + 2];
    pos += 3;
    if (c < 2 || c > 14 || n == 0 || (in.size() - pos) / 8 < n) {
      fprintf(stderr, "msm_digits_probe: bad block %u (op %u, window bits %u, %u cases)\n", b, op, c, n);
      return 2;
    }
    const uint32_t W = (254 + c - 1) / c, nout = 2 * (W + 1) + 6;
    out.push_back(op);
    out.push_back(c);
    out.push_back(n);
    const size_t o0 = out.size();
    out.resize(o0 + (size_t)n * nout, 0u);
    for (uint32_t t = 0; t < n; t++) eval(c, W, in.data() + pos + (size_t)t * 8, out.data() + o0 + (size_t)t * nout);
    pos += (size_t)n * 8;
  }
  if (pos != in.size()) {
    fprintf(stderr, "msm_digits_probe: %zu words after the last block\n", in.size() - pos);
    return 2;
  }
  f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) {
    fprintf(stderr, "msm_digits_probe: cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
