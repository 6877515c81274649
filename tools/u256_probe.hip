// Probe of the 256-bit integer layer under the witness kernels (the u256_* shifts, masks and bit counts of halo2_vectordb_amd/csrc/field.hpp,
// Gadgets::divmod_u256 and Gadgets::mont_small of gadgets.hpp), primitive by primitive, for tests/test_u256_cpu.py and
// tests/test_gpu_u256.py, which hold every output to Python integers:
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -o u256_probe tools/u256_probe.hip
//   u256_probe --host   cases.bin out.bin    the host compilation of the functions; calls no HIP runtime function
//   u256_probe --device cases.bin out.bin    one plain kernel per op, one thread per case: the device compilation of the very functions
//                                            the witness kernels call
// The files have the layout of tools/l9_probe.hip: little-endian uint32 words  MAGIC, number of blocks, then per block  op, 0, count
// followed by count records of NIN[op] words (cases) resp. NOUT[op] words (results); a u256 is 8 words.
//   op  name            in                out
//    0  u256_shr        a s               a >> s                       s in [0, 255]
//    1  u256_shl        a s               a << s mod 2^256             s in [0, 255]
//    2  u256_shr_small  a s               a >> s                       0 < s < 32
//    3  u256_low_bits   a bits            a mod 2^bits                 any bits (256 and above keep everything)
//    4  u256_bits       a                 bit length, 1 word
//    5  u256_extract    a pos len         1 word                       len <= 32, any pos (256 and above give 0)
//    6  u256_add        a b               sum, carry out
//    7  u256_sub        a b               difference, borrow out
//    8  divmod_u256     a b               q r                          b != 0
//    9  mont_small      v                 v 2^256 mod r                v < 2^24
//   10  from_mont<Fr>, to_mont<Fr> of it    x     x / 2^256 mod r, x   x < r
//   11  mont_inv<Fr>    x                 x^(r - 2) (Montgomery form)  x < r
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../halo2_vectordb_amd/csrc/gadgets.hpp"
using namespace vdb;

#define U2P_MAGIC 0x4c395042u
#define U2P_NOPS 12
static constexpr uint32_t NIN[U2P_NOPS] = {9, 9, 9, 9, 8, 10, 16, 16, 16, 1, 8, 8};
static constexpr uint32_t NOUT[U2P_NOPS] = {8, 8, 8, 8, 1, 1, 9, 9, 16, 8, 16, 8};

HD u256 get8(const uint32_t* p) {
  u256 r;
#pragma unroll
  for (int k = 0; k < 8; k++) r.w[k] = p[k];
  return r;
}
HD void put8(uint32_t* p, const u256& v) {
#pragma unroll
  for (int k = 0; k < 8; k++) p[k] = v.w[k];
}

template <int OP>
HD void eval_hd(const uint32_t* in, uint32_t* out) {
  if constexpr (OP == 0) {
    put8(out, u256_shr(get8(in), in[8]));
  } else if constexpr (OP == 1) {
    put8(out, u256_shl(get8(in), in[8]));
  } else if constexpr (OP == 2) {
    put8(out, u256_shr_small(get8(in), in[8]));
  } else if constexpr (OP == 3) {
    put8(out, u256_low_bits(get8(in), in[8]));
  } else if constexpr (OP == 4) {
    out[0] = u256_bits(get8(in));
  } else if constexpr (OP == 5) {
    out[0] = u256_extract(get8(in), in[8], in[9]);
  } else if constexpr (OP == 6) {
    u256 o;
    out[8] = u256_add(o, get8(in), get8(in + 8));
    put8(out, o);
  } else if constexpr (OP == 7) {
    u256 o;
    out[8] = u256_sub(o, get8(in), get8(in + 8));
    put8(out, o);
  } else if constexpr (OP == 8) {
    u256 q, r;
    Gadgets::divmod_u256(get8(in), get8(in + 8), q, r);
    put8(out, q);
    put8(out + 8, r);
  } else if constexpr (OP == 9) {
    put8(out, Gadgets::mont_small(in[0]));
  } else if constexpr (OP == 10) {
    const u256 c = from_mont<Fr>(get8(in));
    put8(out, c);
    put8(out + 8, to_mont<Fr>(c));
  } else if constexpr (OP == 11) {
    put8(out, mont_inv<Fr>(get8(in)));
  }
}

template <int OP>
__global__ __launch_bounds__(64) void k_eval(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  eval_hd<OP>(in + (size_t)t * NIN[OP], out + (size_t)t * NOUT[OP]);
}

static int hip_bad(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  fprintf(stderr, "u256_probe: %s: %s\n", what, hipGetErrorString(e));
  return 1;
}
template <int OP>
static int run_device(const uint32_t* in, uint32_t* out, uint32_t n) {
  uint32_t *din = nullptr, *dout = nullptr;
  const size_t bi = (size_t)n * NIN[OP] * 4, bo = (size_t)n * NOUT[OP] * 4;
  int bad = hip_bad(hipMalloc(&din, bi), "hipMalloc") || hip_bad(hipMalloc(&dout, bo), "hipMalloc");
  bad = bad || hip_bad(hipMemcpy(din, in, bi, hipMemcpyHostToDevice), "hipMemcpy (in)");
  if (!bad) {
    hipLaunchKernelGGL((k_eval<OP>), dim3((n + 63) / 64), dim3(64), 0, 0, din, dout, n);
    bad = hip_bad(hipGetLastError(), "launch") || hip_bad(hipDeviceSynchronize(), "kernel");
  }
  bad = bad || hip_bad(hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost), "hipMemcpy (out)");
  if (din) bad = hip_bad(hipFree(din), "hipFree") || bad;
  if (dout) bad = hip_bad(hipFree(dout), "hipFree") || bad;
  return bad;
}
template <int OP>
static int run_op(int op, bool device, const uint32_t* in, uint32_t* out, uint32_t n) {
  if constexpr (OP < U2P_NOPS) {
    if (op != OP) return run_op<OP + 1>(op, device, in, out, n);
    if (device) return run_device<OP>(in, out, n);
    for (uint32_t t = 0; t < n; t++) eval_hd<OP>(in + (size_t)t * NIN[OP], out + (size_t)t * NOUT[OP]);
    return 0;
  } else {
    fprintf(stderr, "u256_probe: unknown op %d\n", op);
    return 1;
  }
}

int main(int argc, char** argv) {
  if (argc != 4 || (strcmp(argv[1], "--host") && strcmp(argv[1], "--device"))) {
    fprintf(stderr, "usage: u256_probe --host|--device cases.bin out.bin\n");
    return 2;
  }
  const bool device = !strcmp(argv[1], "--device");
  FILE* f = fopen(argv[2], "rb");
  if (!f) {
    fprintf(stderr, "u256_probe: cannot read %s\n", argv[2]);
    return 2;
  }
  std::vector<uint32_t> in;
  {
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
  }
  if (in.size() < 2 || in[0] != U2P_MAGIC) {
    fprintf(stderr, "u256_probe: not a case file\n");
    return 2;
  }
  std::vector<uint32_t> out = {U2P_MAGIC, in[1]};
  size_t pos = 2;
  for (uint32_t b = 0; b < in[1]; b++) {
    if (pos + 3 > in.size()) {
      fprintf(stderr, "u256_probe: truncated case file (block %u)\n", b);
      return 2;
    }
    const uint32_t op = in[pos], mod = in[pos + 1], n = in[pos + 2];
    pos += 3;
    if (op >= U2P_NOPS || mod != 0 || n == 0 || (in.size() - pos) / NIN[op] < n) {
      fprintf(stderr, "u256_probe: bad block %u (op %u, field %u, %u cases)\n", b, op, mod, n);
      return 2;
    }
    out.push_back(op);
    out.push_back(mod);
    out.push_back(n);
    const size_t o0 = out.size();
    out.resize(o0 + (size_t)n * NOUT[op]);
    if (run_op<0>((int)op, device, in.data() + pos, out.data() + o0, n)) return 1;
    pos += (size_t)n * NIN[op];
  }
  if (pos != in.size()) {
    fprintf(stderr, "u256_probe: %zu words after the last block\n", in.size() - pos);
    return 2;
  }
  f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) {
    fprintf(stderr, "u256_probe: cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
