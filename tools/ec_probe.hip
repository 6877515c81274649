// Probe of the layer between the product cores and the kernels: the 256-bit field helpers of halo2_vectordb_amd/csrc/field.hpp (mod_add ..
// mont_inv, the shifts and bit helpers, k_from_wide's composition) and the u256 XYZZ group law of ec.hpp, function by function, for
// tests/test_ec_cpu.py and tests/test_gpu_ec.py, which hold every output to Python integers (tests/ec_model.py):
//   hipcc -O2 -std=c++17 --offload-arch=gfx950 -o ec_probe tools/ec_probe.hip
//   ec_probe --host   cases.bin out.bin    the C++ forms (the #else branches of field.hpp); calls no HIP runtime function
//   ec_probe --device cases.bin out.bin    one plain kernel per op, one thread per case: the device compilation of the library's own text
// The files have the layout of tools/l9_probe.hip with a magic of their own: little-endian uint32 words  MAGIC, number of blocks, then per
// block  op, field (0 = Fr, 1 = Fq), count  followed by count records of NIN[op] words (cases) resp. NOUT[op] words (results).  A u256 is 8
// words; an affine point is x y (16 words), an XYZZ point x y zz zzz (32 words), coordinates in Montgomery form as the library holds them.
//   op  name                in                            out                                     domain
//    0  mod_add             a b                           a + b mod p                             a, b < p
//    1  mod_sub             a b                           a - b mod p                             a, b < p
//    2  mod_neg             a                             -a mod p                                a < p
//    3  mod_dbl             a                             2 a mod p                               a < p
//    4  mont_mul            a b                           a b 2^-256 mod p                        a < 2^256 (k_from_wide's use), b < p
//    5  to_mont, from_mont  a                             t = to_mont(a), from_mont(t)            a < 2^256
//    6  from_wide           lo hi                         fr_add(to_mont(lo), to_mont(to_mont(hi)))   Fr only; lo, hi < 2^256
//    7  mont_pow            a e                           a^e                                     a < p (Montgomery form), e < 2^256
//    8  mont_inv            a                             a^(p - 2)                               a < p (Montgomery form); 0 -> 0
//    9  u256_shr            a s                           a >> s                                  s in [0, 255]
//   10  u256_shl            a s                           a << s mod 2^256                        s in [0, 255]
//   11  u256_shr_small      a s                           a >> s                                  0 < s < 32
//   12  u256_low_bits       a bits                        a mod 2^bits                            any bits (256 and above keep everything)
//   13  u256_bits           a                             bit length, 1 word
//   14  u256_bit            a i                           bit i, 1 word                           i in [0, 255]
//   15  u256_extract        a pos len                     1 word                                  len <= 32, any pos (256 and above give 0)
//   16  compare, add, sub   a b                           geq, eq, a + b (8), carry, a - b (8), borrow   any a, b
//   17  xyzz_add            A B (XYZZ)                    A + B (XYZZ)                            Fq only, as every op below
//   18  xyzz_add_mixed      A (XYZZ) Q (affine) neg       A +- Q (XYZZ)
//   19  xyzz_double         A (XYZZ)                      2 A (XYZZ)
//   20  xyzz_double_affine  Q (affine)                    2 Q (XYZZ)
//   21  xyzz_from_affine    Q (affine)                    F = from_affine(Q) (XYZZ), to_affine(F) (affine)
//   22  xyzz_to_affine      A (XYZZ)                      affine
//   23  xyzz_mul            A (XYZZ) s                    [s] A (XYZZ)                            s < 2^256
//   24  add_mixed chain     A (XYZZ), 64 x (Q neg)        64 x XYZZ: the accumulator after every step
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../halo2_vectordb_amd/csrc/ec.hpp"
using namespace vdb;

#define ECP_MAGIC 0x45435042u
#define ECP_NOPS 25
#define ECP_CHAIN 64
#define ECP_FIRST_GROUP_OP 17
static constexpr uint32_t NIN[ECP_NOPS] = {16, 16, 8, 8, 16, 8, 16, 16, 8, 9, 9, 9, 9, 8, 9, 10, 16, 64, 49, 32, 16, 16, 32, 40, 32 + ECP_CHAIN * 17};
static constexpr uint32_t NOUT[ECP_NOPS] = {8, 8, 8, 8, 8, 16, 8, 8, 8, 8, 8, 8, 8, 1, 1, 1, 20, 32, 32, 32, 32, 48, 16, 32, ECP_CHAIN * 32};

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
HD Affine get_affine(const uint32_t* p) {
  Affine a;
  a.x = get8(p);
  a.y = get8(p + 8);
  return a;
}
HD void put_affine(uint32_t* p, const Affine& a) {
  put8(p, a.x);
  put8(p + 8, a.y);
}
HD XYZZ get_xyzz(const uint32_t* p) {
  XYZZ a;
  a.x = get8(p);
  a.y = get8(p + 8);
  a.zz = get8(p + 16);
  a.zzz = get8(p + 24);
  return a;
}
HD void put_xyzz(uint32_t* p, const XYZZ& a) {
  put8(p, a.x);
  put8(p + 8, a.y);
  put8(p + 16, a.zz);
  put8(p + 24, a.zzz);
}

template <class M, int OP>
HD void eval_hd(const uint32_t* in, uint32_t* out) {
  if constexpr (OP == 0) {
    put8(out, mod_add<M>(get8(in), get8(in + 8)));
  } else if constexpr (OP == 1) {
    put8(out, mod_sub<M>(get8(in), get8(in + 8)));
  } else if constexpr (OP == 2) {
    put8(out, mod_neg<M>(get8(in)));
  } else if constexpr (OP == 3) {
    put8(out, mod_dbl<M>(get8(in)));
  } else if constexpr (OP == 4) {
    put8(out, mont_mul<M>(get8(in), get8(in + 8)));
  } else if constexpr (OP == 5) {
    const u256 t = to_mont<M>(get8(in));
    put8(out, t);
    put8(out + 8, from_mont<M>(t));
  } else if constexpr (OP == 6) {
    // the body of k_from_wide (core.hip)
    const u256 lo = get8(in), hi = get8(in + 8);
    put8(out, fr_add(to_mont<Fr>(lo), to_mont<Fr>(to_mont<Fr>(hi))));
  } else if constexpr (OP == 7) {
    put8(out, mont_pow<M>(get8(in), get8(in + 8)));
  } else if constexpr (OP == 8) {
    put8(out, mont_inv<M>(get8(in)));
  } else if constexpr (OP == 9) {
    put8(out, u256_shr(get8(in), in[8]));
  } else if constexpr (OP == 10) {
    put8(out, u256_shl(get8(in), in[8]));
  } else if constexpr (OP == 11) {
    put8(out, u256_shr_small(get8(in), in[8]));
  } else if constexpr (OP == 12) {
    put8(out, u256_low_bits(get8(in), in[8]));
  } else if constexpr (OP == 13) {
    out[0] = u256_bits(get8(in));
  } else if constexpr (OP == 14) {
    out[0] = u256_bit(get8(in), in[8]);
  } else if constexpr (OP == 15) {
    out[0] = u256_extract(get8(in), in[8], in[9]);
  } else if constexpr (OP == 16) {
    const u256 a = get8(in), b = get8(in + 8);
    u256 s, d;
    out[0] = u256_geq(a, b) ? 1u : 0u;
    out[1] = u256_eq(a, b) ? 1u : 0u;
    out[10] = u256_add(s, a, b);
    put8(out + 2, s);
    out[19] = u256_sub(d, a, b);
    put8(out + 11, d);
  } else if constexpr (OP == 17) {
    XYZZ acc = get_xyzz(in);
    xyzz_add(acc, get_xyzz(in + 32));
    put_xyzz(out, acc);
  } else if constexpr (OP == 18) {
    XYZZ acc = get_xyzz(in);
    xyzz_add_mixed(acc, get_affine(in + 32), in[48] != 0);
    put_xyzz(out, acc);
  } else if constexpr (OP == 19) {
    put_xyzz(out, xyzz_double(get_xyzz(in)));
  } else if constexpr (OP == 20) {
    put_xyzz(out, xyzz_double_affine(get_affine(in)));
  } else if constexpr (OP == 21) {
    const XYZZ f = xyzz_from_affine(get_affine(in));
    put_xyzz(out, f);
    put_affine(out + 32, xyzz_to_affine(f));
  } else if constexpr (OP == 22) {
    put_affine(out, xyzz_to_affine(get_xyzz(in)));
  } else if constexpr (OP == 23) {
    put_xyzz(out, xyzz_mul(get_xyzz(in), get8(in + 32)));
  } else if constexpr (OP == 24) {
    XYZZ acc = get_xyzz(in);
    for (int s = 0; s < ECP_CHAIN; s++) {
      const uint32_t* q = in + 32 + 17 * s;
      xyzz_add_mixed(acc, get_affine(q), q[16] != 0);
      put_xyzz(out + 32 * s, acc);
    }
  }
}

template <class M, int OP>
__global__ __launch_bounds__(64) void k_eval(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  eval_hd<M, OP>(in + (size_t)t * NIN[OP], out + (size_t)t * NOUT[OP]);
}

static int hip_bad(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  fprintf(stderr, "ec_probe: %s: %s\n", what, hipGetErrorString(e));
  return 1;
}
template <class M, int OP>
static int run_device(const uint32_t* in, uint32_t* out, uint32_t n) {
  uint32_t *din = nullptr, *dout = nullptr;
  const size_t bi = (size_t)n * NIN[OP] * 4, bo = (size_t)n * NOUT[OP] * 4;
  int bad = hip_bad(hipMalloc(&din, bi), "hipMalloc") || hip_bad(hipMalloc(&dout, bo), "hipMalloc");
  bad = bad || hip_bad(hipMemcpy(din, in, bi, hipMemcpyHostToDevice), "hipMemcpy (in)");
  if (!bad) {
    hipLaunchKernelGGL((k_eval<M, OP>), dim3((n + 63) / 64), dim3(64), 0, 0, din, dout, n);
    bad = hip_bad(hipGetLastError(), "launch") || hip_bad(hipDeviceSynchronize(), "kernel");
  }
  bad = bad || hip_bad(hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost), "hipMemcpy (out)");
  if (din) bad = hip_bad(hipFree(din), "hipFree") || bad;
  if (dout) bad = hip_bad(hipFree(dout), "hipFree") || bad;
  return bad;
}
template <class M, int OP>
static int run_host(const uint32_t* in, uint32_t* out, uint32_t n) {
  for (uint32_t t = 0; t < n; t++) eval_hd<M, OP>(in + (size_t)t * NIN[OP], out + (size_t)t * NOUT[OP]);
  return 0;
}
template <int OP>
static int run_op(int op, bool device, uint32_t mod, const uint32_t* in, uint32_t* out, uint32_t n) {
  if constexpr (OP < ECP_NOPS) {
    if (op != OP) return run_op<OP + 1>(op, device, mod, in, out, n);
    if (OP == 6 && mod != 0) {
      fprintf(stderr, "ec_probe: op %d is over Fr\n", op);
      return 1;
    }
    if (OP >= ECP_FIRST_GROUP_OP && mod != 1) {
      fprintf(stderr, "ec_probe: op %d is over Fq\n", op);
      return 1;
    }
    if constexpr (OP == 6) {
      return device ? run_device<FrParams, OP>(in, out, n) : run_host<FrParams, OP>(in, out, n);
    } else if constexpr (OP >= ECP_FIRST_GROUP_OP) {
      return device ? run_device<FqParams, OP>(in, out, n) : run_host<FqParams, OP>(in, out, n);
    } else {
      if (device) return mod ? run_device<FqParams, OP>(in, out, n) : run_device<FrParams, OP>(in, out, n);
      return mod ? run_host<FqParams, OP>(in, out, n) : run_host<FrParams, OP>(in, out, n);
    }
  } else {
    fprintf(stderr, "ec_probe: unknown op %d\n", op);
    return 1;
  }
}

int main(int argc, char** argv) {
  if (argc != 4 || (strcmp(argv[1], "--host") && strcmp(argv[1], "--device"))) {
    fprintf(stderr, "usage: ec_probe --host|--device cases.bin out.bin\n");
    return 2;
  }
  const bool device = !strcmp(argv[1], "--device");
  FILE* f = fopen(argv[2], "rb");
  if (!f) {
    fprintf(stderr, "ec_probe: cannot read %s\n", argv[2]);
    return 2;
  }
  std::vector<uint32_t> in;
  {
    uint32_t buf[4096];
    size_t got;
    while ((got = fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(f);
  }
  if (in.size() < 2 || in[0] != ECP_MAGIC) {
    fprintf(stderr, "ec_probe: not a case file\n");
    return 2;
  }
  std::vector<uint32_t> out = {ECP_MAGIC, in[1]};
  size_t pos = 2;
  for (uint32_t b = 0; b < in[1]; b++) {
    if (pos + 3 > in.size()) {
      fprintf(stderr, "ec_probe: truncated case file (block %u)\n", b);
      return 2;
    }
    const uint32_t op = in[pos], mod = in[pos + 1], n = in[pos + 2];
    pos += 3;
    if (op >= ECP_NOPS || mod > 1 || n == 0 || (in.size() - pos) / NIN[op] < n) {
      fprintf(stderr, "ec_probe: bad block %u (op %u, field %u, %u cases)\n", b, op, mod, n);
      return 2;
    }
    out.push_back(op);
    out.push_back(mod);
    out.push_back(n);
    const size_t o0 = out.size();
    out.resize(o0 + (size_t)n * NOUT[op]);
    if (run_op<0>((int)op, device, mod, in.data() + pos, out.data() + o0, n)) return 1;
    pos += (size_t)n * NIN[op];
  }
  if (pos != in.size()) {
    fprintf(stderr, "ec_probe: %zu words after the last block\n", in.size() - pos);
    return 2;
  }
  f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) {
    fprintf(stderr, "ec_probe: cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
